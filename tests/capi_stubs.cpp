// capi_stubs.cpp -- stand-ins for every launcher fa2_capi.cpp calls (csrc/fa2_launch.h), for tests/test_capi_launches.py.
// Linked with the host-only object of fa2_capi.cpp into tests/_capi_stub/libfa2_capi_stub.so: a call through the C ABI then
// ends here instead of on a GPU, and each stub appends what it was handed to a text log, field by field (pointers as
// integers, floats as hex floats).  Nothing here calls the HIP runtime.
#include "../cuda_flashattention_amd/csrc/fa2_launch.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

namespace {

std::string g_log;
bool g_device_ok = true;

void put(const char* fmt, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_log += buf;
}
void begin(const char* name, hipStream_t s) { put("%s stream=%llx", name, (unsigned long long)(uintptr_t)s); }
void ptr(const char* n, const void* p) { put(" %s=%llx", n, (unsigned long long)(uintptr_t)p); }
void num(const char* n, long long v) { put(" %s=%lld", n, v); }
void flt(const char* n, float v) { put(" %s=%a", n, (double)v); }
hipError_t end() { g_log += ";"; return hipSuccess; }

void fwd(const fa2::FwdArgs& a)
{
    ptr("Q", a.Q); ptr("K", a.K); ptr("V", a.V); ptr("O", a.O); ptr("L", a.L); ptr("Oacc", a.Oacc); ptr("M", a.M);
    num("BH", a.BH); num("Nq", a.Nq); num("Nk", a.Nk); num("d", a.d); flt("scale", a.scale); num("causal", a.causal);
    num("shift", a.causal_shift); num("resume", a.resume); num("finalize", a.finalize); num("q_hs", a.q_hs); num("k_hs", a.k_hs);
    num("kv_group", a.kv_group); ptr("sink", a.sink); num("sink_heads", a.sink_heads);
}
void bwd(const fa2::BwdArgs& a)
{
    ptr("Q", a.Q); ptr("K", a.K); ptr("V", a.V); ptr("O", a.O); ptr("dO", a.dO); ptr("L", a.L); ptr("dQ", a.dQ); ptr("dK", a.dK);
    ptr("dV", a.dV); ptr("D", a.D); ptr("RC", a.RC); num("BH", a.BH); num("Nq", a.Nq); num("Nk", a.Nk); num("d", a.d);
    num("q_hs", a.q_hs); num("k_hs", a.k_hs); num("q_row0", a.q_row0); flt("scale", a.scale); num("causal", a.causal);
    num("shift", a.causal_shift); num("phases", a.phases); num("reserve_cus", a.reserve_cus); num("kv_group", a.kv_group);
}
void sinkgrad(const fa2::SinkGrad* sg)
{
    num("sg", sg != nullptr);
    if (sg) { ptr("sg.sink", sg->sink); ptr("sg.dsink", sg->dsink); num("sg.heads", sg->heads); ptr("sg.dL", sg->dL); }
}
void f32(const fa2::F32Args& a)
{
    ptr("Q", a.Q); ptr("K", a.K); ptr("V", a.V); ptr("O", a.O); ptr("L", a.L); ptr("dO", a.dO); ptr("dQ", a.dQ); ptr("dK", a.dK);
    ptr("dV", a.dV); ptr("D", a.D); num("BH", a.BH); num("N", a.N); num("d", a.d); flt("scale", a.scale); num("causal", a.causal);
    num("phases", a.phases); num("Nk", a.Nk); ptr("M", a.M); num("resume", a.resume); num("finalize", a.finalize);
}
void merge(const fa2::MergeArgs& a)
{
    for (int i = 0; i < fa2::kMergeMaxParts; ++i) { ptr("O", a.O[i]); ptr("L", a.L[i]); }
    num("n", a.n); ptr("Oout", a.Oout); ptr("Lout", a.Lout); num("rows", (long long)a.rows);
}

}  // namespace

extern "C" {
const char* fa2_stub_log(void) { return g_log.c_str(); }
void fa2_stub_reset(void) { g_log.clear(); }
void fa2_stub_set_device_ok(int ok) { g_device_ok = ok != 0; }
}

namespace fa2 {

// the three size functions: fixed stand-in formulas
size_t bwd_fused_ctl_bytes(int BH, int N) { return 1000 + 16 * (size_t)BH + (size_t)N; }
size_t bwd_fused_kvpart_bytes(int BH, int N, int d) { return (size_t)4 * BH * N * d; }
int decode_num_splits(int B, int H_kv, int kv_capacity) { return 2 + (B + H_kv + kv_capacity / 256) % 7; }

bool bwd_fused_device_ok(const char** why)
{
    if (!g_device_ok && why) *why = "two kernels: stub device";
    return g_device_ok;
}
hipError_t bwd_fused_read_error(const int* ctl, int* err, hipStream_t s)
{
    begin("read_error", s); ptr("ctl", ctl);
    *err = 0;
    return end();
}
hipError_t bwd_fused_clear_error(int* ctl, hipStream_t s) { begin("clear_error", s); ptr("ctl", ctl); return end(); }

hipError_t launch_fwd1_bf16(const FwdArgs& a, hipStream_t s) { begin("fwd1_bf16", s); fwd(a); return end(); }
hipError_t launch_fwd1_varlen_bf16(const VarlenFwdArgs& v, hipStream_t s)
{
    begin("fwd1_varlen_bf16", s); fwd(v.a); ptr("items", v.items); num("n_items", v.n_items);
    return end();
}
hipError_t launch_accumulate_bf16(float* acc, const void* src, size_t rows, size_t cols, size_t pitch, int init, hipStream_t s)
{
    begin("accumulate_bf16", s); ptr("acc", acc); ptr("src", src); num("rows", (long long)rows); num("cols", (long long)cols);
    num("pitch", (long long)pitch); num("init", init);
    return end();
}
hipError_t launch_finalize_state(const float* Oacc, const float* M, float* L, void* O, size_t rows, int d, hipStream_t s)
{
    begin("finalize_state", s); ptr("Oacc", Oacc); ptr("M", M); ptr("L", L); ptr("O", O); num("rows", (long long)rows); num("d", d);
    return end();
}
hipError_t launch_merge_fwd(const MergeArgs& a, int d, hipStream_t s) { begin("merge_fwd", s); merge(a); num("d", d); return end(); }
hipError_t launch_merge_bwd(const MergeBwdArgs& b, int d, hipStream_t s)
{
    begin("merge_bwd", s); merge(b.m); ptr("dO", b.dO); ptr("dL", b.dL);
    for (int i = 0; i < kMergeMaxParts; ++i) { ptr("dO_part", b.dO_parts[i]); ptr("dL_part", b.dL_parts[i]); }
    num("d", d);
    return end();
}
hipError_t launch_decode(const DecodeArgs& a, int d, hipStream_t s)
{
    begin("decode", s); ptr("Q", a.Q); ptr("K", a.K); ptr("V", a.V); ptr("seqlens", a.seqlens); ptr("sink", a.sink); ptr("O", a.O);
    ptr("L", a.L); ptr("wsO", a.wsO); ptr("wsL", a.wsL); num("B", a.B); num("Hq", a.Hq); num("Hkv", a.Hkv); num("Nq", a.Nq);
    num("Ncap", a.Ncap); num("n_splits", a.n_splits); flt("scale", a.scale); num("causal", a.causal); num("d", d);
    return end();
}
hipError_t launch_fwd_fp8(const FwdFp8Args& a, hipStream_t s)
{
    begin("fwd_fp8", s); ptr("Q", a.Q); ptr("K", a.K); ptr("V", a.V); ptr("Vt", a.Vt); ptr("kn", a.kn); ptr("O", a.O); ptr("L", a.L);
    num("BH", a.BH); num("N", a.N); num("Npad", a.Npad); num("d", a.d); flt("scale", a.scale); num("causal", a.causal);
    flt("o_scale", a.o_scale);
    return end();
}
hipError_t launch_bwd_bf16(const BwdArgs& a, hipStream_t s, const SinkGrad* sg) { begin("bwd_bf16", s); bwd(a); sinkgrad(sg); return end(); }
hipError_t launch_bwd_varlen_bf16(const VarlenBwdArgs& v, hipStream_t s, const SinkGrad* sg)
{
    begin("bwd_varlen_bf16", s); bwd(v.a); ptr("row_items", v.row_items); ptr("key_items", v.key_items);
    num("n_row_items", v.n_row_items); num("n_key_items", v.n_key_items); sinkgrad(sg);
    return end();
}
hipError_t launch_bwd_fused_bf16(const BwdArgs& a, float* dQacc, int* ctl, int mode, hipStream_t s, float* rcpad, void* kvpart,
                                 const SinkGrad* sg)
{
    begin("bwd_fused_bf16", s); bwd(a); ptr("dQacc", dQacc); ptr("ctl", ctl); num("mode", mode); ptr("rcpad", rcpad);
    ptr("kvpart", kvpart); sinkgrad(sg);
    return end();
}
hipError_t launch_fwd_f32(const F32Args& a, hipStream_t s) { begin("fwd_f32", s); f32(a); return end(); }
hipError_t launch_bwd_f32(const F32Args& a, hipStream_t s) { begin("bwd_f32", s); f32(a); return end(); }
hipError_t launch_fa1_f32(const float* Q, const float* K, const float* V, float* O, float* l, float* m, int N, int d, int Bc,
                          hipStream_t s)
{
    begin("fa1_f32", s); ptr("Q", Q); ptr("K", K); ptr("V", V); ptr("O", O); ptr("l", l); ptr("m", m); num("N", N); num("d", d);
    num("Bc", Bc);
    return end();
}
hipError_t launch_fill_f32(float* p, size_t n, float value, hipStream_t s)
{
    begin("fill_f32", s); ptr("p", p); num("n", (long long)n); flt("value", value);
    return end();
}
hipError_t launch_mfma_probe(const void* in, float* out, int iters, int blocks, hipStream_t s)
{
    begin("mfma_probe", s); ptr("in", in); ptr("out", out); num("iters", iters); num("blocks", blocks);
    return end();
}
hipError_t launch_f32_to_bf16(const float* src, void* dst, size_t n, hipStream_t s)
{
    begin("f32_to_bf16", s); ptr("src", src); ptr("dst", dst); num("n", (long long)n);
    return end();
}
hipError_t launch_bf16_to_f32(const void* src, float* dst, size_t n, hipStream_t s)
{
    begin("bf16_to_f32", s); ptr("src", src); ptr("dst", dst); num("n", (long long)n);
    return end();
}
hipError_t launch_read_clocks(unsigned long long* out, hipStream_t s) { begin("read_clocks", s); ptr("out", out); return end(); }

}  // namespace fa2
