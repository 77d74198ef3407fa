// fa2_capi.cpp -- the C ABI of libfa2_mi355x.so (include/fa2_mi355x.h): argument checking,
// status codes and dispatch.  No kernels here and no framework types; the host wrappers of
// the reference (flash_attention_kernel.cu:300-343, flash_attention_backward_kernel.cu:249-299)
// become these functions.
#include "../../include/fa2_mi355x.h"
#include <cstdlib>
#include <cstring>

#include "fa2_launch.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <numeric>
#include <vector>

namespace {

inline int hip_status(hipError_t e) { return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e; }

// The kernels address one head slab through a buffer resource (32-bit byte count, 32-bit byte offsets): a slab of N
// rows must stay below 2 GiB (at 4 bytes per element, the widest type).  Larger problems get a status, not a silent
// wrap-around.
inline int check_common(int B, int H, int N, int d, float scale)
{
    if (B <= 0 || H <= 0 || N <= 0 || d <= 0) return FA2_ERR_INVALID_SHAPE;
    if (!(scale > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    if ((long long)B * H > 0x7fffffffLL / 64) return FA2_ERR_INVALID_SHAPE;
    if ((long long)N * d * 4 > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    return FA2_OK;
}

// bf16 backward only: its two row-constant planes (B H rows floats each) sit behind ONE buffer resource.  The single-kernel
// form builds that resource (and its int offsets) on the length PADDED to a multiple of 256 (fa2_bwd_fused.hip: rc_rsrc,
// rcoff), so the padded length is what must fit -- for every shape: the 255 rows of slack cost nobody a legitimate problem.
inline int check_bwd_planes(int B, int H, int rows)
{
    const long long padded = ((long long)rows + 255) / 256 * 256;
    return (long long)B * H * padded * 8 > 0x7fffffffLL ? FA2_ERR_INVALID_SHAPE : FA2_OK;
}

// what the bf16-only entry points report: head_dim first, whatever the dtype
inline int check_bf16(int head_dim, int dtype)
{
    if (head_dim != 64 && head_dim != 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    return dtype == FA2_DTYPE_BF16 ? FA2_OK : FA2_ERR_UNSUPPORTED_DTYPE;
}

inline int check_dim(int d, int dtype)
{
    if (dtype == FA2_DTYPE_BF16) return check_bf16(d, dtype);
    if (dtype == FA2_DTYPE_F32) return (d >= 1 && d <= 128) ? FA2_OK : FA2_ERR_UNSUPPORTED_HEAD_DIM;
    if (dtype == FA2_DTYPE_FP8_E4M3) return d == 128 ? FA2_OK : FA2_ERR_UNSUPPORTED_HEAD_DIM;
    return FA2_ERR_UNSUPPORTED_DTYPE;
}

// Grow-only per-device scratch for the reference-signature backward, which has no workspace
// argument (the reference cudaMemsets inside its wrapper too, :282-283).
struct ScratchCache {
    std::mutex mu;
    void* ptr[64] = {};
    size_t cap[64] = {};
    int get(size_t bytes, void** out)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return hip_status(e);
        if (dev < 0 || dev >= 64) return FA2_ERR_UNSUPPORTED;
        std::lock_guard<std::mutex> g(mu);
        if (cap[dev] < bytes) {
            if (ptr[dev]) {
                e = hipDeviceSynchronize();      // nothing may still be using the old block
                if (e != hipSuccess) return hip_status(e);
                (void)hipFree(ptr[dev]);
                ptr[dev] = nullptr; cap[dev] = 0;
            }
            e = hipMalloc(&ptr[dev], bytes);
            if (e != hipSuccess) return hip_status(e);
            cap[dev] = bytes;
        }
        *out = ptr[dev];
        return FA2_OK;
    }
} g_scratch;

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The plan of a packed variable-length batch (fa2_varlen_plan_build): this header, the row-block items, the key-block items.
// total / max_len: the query side's rows and longest sequence; total_k: 0 in a one-sided plan (one list for both sides), the key
// side's rows (>= 1) in a two-sided one (fa2_varlen_plan_build_qk with a key list of its own).
struct VarlenHeader { int magic, version, n_seqs, total, n_row_items, n_key_items, max_len, total_k; };
constexpr int kVarlenMagic = 0x4c564146;      // "FAVL"
constexpr int kVarlenVersion = 1;
constexpr int kVarlenBlock = 256;             // rows per row-block item = keys per key-block item (kF1Rows, kBwdRows, kDkKeys)
constexpr int kVarlenMaxRows = 0x7fffffff / (128 * 4);      // check_common's plane rule at the widest row (head_dim 128, 4 bytes)
inline size_t varlen_bytes(long long n_row, long long n_key)
{
    return sizeof(VarlenHeader) + (size_t)(n_row + n_key) * sizeof(fa2::VarlenItem);
}

// What a launch believes of the HOST copy of a plan (nothing of the device copy is read on the host)
// one_list: asked by a one-list entry point, which refuses a two-sided plan (it would read K as T_q rows).  The _qk calls take
// both kinds; a one-sided plan has as many key rows as query rows.
inline int varlen_check(const void* plan_host, const void* plan_dev, size_t plan_bytes, int total_rows, int total_k, bool one_list,
                        int heads, VarlenHeader* out)
{
    if (plan_bytes < sizeof(VarlenHeader) || ((uintptr_t)plan_dev & 3)) return FA2_ERR_INVALID_SHAPE;
    VarlenHeader h;
    memcpy(&h, plan_host, sizeof h);
    if (h.magic != kVarlenMagic || h.version != kVarlenVersion) return FA2_ERR_INVALID_SHAPE;
    if (h.total != total_rows || h.n_row_items < 1 || h.n_key_items < 1 || h.total_k < 0) return FA2_ERR_INVALID_SHAPE;
    if (one_list ? h.total_k != 0 : (h.total_k ? h.total_k : h.total) != total_k) return FA2_ERR_INVALID_SHAPE;
    if (plan_bytes < varlen_bytes(h.n_row_items, h.n_key_items)) return FA2_ERR_INVALID_SHAPE;
    if ((long long)std::max(h.n_row_items, h.n_key_items) * heads > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;      // the grid
    *out = h;
    return FA2_OK;
}

// The public entry point that asks: the order in which faults are reported is the asking entry point's (the backward ones
// through bwd_route, the forward and packed ones through check_request).
enum class Entry { phases, qk, block, fused, status, plan, forward_gqa, forward_qk, forward_packed, backward_packed };

// What a caller asked for, whichever entry point it came through.  A packed call is one batch (B = 1) of q_len = T_q query and
// kv_len = T_k key rows with a plan.  A new per-problem option is a field here, a rule in check_request (or bwd_route) and a
// field of the kernel's struct in fa2_launch.h.
struct Request {
    int B = 1, H = 0, kv_heads = 0;      // kv_heads 0: an entry point without grouped heads (as many K/V heads as query heads)
    int q_len = 0, kv_len = 0, q_stride = 0, kv_stride = 0, q_row0 = 0;      // strides 0: dense slabs of q_len / kv_len rows
    int head_dim = 0, dtype = FA2_DTYPE_BF16;
    float scale = 1.0f;
    int causal = 0, shift = 0, phases = 0;
    const void* ws = nullptr; size_t ws_bytes = 0;
    const float* sink = nullptr; float* dsink = nullptr; const float* dL = nullptr;
    bool need_sinks = false;      // fa2_backward_sink and its packed form: sink and dsink, both (otherwise: both or neither)
    const void *plan_host = nullptr, *plan_dev = nullptr; size_t plan_bytes = 0; bool one_list = false;
    bool ws_short(size_t need) const { return !ws || ws_bytes < need; }
};

// (H_kv = 0 from a grouped entry point must not read as "no grouped heads": -1 is as invalid)
inline int grouped(int H_kv) { return H_kv ? H_kv : -1; }
inline bool heads_divide(int H_q, int H_kv) { return H_kv > 0 && H_q % H_kv == 0; }

// The checks of every grouped bf16 entry point, in the order its rung of the interface reports them: fa2_forward_gqa the dtype
// before the head_dim, everything after it the head_dim first; the packed calls their plan (-> *plan) in between.
inline int check_request(Entry entry, const Request& q, VarlenHeader* plan = nullptr)
{
    int st = check_common(q.B, q.H, q.q_len, q.head_dim, q.scale);
    if (!st) st = check_common(q.B, q.H, q.kv_len, q.head_dim, q.scale);
    if (st) return st;
    if (!heads_divide(q.H, q.kv_heads)) return FA2_ERR_INVALID_SHAPE;
    if (entry == Entry::backward_packed && (st = check_bwd_planes(q.B, q.H, q.q_len))) return st;
    if (plan && (st = varlen_check(q.plan_host, q.plan_dev, q.plan_bytes, q.q_len, q.kv_len, q.one_list, q.H, plan))) return st;
    if (entry == Entry::forward_gqa && q.dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    return check_bf16(q.head_dim, q.dtype);
}

}  // namespace

extern "C" {

// The compiler that produced the code objects is part of the version: the kernels pin registers and count
// wait states by hand, and tests/test_isa_guard.py re-checks the generated code whenever this string changes.
#define FA2_STR2(x) #x
#define FA2_STR(x) FA2_STR2(x)
const char* fa2_version(void)
{
    return "fa2_mi355x 0.2 (gfx950; hip " FA2_STR(HIP_VERSION_MAJOR) "." FA2_STR(HIP_VERSION_MINOR) "." FA2_STR(HIP_VERSION_PATCH)
           "; clang " __clang_version__ ")";
}

const char* fa2_status_string(int s)
{
    switch (s) {
    case FA2_OK: return "ok";
    case FA2_ERR_NULL_POINTER: return "null pointer";
    case FA2_ERR_INVALID_SHAPE: return "invalid shape or scale";
    case FA2_ERR_UNSUPPORTED_HEAD_DIM: return "unsupported head_dim";
    case FA2_ERR_UNSUPPORTED_DTYPE: return "unsupported dtype";
    case FA2_ERR_WORKSPACE: return "workspace missing or too small";
    case FA2_ERR_UNSUPPORTED: return "unsupported combination";
    case FA2_ERR_HANDOFF_TIMEOUT: return "single-kernel backward: a bounded wait for the previous key block ran out (dQ is NaN)";
    default: break;
    }
    if (s <= FA2_ERR_RCCL_BASE) return "RCCL error (code = -(status) - 2000)";
    if (s <= FA2_ERR_HIP_BASE) return hipGetErrorString((hipError_t)(FA2_ERR_HIP_BASE - s));
    return "unknown status";
}

// Every bf16 forward but the resumable steps: the checks in the order of the asking entry point, then the dense launch or
// (Entry::forward_packed, with a plan) the packed one.  Dense: the causal mask is aligned bottom-right, key j visible to query i
// iff j <= i + kv_len - q_len.
struct FwdTensors { const void *Q, *K, *V; void* O; float* L; };
static int forward_bf16(Entry entry, const FwdTensors& t, const Request& q, void* stream)
{
    const bool packed = entry == Entry::forward_packed;
    if (!t.Q || !t.K || !t.V || !t.O || !t.L || (packed && (!q.plan_host || !q.plan_dev))) return FA2_ERR_NULL_POINTER;
    VarlenHeader h;
    if (const int st = check_request(entry, q, packed ? &h : nullptr)) return st;
    fa2::VarlenFwdArgs v{};
    fa2::FwdArgs& a = v.a;
    a.Q = t.Q; a.K = t.K; a.V = t.V; a.O = t.O; a.L = t.L;
    a.BH = q.B * q.H; a.d = q.head_dim; a.scale = q.scale; a.causal = q.causal ? 1 : 0; a.finalize = 1;
    a.kv_group = q.H / q.kv_heads; a.sink = q.sink; a.sink_heads = q.H;
    if (!packed) {
        a.Nq = q.q_len; a.Nk = q.kv_len; a.causal_shift = q.causal ? a.Nk - a.Nq : 0;
        return hip_status(fa2::launch_fwd1_bf16(a, (hipStream_t)stream));
    }
    a.q_hs = q.q_len; a.k_hs = q.kv_len;      // Nq, Nk and the mask's shift are per item
    v.items = reinterpret_cast<const fa2::VarlenItem*>((const char*)q.plan_dev + sizeof(VarlenHeader));
    v.n_items = h.n_row_items;
    return hip_status(fa2::launch_fwd1_varlen_bf16(v, (hipStream_t)stream));
}

int fa2_forward(const void* Q, const void* K, const void* V, void* O, float* L,
                int B, int H, int seq_len, int head_dim, float softmax_scale,
                int dtype, int causal, void* stream)
{
    if (dtype == FA2_DTYPE_BF16)      // fa2_forward_gqa's problem with as many K/V heads as query heads, and its checks
        return forward_bf16(Entry::forward_gqa, {Q, K, V, O, L}, {.B = B, .H = H, .kv_heads = H, .q_len = seq_len, .kv_len = seq_len,
                            .head_dim = head_dim, .scale = softmax_scale, .causal = causal}, stream);
    if (!Q || !K || !V || !O || !L) return FA2_ERR_NULL_POINTER;
    int st = check_common(B, H, seq_len, head_dim, softmax_scale);
    if (st) return st;
    st = check_dim(head_dim, dtype);
    if (st) return st;
    if (dtype == FA2_DTYPE_FP8_E4M3) {      // workspace from the stream-ordered allocator
        const size_t need = fa2_forward_fp8_workspace_bytes(B, H, seq_len, head_dim);
        void* ws = nullptr;
        hipError_t e = hipMallocAsync(&ws, need, (hipStream_t)stream);
        if (e != hipSuccess) return hip_status(e);
        st = fa2_forward_fp8(Q, K, V, O, L, B, H, seq_len, head_dim, softmax_scale, causal, ws, need, stream);
        e = hipFreeAsync(ws, (hipStream_t)stream);
        return st ? st : hip_status(e);
    }
    fa2::F32Args a{};
    a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V; a.O = (float*)O; a.L = L;
    a.BH = B * H; a.N = seq_len; a.d = head_dim; a.scale = softmax_scale; a.causal = causal ? 1 : 0;
    a.Nk = seq_len; a.M = nullptr; a.resume = 0; a.finalize = 1;
    return hip_status(fa2::launch_fwd_f32(a, (hipStream_t)stream));
}

int fa2_forward_gqa(const void* Q, const void* K, const void* V, void* O, float* L,
                    int B, int H_q, int H_kv, int seq_len, int head_dim, float softmax_scale,
                    int dtype, int causal, void* stream)
{
    return forward_bf16(Entry::forward_gqa, {Q, K, V, O, L}, {.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = seq_len,
                        .kv_len = seq_len, .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal}, stream);
}

// ---- packed variable-length batches ---------------------------------------------------------------------------------------
size_t fa2_varlen_plan_bytes(int n_seqs, int total_rows) { return fa2_varlen_plan_bytes_qk(n_seqs, total_rows, total_rows); }

size_t fa2_varlen_plan_bytes_qk(int n_seqs, int total_q, int total_k)
{
    if (n_seqs < 1 || total_q < 1 || total_k < 1) return 0;
    // a sequence of len rows has ceil(len / 256) <= len / 256 + 1 blocks, and only non-empty sequences have any
    const long long n_row = (long long)total_q / kVarlenBlock + std::min(n_seqs, total_q);
    const long long n_key = (long long)total_k / kVarlenBlock + std::min(n_seqs, total_k);
    return varlen_bytes(n_row, n_key);
}

int fa2_varlen_plan_build(const int* cu_seqlens_host, int n_seqs, void* plan_host, size_t plan_bytes)
{
    return fa2_varlen_plan_build_qk(cu_seqlens_host, nullptr, n_seqs, plan_host, plan_bytes);
}

int fa2_varlen_plan_build_qk(const int* cu_seqlens_q_host, const int* cu_seqlens_k_host, int n_seqs, void* plan_host, size_t plan_bytes)
{
    const int *cq = cu_seqlens_q_host, *ck = cu_seqlens_k_host;
    if (!cq || !plan_host) return FA2_ERR_NULL_POINTER;
    if (n_seqs < 1) return FA2_ERR_INVALID_SHAPE;
    // no key list, or the query list again: the one-sided plan -- the two-sided plan of (cq, cq) with total_k = 0 in its header
    const bool one_sided = !ck || std::equal(cq, cq + n_seqs + 1, ck);
    if (one_sided) ck = cq;
    for (const int* cu : {cq, ck}) {
        if (cu[0] != 0) return FA2_ERR_INVALID_SHAPE;
        for (int i = 0; i < n_seqs; ++i)
            if (cu[i + 1] < cu[i]) return FA2_ERR_INVALID_SHAPE;
        if (cu[n_seqs] < 1 || cu[n_seqs] > kVarlenMaxRows) return FA2_ERR_INVALID_SHAPE;
    }
    const auto len_q = [&](int i) { return cq[i + 1] - cq[i]; };
    const auto len_k = [&](int i) { return ck[i + 1] - ck[i]; };
    const auto blocks = [](int len) { return (len + kVarlenBlock - 1) / kVarlenBlock; };
    // sequences by descending work (len_q x len_k), ties by index: by descending length in a one-sided plan.  A sequence
    // with one empty side has no product to form but still has outputs to write (O = 0, L = -inf; dK = dV = 0): it comes last
    std::vector<int> order(n_seqs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return (long long)len_q(a) * len_k(a) > (long long)len_q(b) * len_k(b); });
    long long n_row = 0, n_key = 0;
    int max_len = 0;
    for (int i = 0; i < n_seqs; ++i) {
        n_row += blocks(len_q(i));
        n_key += blocks(len_k(i));
        max_len = std::max(max_len, len_q(i));
    }
    if (plan_bytes < varlen_bytes(n_row, n_key)) return FA2_ERR_WORKSPACE;
    const VarlenHeader h{kVarlenMagic, kVarlenVersion, n_seqs, cq[n_seqs], (int)n_row, (int)n_key, max_len, one_sided ? 0 : ck[n_seqs]};
    memcpy(plan_host, &h, sizeof h);
    // (written through memcpy: the caller's buffer has no alignment beyond a byte's)
    char* out = (char*)plan_host + sizeof h;
    const auto put = [&](int seq, int block) {
        const fa2::VarlenItem it{cq[seq], ck[seq], len_q(seq), len_k(seq), block};
        memcpy(out, &it, sizeof it);
        out += sizeof it;
    };
    for (int seq : order)      // row blocks of every sequence with a query (len_k = 0 included), descending within a sequence
        for (int b = blocks(len_q(seq)) - 1; b >= 0; --b) put(seq, b);      // (the heaviest first under a causal mask)
    for (int seq : order)      // key blocks of every sequence with a key (len_q = 0 included), ascending (block 0 is the heaviest)
        for (int b = 0; b < blocks(len_k(seq)); ++b) put(seq, b);
    return FA2_OK;
}

int fa2_forward_qk(const void* Q, const void* K, const void* V, void* O, float* L,
                   int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                   int dtype, int causal, void* stream)
{
    return forward_bf16(Entry::forward_qk, {Q, K, V, O, L}, {.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = q_len, .kv_len = kv_len,
                        .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal}, stream);
}

// ---- attention sinks: the _qk problems with one learned logit per query head in every row's softmax (include/fa2_mi355x.h)
int fa2_forward_sink(const void* Q, const void* K, const void* V, const float* sink, void* O, float* L,
                     int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                     int dtype, int causal, void* stream)
{
    if (!sink) return FA2_ERR_NULL_POINTER;
    return forward_bf16(Entry::forward_qk, {Q, K, V, O, L}, {.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = q_len, .kv_len = kv_len,
                        .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal, .sink = sink}, stream);
}

// the packed forward entry points (one_list: fa2_forward_varlen, one T for both sides, which refuses a two-sided plan)
int fa2_forward_varlen(const void* Q, const void* K, const void* V, void* O, float* L,
                       int H_q, int H_kv, int total_rows, int head_dim, float softmax_scale, int dtype, int causal,
                       const void* plan_host, const void* plan_dev, size_t plan_bytes, void* stream)
{
    return forward_bf16(Entry::forward_packed, {Q, K, V, O, L}, {.H = H_q, .kv_heads = grouped(H_kv), .q_len = total_rows,
                        .kv_len = total_rows, .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal,
                        .plan_host = plan_host, .plan_dev = plan_dev, .plan_bytes = plan_bytes, .one_list = true}, stream);
}

int fa2_forward_varlen_qk(const void* Q, const void* K, const void* V, void* O, float* L,
                          int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                          const void* plan_host, const void* plan_dev, size_t plan_bytes, void* stream)
{
    return forward_bf16(Entry::forward_packed, {Q, K, V, O, L}, {.H = H_q, .kv_heads = grouped(H_kv), .q_len = total_q,
                        .kv_len = total_k, .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal,
                        .plan_host = plan_host, .plan_dev = plan_dev, .plan_bytes = plan_bytes}, stream);
}

int fa2_forward_varlen_sink(const void* Q, const void* K, const void* V, const float* sink, void* O, float* L,
                            int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                            const void* plan_host, const void* plan_dev, size_t plan_bytes, void* stream)
{
    if (!sink) return FA2_ERR_NULL_POINTER;
    return forward_bf16(Entry::forward_packed, {Q, K, V, O, L}, {.H = H_q, .kv_heads = grouped(H_kv), .q_len = total_q,
                        .kv_len = total_k, .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal,
                        .sink = sink, .plan_host = plan_host, .plan_dev = plan_dev, .plan_bytes = plan_bytes}, stream);
}

size_t fa2_forward_fp8_workspace_bytes(int B, int H, int seq_len, int head_dim)
{
    if (B <= 0 || H <= 0 || seq_len <= 0 || head_dim != 128) return 0;
    const size_t npad = ((size_t)seq_len + 63) / 64 * 64;
    return (size_t)B * H * head_dim * npad + (size_t)B * H * (npad / 64) * sizeof(float);      // V^T | key-norm maxima (npad % 64 == 0: aligned)
}

int fa2_forward_fp8(const void* Q, const void* K, const void* V, void* O, float* L,
                    int B, int H, int seq_len, int head_dim, float softmax_scale, int causal,
                    void* workspace, size_t workspace_bytes, void* stream)
{
    return fa2_forward_fp8_scaled(Q, K, V, O, L, B, H, seq_len, head_dim, softmax_scale, 1.0f, 1.0f, 1.0f, causal, workspace,
                                  workspace_bytes, stream);
}

int fa2_forward_fp8_scaled(const void* Q, const void* K, const void* V, void* O, float* L,
                           int B, int H, int seq_len, int head_dim, float softmax_scale,
                           float q_descale, float k_descale, float v_descale, int causal,
                           void* workspace, size_t workspace_bytes, void* stream)
{
    if (!Q || !K || !V || !O || !L) return FA2_ERR_NULL_POINTER;
    if (!(q_descale > 0.0f) || !(k_descale > 0.0f) || !(v_descale > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    if (!std::isfinite(q_descale) || !std::isfinite(k_descale) || !std::isfinite(v_descale)) return FA2_ERR_INVALID_SHAPE;      // +inf
    int st = check_common(B, H, seq_len, head_dim, softmax_scale);
    if (st) return st;
    // scores are formed from the STORED values: the two descales belong to the softmax scale (the lazy reference, its
    // thresholds and the key-norm bound are all in units of that product); V's multiplies O once, in the epilogue
    softmax_scale *= q_descale * k_descale;
    if (!(softmax_scale > 0.0f) || !(softmax_scale < 3.0e38f)) return FA2_ERR_INVALID_SHAPE;
    st = check_dim(head_dim, FA2_DTYPE_FP8_E4M3);
    if (st) return st;
    if (!workspace || workspace_bytes < fa2_forward_fp8_workspace_bytes(B, H, seq_len, head_dim)) return FA2_ERR_WORKSPACE;
    fa2::FwdFp8Args a{};
    a.Q = Q; a.K = K; a.V = V; a.Vt = workspace; a.O = O; a.L = L;
    a.BH = B * H; a.N = seq_len; a.Npad = (seq_len + 63) / 64 * 64; a.d = head_dim;
    a.kn = reinterpret_cast<float*>((char*)workspace + (size_t)a.BH * head_dim * a.Npad);
    a.scale = softmax_scale; a.causal = causal ? 1 : 0; a.o_scale = v_descale;
    return hip_status(fa2::launch_fwd_fp8(a, (hipStream_t)stream));
}

// shapes the single-kernel (five-product) backward takes: csrc/fa2_bwd_fused.hip.  Any seq_len: its loops run on the length
// rounded up to a multiple of 256 (keys past the end are masked, rows past the end get row constants that make P vanish), so
// it is taken whenever that padding costs less than the two extra block products of the two-kernel form (64-key tiles), and
// at head_dim 64, where it is ~10 % ahead of the two kernels (half the MFMAs beside the same VALU and hand-off work), whenever
// the padding costs under 7 %.  The sets these inequalities give: include/fa2_mi355x.h, fa2_backward.
static int fused_npad(int n) { return (n + 255) / 256 * 256; }
static bool bwd_fused_shape(int seq_len, int head_dim, int dtype)
{
    if (dtype != FA2_DTYPE_BF16 || seq_len < 1) return false;
    const long long np = fused_npad(seq_len), n64 = (seq_len + 63) / 64 * 64;
    if (head_dim == 64) return 13 * np <= 14 * n64 && np * 128 * 4 <= 0x7fffffffLL;
    if (head_dim != 128) return false;
    return 5 * np <= 7 * n64 && np * head_dim * 4 <= 0x7fffffffLL;
}

// The backward workspace for `rows` rows per head (a block's q_head_stride), each part 256-byte aligned: D [BH][rows] | RC
// [2][BH][rows] (-L/scale, -D) | then, where the single kernel takes the shape (`single`), its fp32 dQ sums [BH][NP][128]
// (128 floats per row at either head_dim) | control block | (ragged rows only) RC padded to NP rows (NP = roundup(rows, 256)) |
// (grouped-query attention, kv_group > 1, only) the single kernel's per-query-head dK / dV partials, bf16 [2][BH][rows][head_dim].
// The partials come LAST: everything in front of them lies where it lies for the multi-head problem (B, H, rows, head_dim), so
// fa2_backward_status finds the control block of a grouped launch with those four numbers.
struct BwdWs { bool single; float *D, *RC, *acc; int* ctl; float* rcpad; size_t base_bytes, bytes; void* kvpart; };
static BwdWs bwd_ws(const void* base, int B, int H, int rows, int head_dim, int dtype, int kv_group = 1)
{
    const int np = fused_npad(rows);
    const bool single = bwd_fused_shape(rows, head_dim, dtype);
    const size_t plane = align256((size_t)B * H * rows * sizeof(float)), acc = align256((size_t)B * H * np * 128 * 4);
    const size_t ctl = single ? align256(fa2::bwd_fused_ctl_bytes(B * H, np)) : 0;
    const size_t pad = np != rows ? align256((size_t)2 * B * H * np * 4) : 0;
    char* b = (char*)const_cast<void*>(base);
    const size_t mha = 3 * plane + (single ? acc + ctl + pad : 0);
    const size_t part = single && kv_group > 1 ? align256(fa2::bwd_fused_kvpart_bytes(B * H, rows, head_dim)) : 0;
    return BwdWs{single, (float*)b, (float*)(b + plane), (float*)(b + 3 * plane), (int*)(b + 3 * plane + acc),
                 pad ? (float*)(b + 3 * plane + acc + ctl) : nullptr, 3 * plane, mha + part, part ? b + mha : nullptr};
}

// FA2_BACKWARD_PATH=two_kernel keeps fa2_backward on the two deterministic kernels for every shape (A/B runs, triage)
static bool bwd_fused_allowed()
{
    static const bool allowed = [] {
        const char* e = getenv("FA2_BACKWARD_PATH");
        return !(e && strcmp(e, "two_kernel") == 0);
    }();
    return allowed;
}

enum class Path { none, f32, two_kernel, single };
struct Route {
    int status = FA2_OK;
    Path path = Path::none;
    int mode = 1;                 // single: 0 = dQ by fp32 atomics, 1 = the ordered hand-off
    bool clear_error = false;     // two kernels on a workspace with a control block: its error word must describe this call
    fa2::BwdArgs args{};
    BwdWs ws{};
    const char* why = "";         // fa2_backward_plan's reason
};

static bool any_null(const fa2::BwdArgs& t) { return !t.Q || !t.K || !t.V || !t.O || !t.L || !t.dO || !t.dQ || !t.dK || !t.dV; }

// The arguments of a bf16 backward launch, dense or packed, from its nine tensors `t`, the request and the workspace's planes
// (phases and reserve_cus are the caller's)
static void bwd_args(fa2::BwdArgs& a, const fa2::BwdArgs& t, const Request& q, const BwdWs& ws)
{
    a.Q = t.Q; a.K = t.K; a.V = t.V; a.O = t.O; a.dO = t.dO; a.L = t.L; a.dQ = t.dQ; a.dK = t.dK; a.dV = t.dV;
    a.D = ws.D; a.RC = ws.RC; a.BH = q.B * q.H; a.Nq = q.q_len; a.Nk = q.kv_len; a.d = q.head_dim;
    a.q_hs = q.q_stride ? q.q_stride : q.q_len; a.k_hs = q.kv_stride ? q.kv_stride : q.kv_len; a.q_row0 = q.q_row0;
    a.scale = q.scale; a.causal = q.causal ? 1 : 0; a.causal_shift = q.causal ? q.shift : 0;
    a.kv_group = q.kv_heads > 0 ? q.H / q.kv_heads : 1;
}

// Where every DENSE backward is routed (the rule: include/fa2_mi355x.h, fa2_backward): validation in the order of the asking
// entry point, then what to run, its arguments and its workspace.  The packed backward (backward_varlen) has one implementation
// and nothing to route: it shares check_request and bwd_args with this.  `t` holds the nine tensors (none for status and plan);
// q.phases is fa2_backward_fused's mode.  q.kv_heads != 0 comes from the grouped-query entry points (phases, qk and plan only), is
// validated here and changes nothing about WHICH implementation runs -- rule (a) depends on seq_len and head_dim alone.
static Route bwd_route(Entry entry, const fa2::BwdArgs& t, const Request& q)
{
    Route r;
    const auto fail = [&r](int st) { r.status = st; return r; };
    const auto device_ok = [&r] { return fa2::bwd_fused_device_ok(&r.why); };
    const auto env_and_device_ok = [&] { return bwd_fused_allowed() && device_ok(); };      // rules (b) and (c)
    if (entry <= Entry::fused && any_null(t)) return fail(FA2_ERR_NULL_POINTER);
    const int B = q.B, H = q.H, q_len = q.q_len, kv_len = q.kv_len, d = q.head_dim, dtype = q.dtype, phases = q.phases;
    const int q_hs = q.q_stride ? q.q_stride : q_len, k_hs = q.kv_stride ? q.kv_stride : kv_len;
    const bool gqa = q.kv_heads != 0;           // asked through a grouped-query entry point (bf16 only, whatever the group size)
    switch (entry) {
    case Entry::qk:          // fa2_backward_qk: q_len queries against kv_len keys, grouped or not, bf16
        if ((r.status = check_request(entry, q))) return r;
        if (q_len != kv_len) {      // a rectangle: the two deterministic kernels, whatever the shape
            if ((r.status = check_bwd_planes(B, H, q_len))) return r;
            r.ws = bwd_ws(q.ws, B, H, q_len, d, dtype);      // D and the two row-constant planes over [B][H][q_len], nothing else
            r.ws.single = false; r.ws.bytes = r.ws.base_bytes;
            if (q.ws_short(r.ws.bytes)) return fail(FA2_ERR_WORKSPACE);
            if (phases & 8) return fail(FA2_ERR_UNSUPPORTED);      // the single kernel takes no rectangle here
            r.path = Path::two_kernel; r.args.phases = phases & 7;
            break;
        }
        [[fallthrough]];     // equal lengths: fa2_backward_gqa's problem -- its rule, its workspace, its launches
    case Entry::phases:      // phases: 1 = D and the row constants, 2 = dQ kernel, 4 = dK/dV kernel, 8 = the single kernel
        if ((r.status = check_common(B, H, q_len, d, q.scale))) return r;
        if (gqa && !heads_divide(H, q.kv_heads)) return fail(FA2_ERR_INVALID_SHAPE);
        if (dtype == FA2_DTYPE_FP8_E4M3) return fail(FA2_ERR_UNSUPPORTED_DTYPE);      // fp8 is forward only
        if (gqa && dtype != FA2_DTYPE_BF16) return fail(FA2_ERR_UNSUPPORTED_DTYPE);
        if ((r.status = check_dim(d, dtype))) return r;
        r.ws = bwd_ws(q.ws, B, H, q_len, d, dtype, gqa ? H / q.kv_heads : 1);
        if (q.ws_short(r.ws.bytes)) return fail(FA2_ERR_WORKSPACE);
        if (dtype == FA2_DTYPE_F32) { r.path = Path::f32; r.args.phases = phases & 7; break; }
        if ((r.status = check_bwd_planes(B, H, q_len))) return r;
        // bit 3 does not combine with bits 1 and 2 (two ways of computing the same outputs); 7 takes the single kernel where
        // the rule allows it (7 | 16 and 6: the two kernels)
        if ((phases & 8) && ((phases & 6) || !r.ws.single || !device_ok())) return fail(FA2_ERR_UNSUPPORTED);
        if ((phases & 8) || (phases == 7 && r.ws.single && env_and_device_ok())) {
            r.path = Path::single; r.args.phases = phases == 7 ? 9 : (phases & 9);
        } else {
            r.path = Path::two_kernel; r.args.phases = phases & 7; r.clear_error = r.ws.single;
        }
        break;
    case Entry::block: {
        r.status = check_common(B, H, q_len, d, q.scale);
        if (!r.status) r.status = check_common(B, H, kv_len > 0 ? kv_len : 1, d, q.scale);
        if (!r.status) r.status = check_common(B, H, q_hs > 0 ? q_hs : 1, d, q.scale);
        if (r.status) return r;
        if (kv_len <= 0 || q.q_row0 < 0 || q_hs < q.q_row0 + q_len || k_hs < kv_len) return fail(FA2_ERR_INVALID_SHAPE);
        if ((r.status = check_bwd_planes(B, H, q_hs))) return r;
        if (dtype != FA2_DTYPE_BF16) return fail(FA2_ERR_UNSUPPORTED_DTYPE);
        if ((r.status = check_dim(d, dtype))) return r;
        r.ws = bwd_ws(q.ws, B, H, q_hs, d, dtype);      // the square problem's layout for q_hs rows, whatever the block
        if (q.ws_short(r.ws.base_bytes)) return fail(FA2_ERR_WORKSPACE);
        const bool ctl = r.ws.single && q.ws_bytes >= r.ws.bytes;      // room for the running sums and a control block
        const bool square = q_len == kv_len && q_hs == q_len && k_hs == kv_len && q.q_row0 == 0 && (!q.causal || q.shift == 0);
        const bool rect = !q.causal && d == 128 && q_len % 32 == 0 && q_len >= 512 && kv_len % 256 == 0 && kv_len <= fused_npad(q_hs);
        if ((phases & 6) == 6 && (square || rect) && ctl && env_and_device_ok()) {
            r.path = Path::single; r.args.phases = 8 | (phases & 1);
            // bits 8..15: how many CUs to leave (FA2_PHASE_LEAVE_CUS(n)); 0 there = the default of 16
            r.args.reserve_cus = (phases & FA2_PHASE_LEAVE_ROOM) ? (((phases >> 8) & 0xff) ? ((phases >> 8) & 0xff) : 16) : 0;
        } else {
            r.path = Path::two_kernel; r.args.phases = phases & 7; r.clear_error = ctl;
        }
        break;
    }
    case Entry::fused:
        if ((r.status = check_common(B, H, q_len, d, q.scale)) || (r.status = check_bwd_planes(B, H, q_len))) return r;
        r.ws = bwd_ws(q.ws, B, H, q_len, d, FA2_DTYPE_BF16);
        if (!r.ws.single || (phases != 0 && phases != 1)) return fail(FA2_ERR_UNSUPPORTED);
        if (phases == 0 && (q_len % 256 != 0 || d != 128)) return fail(FA2_ERR_UNSUPPORTED);      // the atomics form: d = 128, aligned
        if (phases == 1 && !device_ok()) return fail(FA2_ERR_UNSUPPORTED);
        if (q.ws_short(r.ws.bytes)) return fail(FA2_ERR_WORKSPACE);
        r.path = Path::single; r.mode = phases; r.args.phases = 9;
        break;
    case Entry::status:      // Path::single: read the error word.  Where this process never runs the single kernel (shape,
                             // environment or device) the caller's buffer is not to be trusted: Path::none, drain the stream
        if (!q.ws) return fail(FA2_ERR_NULL_POINTER);
        if (B <= 0 || H <= 0 || q_len <= 0) return fail(FA2_ERR_INVALID_SHAPE);
        r.ws = bwd_ws(q.ws, B, H, q_len, d, dtype);
        if (!r.ws.single || !env_and_device_ok()) break;
        if (q.ws_bytes < r.ws.bytes) return fail(FA2_ERR_WORKSPACE);
        r.path = Path::single;
        break;
    case Entry::plan:
        if (B <= 0 || H <= 0 || q_len <= 0) return fail(FA2_ERR_INVALID_SHAPE);
        if (gqa && !heads_divide(H, q.kv_heads)) return fail(FA2_ERR_INVALID_SHAPE);
        if (dtype == FA2_DTYPE_FP8_E4M3 || (gqa && dtype != FA2_DTYPE_BF16)) return fail(FA2_ERR_UNSUPPORTED_DTYPE);
        if ((r.status = check_dim(d, dtype))) return r;
        r.path = dtype == FA2_DTYPE_F32 ? Path::f32 : Path::two_kernel;
        if (dtype == FA2_DTYPE_F32) r.why = "fp32 path (exact f32 MFMA kernels)";
        else if (!bwd_fused_shape(q_len, d, dtype))
            r.why = "two kernels: the single kernel takes bf16 with head_dim 128 and a seq_len whose padding to a multiple of 256 "
                    "costs less than two block products (5 roundup(N,256) <= 7 roundup(N,64)), or head_dim 64 and a seq_len whose "
                    "padding costs less than 7 % (13 roundup(N,256) <= 14 roundup(N,64))";
        else if (!bwd_fused_allowed()) r.why = "two kernels: FA2_BACKWARD_PATH=two_kernel";
        else if (device_ok()) r.path = Path::single;
        return r;
    default: return fail(FA2_ERR_UNSUPPORTED);      // the forward and packed entries do not come here
    }
    bwd_args(r.args, t, q, r.ws);
    return r;
}

// The sinks and the gradient of L a backward was handed, as the launchers take them beside BwdArgs (phase bit 0 computes with
// them on either bf16 path; nullptr: a call without either).  fa2_backward_sink needs both sinks, fa2_backward_lse both or
// neither; kernel 0 alone reads dL.
struct Sinks { int status; bool any; fa2::SinkGrad sg; const fa2::SinkGrad* ptr() const { return any ? &sg : nullptr; } };
static Sinks sink_grad(const Request& q)
{
    if (q.need_sinks ? !q.sink || !q.dsink : !q.sink != !q.dsink) return {FA2_ERR_NULL_POINTER, false, {}};
    return {FA2_OK, q.sink || q.dL, {q.sink, q.dsink, q.H, q.dL}};
}

// every dense backward entry point: the sinks' rule, the route, the launches
static int backward(Entry entry, const fa2::BwdArgs& t, const Request& q, void* stream)
{
    const hipStream_t s = (hipStream_t)stream;
    const Sinks sinks = sink_grad(q);
    if (sinks.status) return sinks.status;
    const Route r = bwd_route(entry, t, q);
    const fa2::BwdArgs& a = r.args;
    if (r.status) return r.status;
    if (r.clear_error) {
        const hipError_t e = fa2::bwd_fused_clear_error(r.ws.ctl, s);
        if (e != hipSuccess) return hip_status(e);
    }
    if (r.path == Path::single)
        return hip_status(fa2::launch_bwd_fused_bf16(a, r.ws.acc, r.ws.ctl, r.mode, s, r.ws.rcpad, r.ws.kvpart, sinks.ptr()));
    if (r.path == Path::two_kernel) return hip_status(fa2::launch_bwd_bf16(a, s, sinks.ptr()));
    const fa2::F32Args f{(const float*)a.Q, (const float*)a.K, (const float*)a.V, (float*)a.O, (float*)a.L, (const float*)a.dO,
                         (float*)a.dQ, (float*)a.dK, (float*)a.dV, a.D, a.BH, a.Nq, a.d, a.scale, a.causal, a.phases};
    return hip_status(fa2::launch_bwd_f32(f, s));
}

size_t fa2_backward_workspace_bytes(int B, int H, int seq_len, int head_dim, int dtype)
{
    return B <= 0 || H <= 0 || seq_len <= 0 ? 0 : bwd_ws(nullptr, B, H, seq_len, head_dim, dtype).bytes;
}

size_t fa2_backward_fused_workspace_bytes(int B, int H, int seq_len, int head_dim)
{
    if (B <= 0 || H <= 0 || seq_len <= 0) return 0;
    const BwdWs w = bwd_ws(nullptr, B, H, seq_len, head_dim, FA2_DTYPE_BF16);
    return w.single ? w.bytes : 0;
}

int fa2_backward(const void* Q, const void* K, const void* V, const void* O, const float* L,
                 const void* dO, void* dQ, void* dK, void* dV,
                 int B, int H, int seq_len, int head_dim, float softmax_scale,
                 int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream)
{
    return fa2_backward_phases(Q, K, V, O, L, dO, dQ, dK, dV, B, H, seq_len, head_dim, softmax_scale,
                               dtype, causal, workspace, workspace_bytes, stream, 7);
}

int fa2_backward_phases(const void* Q, const void* K, const void* V, const void* O, const float* L,
                        const void* dO, void* dQ, void* dK, void* dV,
                        int B, int H, int seq_len, int head_dim, float softmax_scale,
                        int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream,
                        int phases)
{
    return backward(Entry::phases, {Q, K, V, O, dO, L, dQ, dK, dV}, {.B = B, .H = H, .q_len = seq_len, .kv_len = seq_len, .head_dim = head_dim, .dtype = dtype,
                    .scale = softmax_scale, .causal = causal, .phases = phases, .ws = workspace, .ws_bytes = workspace_bytes}, stream);
}

int fa2_backward_block(const void* Q, const void* K, const void* V, const void* O, const float* L,
                       const void* dO, void* dQ, void* dK, void* dV,
                       int B, int H, int q_len, int kv_len, int head_dim, float softmax_scale, int dtype,
                       int q_head_stride, int kv_head_stride, int q_row0, int causal, int causal_shift,
                       void* workspace, size_t workspace_bytes, void* stream, int phases)
{
    return backward(Entry::block, {Q, K, V, O, dO, L, dQ, dK, dV}, {.B = B, .H = H, .q_len = q_len, .kv_len = kv_len, .q_stride = q_head_stride,
                    .kv_stride = kv_head_stride, .q_row0 = q_row0, .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale,
                    .causal = causal, .shift = causal_shift, .phases = phases, .ws = workspace, .ws_bytes = workspace_bytes}, stream);
}

int fa2_backward_fused(const void* Q, const void* K, const void* V, const void* O, const float* L,
                       const void* dO, void* dQ, void* dK, void* dV,
                       int B, int H, int seq_len, int head_dim, float softmax_scale, int mode,
                       void* workspace, size_t workspace_bytes, void* stream)
{
    return backward(Entry::fused, {Q, K, V, O, dO, L, dQ, dK, dV}, {.B = B, .H = H, .q_len = seq_len, .kv_len = seq_len, .head_dim = head_dim,
                    .scale = softmax_scale, .phases = mode, .ws = workspace, .ws_bytes = workspace_bytes}, stream);
}

// both *_plan functions: 1 = the single kernel, 2 = the two kernels or fp32, and why
static int backward_plan(const Request& q, const char** reason)
{
    const Route r = bwd_route(Entry::plan, {}, q);
    if (reason) *reason = r.status ? "" : r.why;
    return r.status ? r.status : r.path == Path::single ? 1 : 2;
}

int fa2_backward_plan(int B, int H, int seq_len, int head_dim, int dtype, int causal, const char** reason)
{
    return backward_plan({.B = B, .H = H, .q_len = seq_len, .kv_len = seq_len, .head_dim = head_dim, .dtype = dtype, .causal = causal},
                         reason);
}

size_t fa2_backward_gqa_workspace_bytes(int B, int H_q, int H_kv, int seq_len, int head_dim, int dtype)
{
    if (B <= 0 || H_q <= 0 || H_kv <= 0 || H_q % H_kv != 0 || seq_len <= 0) return 0;
    return bwd_ws(nullptr, B, H_q, seq_len, head_dim, dtype, H_q / H_kv).bytes;
}

int fa2_backward_gqa(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                     void* dQ, void* dK, void* dV,
                     int B, int H_q, int H_kv, int seq_len, int head_dim, float softmax_scale,
                     int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases)
{
    return backward(Entry::phases, {Q, K, V, O, dO, L, dQ, dK, dV}, {.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = seq_len, .kv_len = seq_len,
                    .head_dim = head_dim, .dtype = dtype, .scale = softmax_scale, .causal = causal, .phases = phases, .ws = workspace,
                    .ws_bytes = workspace_bytes}, stream);
}

int fa2_backward_gqa_plan(int B, int H_q, int H_kv, int seq_len, int head_dim, int dtype, int causal, const char** reason)
{
    return backward_plan({.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = seq_len, .kv_len = seq_len, .head_dim = head_dim,
                          .dtype = dtype, .causal = causal}, reason);
}

size_t fa2_backward_qk_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, int dtype)
{
    if (kv_len <= 0) return 0;
    if (q_len == kv_len) return fa2_backward_gqa_workspace_bytes(B, H_q, H_kv, q_len, head_dim, dtype);
    if (B <= 0 || H_q <= 0 || H_kv <= 0 || H_q % H_kv != 0 || q_len <= 0) return 0;
    return bwd_ws(nullptr, B, H_q, q_len, head_dim, dtype).base_bytes;
}

int fa2_backward_qk(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                    void* dQ, void* dK, void* dV,
                    int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                    int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases)
{
    return fa2_backward_lse(Q, K, V, nullptr, O, L, dO, nullptr, dQ, dK, dV, nullptr, B, H_q, H_kv, q_len, kv_len, head_dim, softmax_scale,
                            dtype, causal, workspace, workspace_bytes, stream, phases);
}

size_t fa2_backward_sink_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, int dtype)
{
    return fa2_backward_qk_workspace_bytes(B, H_q, H_kv, q_len, kv_len, head_dim, dtype);
}

int fa2_backward_sink(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L, const void* dO,
                      void* dQ, void* dK, void* dV, float* dsink,
                      int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                      int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases)
{
    return backward(Entry::qk, {Q, K, V, O, dO, L, dQ, dK, dV}, {.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = q_len, .kv_len = kv_len, .head_dim = head_dim,
                    .dtype = dtype, .scale = softmax_scale, .causal = causal, .shift = kv_len - q_len, .phases = phases,
                    .ws = workspace, .ws_bytes = workspace_bytes, .sink = sink, .dsink = dsink, .need_sinks = true}, stream);
}

// fa2_backward_qk / fa2_backward_sink with a gradient for L (kernel 0 alone reads it, with phase bit 0)
int fa2_backward_lse(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L, const void* dO,
                     const float* dL, void* dQ, void* dK, void* dV, float* dsink,
                     int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                     int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases)
{
    return backward(Entry::qk, {Q, K, V, O, dO, L, dQ, dK, dV}, {.B = B, .H = H_q, .kv_heads = grouped(H_kv), .q_len = q_len, .kv_len = kv_len, .head_dim = head_dim,
                    .dtype = dtype, .scale = softmax_scale, .causal = causal, .shift = kv_len - q_len, .phases = phases,
                    .ws = workspace, .ws_bytes = workspace_bytes, .sink = sink, .dsink = dsink, .dL = dL},
                    stream);
}

// D [H_q][T] and the two row-constant planes, laid out as the front of every other backward workspace
size_t fa2_backward_varlen_workspace_bytes(int H_q, int H_kv, int total_rows, int head_dim, int dtype)
{
    if (H_q <= 0 || H_kv <= 0 || H_q % H_kv != 0 || total_rows <= 0) return 0;
    return bwd_ws(nullptr, 1, H_q, total_rows, head_dim, dtype).base_bytes;
}

// Every packed backward entry point.  One implementation (the two deterministic kernels over the plan's items), so there is
// nothing to route: the checks are check_request's, the arguments bwd_args', as for the dense calls.
static int backward_varlen(const fa2::BwdArgs& t, const Request& q, void* stream)
{
    const Sinks sinks = sink_grad(q);
    if (sinks.status) return sinks.status;
    if (any_null(t) || !q.plan_host || !q.plan_dev) return FA2_ERR_NULL_POINTER;
    VarlenHeader h;
    if (const int st = check_request(Entry::backward_packed, q, &h)) return st;
    const BwdWs ws = bwd_ws(q.ws, 1, q.H, q.q_len, q.head_dim, q.dtype);
    if (q.ws_short(ws.base_bytes)) return FA2_ERR_WORKSPACE;
    fa2::VarlenBwdArgs v{};
    bwd_args(v.a, t, q, ws);
    v.a.phases = 7;
    const auto* items = reinterpret_cast<const fa2::VarlenItem*>((const char*)q.plan_dev + sizeof(VarlenHeader));
    v.row_items = items; v.n_row_items = h.n_row_items;
    v.key_items = items + h.n_row_items; v.n_key_items = h.n_key_items;
    return hip_status(fa2::launch_bwd_varlen_bf16(v, (hipStream_t)stream, sinks.ptr()));
}

int fa2_backward_varlen(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                        void* dQ, void* dK, void* dV,
                        int H_q, int H_kv, int total_rows, int head_dim, float softmax_scale, int dtype, int causal,
                        const void* plan_host, const void* plan_dev, size_t plan_bytes,
                        void* workspace, size_t workspace_bytes, void* stream)
{
    return backward_varlen({Q, K, V, O, dO, L, dQ, dK, dV}, {.H = H_q, .kv_heads = grouped(H_kv), .q_len = total_rows, .kv_len = total_rows, .head_dim = head_dim,
                           .dtype = dtype, .scale = softmax_scale, .causal = causal, .ws = workspace, .ws_bytes = workspace_bytes,
                           .plan_host = plan_host, .plan_dev = plan_dev, .plan_bytes = plan_bytes, .one_list = true}, stream);
}

// the planes are indexed by query rows: the key side does not enter the size
size_t fa2_backward_varlen_qk_workspace_bytes(int H_q, int H_kv, int total_q, int total_k, int head_dim, int dtype)
{
    return total_k <= 0 ? 0 : fa2_backward_varlen_workspace_bytes(H_q, H_kv, total_q, head_dim, dtype);
}

int fa2_backward_varlen_qk(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                           void* dQ, void* dK, void* dV,
                           int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                           const void* plan_host, const void* plan_dev, size_t plan_bytes,
                           void* workspace, size_t workspace_bytes, void* stream)
{
    return fa2_backward_varlen_lse(Q, K, V, nullptr, O, L, dO, nullptr, dQ, dK, dV, nullptr, H_q, H_kv, total_q, total_k, head_dim, softmax_scale,
                                   dtype, causal, plan_host, plan_dev, plan_bytes, workspace, workspace_bytes, stream);
}

size_t fa2_backward_varlen_sink_workspace_bytes(int H_q, int H_kv, int total_q, int total_k, int head_dim, int dtype)
{
    return fa2_backward_varlen_qk_workspace_bytes(H_q, H_kv, total_q, total_k, head_dim, dtype);
}

int fa2_backward_varlen_sink(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L,
                             const void* dO, void* dQ, void* dK, void* dV, float* dsink,
                             int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                             const void* plan_host, const void* plan_dev, size_t plan_bytes,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    return backward_varlen({Q, K, V, O, dO, L, dQ, dK, dV}, {.H = H_q, .kv_heads = grouped(H_kv), .q_len = total_q, .kv_len = total_k, .head_dim = head_dim,
                           .dtype = dtype, .scale = softmax_scale, .causal = causal, .ws = workspace, .ws_bytes = workspace_bytes,
                           .sink = sink, .dsink = dsink, .need_sinks = true,
                           .plan_host = plan_host, .plan_dev = plan_dev, .plan_bytes = plan_bytes}, stream);
}

int fa2_backward_varlen_lse(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L,
                            const void* dO, const float* dL, void* dQ, void* dK, void* dV, float* dsink,
                            int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                            const void* plan_host, const void* plan_dev, size_t plan_bytes,
                            void* workspace, size_t workspace_bytes, void* stream)
{
    return backward_varlen({Q, K, V, O, dO, L, dQ, dK, dV}, {.H = H_q, .kv_heads = grouped(H_kv), .q_len = total_q, .kv_len = total_k, .head_dim = head_dim,
                           .dtype = dtype, .scale = softmax_scale, .causal = causal, .ws = workspace, .ws_bytes = workspace_bytes,
                           .sink = sink, .dsink = dsink, .dL = dL,
                           .plan_host = plan_host, .plan_dev = plan_dev, .plan_bytes = plan_bytes}, stream);
}

// ---- merging partial results (include/fa2_mi355x.h): argument checks, then the part pointers by value into the kernels
static int merge_check(const void* const* O_parts, const float* const* L_parts, int n_parts, size_t rows, int head_dim, int dtype)
{
    if (!O_parts || !L_parts) return FA2_ERR_NULL_POINTER;
    if (n_parts < 1 || n_parts > fa2::kMergeMaxParts || rows == 0) return FA2_ERR_INVALID_SHAPE;
    for (int i = 0; i < n_parts; ++i)
        if (!O_parts[i] || !L_parts[i]) return FA2_ERR_NULL_POINTER;
    if (rows > (size_t)0x7fffffff * 8) return FA2_ERR_INVALID_SHAPE;      // the grid: one workgroup per 16 or 32 rows
    return check_bf16(head_dim, dtype);
}

int fa2_merge_states(const void* const* O_parts, const float* const* L_parts, int n_parts, void* O, float* L, size_t rows,
                     int head_dim, int dtype, void* stream)
{
    if (!O || !L) return FA2_ERR_NULL_POINTER;
    const int st = merge_check(O_parts, L_parts, n_parts, rows, head_dim, dtype);
    if (st) return st;
    fa2::MergeArgs a{};
    for (int i = 0; i < n_parts; ++i) { a.O[i] = O_parts[i]; a.L[i] = L_parts[i]; }
    a.n = n_parts; a.Oout = O; a.Lout = L; a.rows = rows;
    return hip_status(fa2::launch_merge_fwd(a, head_dim, (hipStream_t)stream));
}

int fa2_merge_states_backward(const void* const* O_parts, const float* const* L_parts, const void* O, const float* L, const void* dO,
                              const float* dL, void* const* dO_parts, float* const* dL_parts, int n_parts, size_t rows, int head_dim,
                              int dtype, void* stream)
{
    if (!O || !L || !dO || !dO_parts || !dL_parts) return FA2_ERR_NULL_POINTER;
    const int st = merge_check(O_parts, L_parts, n_parts, rows, head_dim, dtype);
    if (st) return st;
    fa2::MergeBwdArgs b{};
    for (int i = 0; i < n_parts; ++i) {
        if (!dO_parts[i] || !dL_parts[i]) return FA2_ERR_NULL_POINTER;
        b.m.O[i] = O_parts[i]; b.m.L[i] = L_parts[i]; b.dO_parts[i] = dO_parts[i]; b.dL_parts[i] = dL_parts[i];
    }
    b.m.n = n_parts; b.m.Oout = const_cast<void*>(O); b.m.Lout = const_cast<float*>(L); b.m.rows = rows;
    b.dO = dO; b.dL = dL;
    return hip_status(fa2::launch_merge_bwd(b, head_dim, (hipStream_t)stream));
}

// ---- split-KV decode over a KV cache (include/fa2_mi355x.h; fa2_decode.hip).  Nothing here reads a sequence length.
int fa2_decode_num_splits(int B, int H_kv, int kv_capacity, int head_dim)
{
    (void)head_dim;      // part of the signature: the rule may come to depend on the row size
    if (B <= 0 || H_kv <= 0 || kv_capacity <= 0) return 1;
    return fa2::decode_num_splits(B, H_kv, kv_capacity);
}

// The window a call runs with: -1 (none: the plain kernels, the plain split rule) unless it can exclude a key of a full cache.
static int decode_window(int window_left, int kv_capacity)
{
    return window_left < 0 || window_left >= kv_capacity - 1 ? -1 : window_left;
}

// With a window a sequence's splits share at most window_left + q_len + 127 keys (from rounddown(lo_b, 128) to len_b): the
// rule above on that capacity.
int fa2_decode_window_num_splits(int B, int H_kv, int q_len, int kv_capacity, int head_dim, int window_left)
{
    if (B <= 0 || H_kv <= 0 || kv_capacity <= 0) return 1;
    const int w = decode_window(window_left, kv_capacity);
    if (w < 0 || q_len <= 0) return fa2_decode_num_splits(B, H_kv, kv_capacity, head_dim);
    const long long span = (long long)w + q_len + (fa2::kDecodeKB - 1);
    return fa2_decode_num_splits(B, H_kv, (int)std::min<long long>(kv_capacity, span), head_dim);
}

size_t fa2_decode_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, int n_splits)
{
    if (B <= 0 || H_q <= 0 || H_kv <= 0 || q_len <= 0 || kv_capacity <= 0 || head_dim <= 0) return 0;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return 0;
    if (n_splits == 0) n_splits = fa2_decode_num_splits(B, H_kv, kv_capacity, head_dim);
    if (n_splits == 1) return 0;
    return align256((size_t)n_splits * B * H_q * q_len * ((size_t)head_dim + 1) * sizeof(float));
}

// The caches of a decode call: bf16 like Q (kv_dtype = FA2_DTYPE_BF16, no descales), or -- the _fp8kv entry points -- OCP e4m3
// with fp32 DEVICE descales per K/V head (nullptr = 1), which nothing here reads either.  The _window entry points take either
// (any_kv; a descale beside a bf16 cache is refused where the dtype is) and a window_left; every other one has none (-1).
struct DecodeKv {
    int kv_dtype = FA2_DTYPE_BF16; const float* k_descale = nullptr; const float* v_descale = nullptr;
    bool any_kv = false; int window_left = -1;
};
// Q's dtype, then the caches': both at the position of the dtype check, head_dim first
static int decode_check_dtypes(int head_dim, int dtype, const DecodeKv& kv, bool fp8kv_entry)
{
    if (const int st = check_bf16(head_dim, dtype)) return st;
    if (kv.any_kv) {
        if (kv.kv_dtype == FA2_DTYPE_FP8_E4M3) return FA2_OK;
        return kv.kv_dtype == FA2_DTYPE_BF16 && !kv.k_descale && !kv.v_descale ? FA2_OK : FA2_ERR_UNSUPPORTED_DTYPE;
    }
    return kv.kv_dtype == (fp8kv_entry ? FA2_DTYPE_FP8_E4M3 : FA2_DTYPE_BF16) ? FA2_OK : FA2_ERR_UNSUPPORTED_DTYPE;
}
static void decode_kv_args(fa2::DecodeArgs& a, const DecodeKv& kv, int kv_capacity)
{
    a.kv_fp8 = kv.kv_dtype == FA2_DTYPE_FP8_E4M3; a.k_descale = kv.k_descale; a.v_descale = kv.v_descale;
    a.window_left = decode_window(kv.window_left, kv_capacity);
}

static int decode_contiguous(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                             void* O, float* L, int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                             int dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream,
                             const DecodeKv& kv, bool fp8kv_entry)
{
    if (!Q || !K_cache || !V_cache || !O || !L) return FA2_ERR_NULL_POINTER;
    int st = check_common(B, H_q, q_len, head_dim, softmax_scale);
    if (st) return st;
    if (!heads_divide(H_q, H_kv) || kv_capacity <= 0) return FA2_ERR_INVALID_SHAPE;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
    // one (b, head) slab, one buffer resource: 2 bytes per element, 1 in an e4m3 cache
    if ((long long)kv_capacity * head_dim * (fp8kv_entry ? 1 : 2) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    if (kv.window_left < -1) return FA2_ERR_INVALID_SHAPE;
    if ((st = decode_check_dtypes(head_dim, dtype, kv, fp8kv_entry))) return st;
    if (n_splits == 0) n_splits = fa2_decode_window_num_splits(B, H_kv, q_len, kv_capacity, head_dim, kv.window_left);
    if ((long long)B * H_kv * n_splits > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;             // the grid
    const size_t need = fa2_decode_workspace_bytes(B, H_q, H_kv, q_len, kv_capacity, head_dim, n_splits);
    if (n_splits > 1 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) return FA2_ERR_WORKSPACE;
    if ((long long)(H_q / H_kv) * q_len > fa2::kDecodeMaxRows) return FA2_ERR_UNSUPPORTED;
    if (kv.window_left >= 0 && !causal) return FA2_ERR_UNSUPPORTED;      // (whatever the capacity: the window is a causal one)
    fa2::DecodeArgs a{};
    a.Q = Q; a.K = K_cache; a.V = V_cache; a.seqlens = seqlens_k; a.sink = sink; a.O = O; a.L = L;
    a.wsO = (float*)workspace;
    a.wsL = n_splits > 1 ? (float*)workspace + (size_t)n_splits * B * H_q * q_len * head_dim : nullptr;
    a.B = B; a.Hq = H_q; a.Hkv = H_kv; a.Nq = q_len; a.Ncap = kv_capacity; a.n_splits = n_splits;
    a.scale = softmax_scale; a.causal = causal ? 1 : 0;
    decode_kv_args(a, kv, kv_capacity);
    return hip_status(fa2::launch_decode(a, head_dim, (hipStream_t)stream));
}

int fa2_forward_decode(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                       void* O, float* L, int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                       int dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream)
{
    return decode_contiguous(Q, K_cache, V_cache, seqlens_k, sink, O, L, B, H_q, H_kv, q_len, kv_capacity, head_dim, softmax_scale, dtype,
                             causal, n_splits, workspace, workspace_bytes, stream, {}, false);
}

// fa2_forward_decode over e4m3 caches: the same checks in the same order (the slab limit at one byte per element)
int fa2_forward_decode_fp8kv(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                             const float* k_descale, const float* v_descale, void* O, float* L,
                             int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                             int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream)
{
    return decode_contiguous(Q, K_cache, V_cache, seqlens_k, sink, O, L, B, H_q, H_kv, q_len, kv_capacity, head_dim, softmax_scale, dtype,
                             causal, n_splits, workspace, workspace_bytes, stream, {kv_dtype, k_descale, v_descale}, true);
}

// The same call over a pool of pages.  Nothing here reads the block table either: the capacity max_pages_per_seq x page_size
// stands where kv_capacity stood, and the kernel turns table entries into addresses (clamped to the pool).
static int decode_paged(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                        const int* seqlens_k, const float* sink, void* O, float* L,
                        int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                        int head_dim, float softmax_scale, int dtype, int causal, int n_splits,
                        void* workspace, size_t workspace_bytes, void* stream, const DecodeKv& kv, bool fp8kv_entry)
{
    if (!Q || !K_pages || !V_pages || !block_table || !O || !L) return FA2_ERR_NULL_POINTER;
    int st = check_common(B, H_q, q_len, head_dim, softmax_scale);
    if (st) return st;
    if (!heads_divide(H_q, H_kv) || n_pages <= 0 || page_size <= 0 || max_pages_per_seq <= 0) return FA2_ERR_INVALID_SHAPE;
    if (page_size % fa2::kDecodeTile) return FA2_ERR_INVALID_SHAPE;                              // a tile never crosses a page
    // key indices are ints, and the kernel forms begin = split chunk <= len + n_splits kDecodeKB and kb + 2 kDecodeKB (kb + 4
    // kDecodeKB over e4m3 pools, two tiles in flight)
    if ((long long)max_pages_per_seq * page_size > 0x7fffffffLL - (fa2::kDecodeMaxSplits + 2) * fa2::kDecodeKB) return FA2_ERR_INVALID_SHAPE;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
    if (kv.window_left < -1) return FA2_ERR_INVALID_SHAPE;
    const int kv_capacity = max_pages_per_seq * page_size;
    const int resolved = n_splits ? n_splits : fa2_decode_window_num_splits(B, H_kv, q_len, kv_capacity, head_dim, kv.window_left);
    if ((long long)B * H_kv * resolved > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;             // the grid
    if ((st = decode_check_dtypes(head_dim, dtype, kv, fp8kv_entry))) return st;
    n_splits = resolved;
    const size_t need = fa2_decode_workspace_bytes(B, H_q, H_kv, q_len, kv_capacity, head_dim, n_splits);
    if (n_splits > 1 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))) return FA2_ERR_WORKSPACE;
    if ((long long)(H_q / H_kv) * q_len > fa2::kDecodeMaxRows) return FA2_ERR_UNSUPPORTED;
    if (kv.window_left >= 0 && !causal) return FA2_ERR_UNSUPPORTED;
    fa2::DecodeArgs a{};
    a.Q = Q; a.K = K_pages; a.V = V_pages; a.seqlens = seqlens_k; a.sink = sink; a.O = O; a.L = L;
    a.wsO = (float*)workspace;
    a.wsL = n_splits > 1 ? (float*)workspace + (size_t)n_splits * B * H_q * q_len * head_dim : nullptr;
    a.B = B; a.Hq = H_q; a.Hkv = H_kv; a.Nq = q_len; a.Ncap = kv_capacity; a.n_splits = n_splits;
    a.scale = softmax_scale; a.causal = causal ? 1 : 0;
    a.block_table = block_table; a.n_pages = n_pages; a.page_size = page_size; a.max_pages = max_pages_per_seq;
    decode_kv_args(a, kv, kv_capacity);
    return hip_status(fa2::launch_decode(a, head_dim, (hipStream_t)stream));
}

int fa2_forward_decode_paged(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                             const int* seqlens_k, const float* sink, void* O, float* L,
                             int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                             int head_dim, float softmax_scale, int dtype, int causal, int n_splits,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    return decode_paged(Q, K_pages, V_pages, block_table, seqlens_k, sink, O, L, B, H_q, H_kv, q_len, n_pages, page_size,
                        max_pages_per_seq, head_dim, softmax_scale, dtype, causal, n_splits, workspace, workspace_bytes, stream, {}, false);
}

int fa2_forward_decode_paged_fp8kv(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                                   const int* seqlens_k, const float* sink, const float* k_descale, const float* v_descale,
                                   void* O, float* L,
                                   int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                                   int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                                   void* workspace, size_t workspace_bytes, void* stream)
{
    return decode_paged(Q, K_pages, V_pages, block_table, seqlens_k, sink, O, L, B, H_q, H_kv, q_len, n_pages, page_size,
                        max_pages_per_seq, head_dim, softmax_scale, dtype, causal, n_splits, workspace, workspace_bytes, stream,
                        {kv_dtype, k_descale, v_descale}, true);
}

// fa2_forward_decode / _fp8kv and their paged forms with a sliding window: the siblings' checks in their order
int fa2_forward_decode_window(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                              const float* k_descale, const float* v_descale, void* O, float* L,
                              int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                              int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream,
                              int window_left)
{
    return decode_contiguous(Q, K_cache, V_cache, seqlens_k, sink, O, L, B, H_q, H_kv, q_len, kv_capacity, head_dim, softmax_scale, dtype,
                             causal, n_splits, workspace, workspace_bytes, stream, {kv_dtype, k_descale, v_descale, true, window_left},
                             kv_dtype == FA2_DTYPE_FP8_E4M3);
}

int fa2_forward_decode_paged_window(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                                    const int* seqlens_k, const float* sink, const float* k_descale, const float* v_descale,
                                    void* O, float* L,
                                    int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                                    int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                                    void* workspace, size_t workspace_bytes, void* stream, int window_left)
{
    return decode_paged(Q, K_pages, V_pages, block_table, seqlens_k, sink, O, L, B, H_q, H_kv, q_len, n_pages, page_size,
                        max_pages_per_seq, head_dim, softmax_scale, dtype, causal, n_splits, workspace, workspace_bytes, stream,
                        {kv_dtype, k_descale, v_descale, true, window_left}, kv_dtype == FA2_DTYPE_FP8_E4M3);
}

int fa2_backward_status(const void* workspace, size_t workspace_bytes, int B, int H, int seq_len, int head_dim, int dtype,
                        void* stream)
{
    const Route r = bwd_route(Entry::status, {}, {.B = B, .H = H, .q_len = seq_len, .kv_len = seq_len, .head_dim = head_dim,
                                                  .dtype = dtype, .ws = workspace, .ws_bytes = workspace_bytes});
    if (r.status) return r.status;
    if (r.path != Path::single) return hip_status(hipStreamSynchronize((hipStream_t)stream));
    int err = 0;
    const hipError_t e = fa2::bwd_fused_read_error(r.ws.ctl, &err, (hipStream_t)stream);
    if (e != hipSuccess) return hip_status(e);
    return err ? FA2_ERR_HANDOFF_TIMEOUT : FA2_OK;
}

int fa2_forward_step(const void* Q, const void* K, const void* V,
                     void* O, float* L, float* Oacc, float* M,
                     int B, int H, int q_len, int kv_len, int head_dim, float softmax_scale,
                     int dtype, int first, int last, void* stream)
{
    if (!Q || !K || !V || !L) return FA2_ERR_NULL_POINTER;
    int st = check_common(B, H, q_len, head_dim, softmax_scale);
    if (st) return st;
    if (kv_len <= 0) return FA2_ERR_INVALID_SHAPE;
    if (dtype == FA2_DTYPE_FP8_E4M3) return FA2_ERR_UNSUPPORTED_DTYPE;      // no resumable fp8 step
    st = check_dim(head_dim, dtype);
    if (st) return st;
    if (dtype == FA2_DTYPE_F32) {
        // fp32: O itself carries the un-normalised accumulator between steps (the reference's
        // layout); Oacc is ignored.
        if (!O) return FA2_ERR_NULL_POINTER;
        if ((!first || !last) && !M) return FA2_ERR_NULL_POINTER;
        fa2::F32Args a{};
        a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V; a.O = (float*)O; a.L = L;
        a.BH = B * H; a.N = q_len; a.Nk = kv_len; a.d = head_dim; a.scale = softmax_scale; a.causal = 0;
        a.M = M; a.resume = first ? 0 : 1; a.finalize = last ? 1 : 0;
        return hip_status(fa2::launch_fwd_f32(a, (hipStream_t)stream));
    }
    return fa2_forward_step_strided(Q, K, V, O, L, Oacc, M, B, H, q_len, kv_len, head_dim, softmax_scale, dtype, first,
                                    last, 0, 0, 0, 0, stream);
}

int fa2_forward_step_strided(const void* Q, const void* K, const void* V,
                             void* O, float* L, float* Oacc, float* M,
                             int B, int H, int q_len, int kv_len, int head_dim, float softmax_scale,
                             int dtype, int first, int last, int q_head_stride, int kv_head_stride,
                             int causal, int causal_shift, void* stream)
{
    if (!Q || !K || !V || !L) return FA2_ERR_NULL_POINTER;
    int st = check_common(B, H, q_len, head_dim, softmax_scale);
    if (st) return st;
    if (kv_len <= 0) return FA2_ERR_INVALID_SHAPE;
    if (dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    st = check_dim(head_dim, dtype);
    if (st) return st;
    if ((q_head_stride && q_head_stride < q_len) || (kv_head_stride && kv_head_stride < kv_len)) return FA2_ERR_INVALID_SHAPE;
    if (last && !O) return FA2_ERR_NULL_POINTER;
    if ((!first || !last) && (!Oacc || !M)) return FA2_ERR_NULL_POINTER;
    fa2::FwdArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.L = L; a.Oacc = Oacc; a.M = M;
    a.BH = B * H; a.Nq = q_len; a.Nk = kv_len; a.d = head_dim; a.scale = softmax_scale;
    a.causal = causal ? 1 : 0; a.causal_shift = causal ? causal_shift : 0;
    a.resume = first ? 0 : 1; a.finalize = last ? 1 : 0;
    a.q_hs = q_head_stride; a.k_hs = kv_head_stride; a.kv_group = 1;
    return hip_status(fa2::launch_fwd1_bf16(a, (hipStream_t)stream));
}

int fa2_forward_state_finalize(void* O, float* L, const float* Oacc, const float* M,
                               size_t rows, int head_dim, int dtype, void* stream)
{
    if (!O || !L || !Oacc || !M) return FA2_ERR_NULL_POINTER;
    if (dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    int st = check_dim(head_dim, dtype);
    if (st) return st;
    return hip_status(fa2::launch_finalize_state(Oacc, M, L, O, rows, head_dim, (hipStream_t)stream));
}

int flash_attention_2_forward(const float* Q, const float* K, const float* V,
                              float* O, float* L, int seq_len, int head_dim, float softmax_scale)
{
    return fa2_forward(Q, K, V, O, L, 1, 1, seq_len, head_dim, softmax_scale, FA2_DTYPE_F32, 0, nullptr);
}

int flash_attention(const float* Q, const float* K, const float* V, float* O, float* l, float* m, int N, int d, int Bc, int M)
{
    (void)M;                 // the reference sizes nothing from M either (main.cu:22: "we set Bc directly")
    if (!Q || !K || !V || !O || !l || !m) return FA2_ERR_NULL_POINTER;
    if (N <= 0 || d <= 0 || Bc <= 0) return FA2_ERR_INVALID_SHAPE;
    if (d > 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    return hip_status(fa2::launch_fa1_f32(Q, K, V, O, l, m, N, d, Bc, nullptr));
}

int flash_attention_2_backward(const float* Q, const float* K, const float* V,
                               const float* O, const float* L, const float* dO,
                               float* dQ, float* dK, float* dV,
                               int seq_len, int head_dim, float softmax_scale)
{
    const size_t need = fa2_backward_workspace_bytes(1, 1, seq_len, head_dim, FA2_DTYPE_F32);
    if (need == 0) return FA2_ERR_INVALID_SHAPE;
    void* ws = nullptr;
    int st = g_scratch.get(need, &ws);
    if (st) return st;
    return fa2_backward(Q, K, V, O, L, dO, dQ, dK, dV, 1, 1, seq_len, head_dim, softmax_scale,
                        FA2_DTYPE_F32, 0, ws, need, nullptr);
}

int fa2_accumulate_bf16(float* acc, const void* src, size_t n, int init, void* stream)
{
    return fa2_accumulate_bf16_2d(acc, src, 1, n, n, init, stream);
}

int fa2_accumulate_bf16_2d(float* acc, const void* src, size_t rows, size_t cols, size_t pitch, int init, void* stream)
{
    if (!acc || !src) return FA2_ERR_NULL_POINTER;
    if (pitch < cols && rows > 1) return FA2_ERR_INVALID_SHAPE;
    return hip_status(fa2::launch_accumulate_bf16(acc, src, rows, cols, pitch, init, (hipStream_t)stream));
}

int fa2_read_clocks(unsigned long long* out32, void* stream)
{
    if (!out32) return FA2_ERR_NULL_POINTER;
    if ((uintptr_t)out32 & 15) return FA2_ERR_INVALID_SHAPE;
    return hip_status(fa2::launch_read_clocks(out32, (hipStream_t)stream));
}

int fa2_mfma_probe(const void* operands, float* out, int iters, int workgroups, void* stream)
{
    if (!operands || !out) return FA2_ERR_NULL_POINTER;
    if (iters < 1 || workgroups < 1) return FA2_ERR_INVALID_SHAPE;
    return hip_status(fa2::launch_mfma_probe(operands, out, iters, workgroups, (hipStream_t)stream));
}

int fa2_fill_f32(float* dst, size_t n, float value, void* stream)
{
    if (!dst && n) return FA2_ERR_NULL_POINTER;
    return hip_status(fa2::launch_fill_f32(dst, n, value, (hipStream_t)stream));
}

int fa2_convert_f32_to_bf16(const float* src, void* dst, size_t n, void* stream)
{
    if ((!src || !dst) && n) return FA2_ERR_NULL_POINTER;
    return hip_status(fa2::launch_f32_to_bf16(src, dst, n, (hipStream_t)stream));
}

int fa2_convert_bf16_to_f32(const void* src, float* dst, size_t n, void* stream)
{
    if ((!src || !dst) && n) return FA2_ERR_NULL_POINTER;
    return hip_status(fa2::launch_bf16_to_f32(src, dst, n, (hipStream_t)stream));
}

}  // extern "C"
