// fa2_extend_ragged.hip -- the C entry points of ragged extend attention (include/fa2_extend_ragged_mi355x.h): the extend calls
// with a q_len per sequence and token-major rows.  Host code only: the checks in the siblings' order (fa2_extend.hip), then
// launch_extend_ragged_plan / launch_extend_ragged (fa2_decode.hip: the plan kernel, extend_ragged_split_body).  Nothing here
// reads cu_seqlens_q, a length, a table or a descale.
#include "fa2_extend_ragged_mi355x.h"
#include "fa2_launch.h"

#include <algorithm>
#include <stdint.h>

namespace fa2 {
namespace {

inline int ragged_hip_status(hipError_t e) { return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e; }

// what the plan and the grid are sized by; false for arguments every call refuses
inline bool ragged_dims(int B, int H_q, int H_kv, int total_q)
{
    return B > 0 && H_q > 0 && H_kv > 0 && total_q > 0 && H_q % H_kv == 0 && (long long)total_q * H_q <= 0x7fffffffLL - kExtendRows;
}

// the window a call runs with: -1 unless it can exclude a key of a full cache (the siblings' rule)
inline int ragged_window(int window_left, int kv_capacity)
{
    return window_left < 0 || window_left >= kv_capacity - 1 ? -1 : window_left;
}

// n_splits total_q H_q (head_dim + 1) floats rounded up to 256 bytes; 0: it does not fit
inline size_t ragged_partials_bytes(int H_q, int total_q, int head_dim, int n_splits)
{
    const unsigned __int128 bytes = (unsigned __int128)n_splits * total_q * H_q * ((unsigned)head_dim + 1) * sizeof(float);
    if (bytes > SIZE_MAX / 2) return 0;
    return ((size_t)bytes + 255) & ~(size_t)255;
}

struct RaggedCall {
    const void* Q; long long q_stride; const void* K; const void* V; const int* block_table; const void* plan; size_t plan_bytes;
    const int* seqlens_k; const float* sink; const float* k_descale; const float* v_descale; void* O; float* L;
    int B, H_q, H_kv, total_q, kv_capacity, n_pages, page_size, max_pages, head_dim;
    float scale;
    int dtype, kv_dtype, causal, n_splits;
    void* ws; size_t ws_bytes; void* stream;
    int window_left;
};

// the siblings' checks in the siblings' order (extend_run, fa2_extend.hip) with the plan's and the stride's among them
int ragged_run(const RaggedCall& c, bool paged)
{
    if (!c.Q || !c.K || !c.V || !c.O || !c.L || (paged && !c.block_table) || !c.plan) return FA2_ERR_NULL_POINTER;
    if (c.B <= 0 || c.H_q <= 0 || c.total_q <= 0 || c.head_dim <= 0 || !(c.scale > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    if ((long long)c.B * c.H_q > 0x7fffffffLL / 64) return FA2_ERR_INVALID_SHAPE;
    if (c.H_kv <= 0 || c.H_q % c.H_kv) return FA2_ERR_INVALID_SHAPE;
    if (c.q_stride < (long long)c.H_q * c.head_dim || c.q_stride % 8) return FA2_ERR_INVALID_SHAPE;
    const bool fp8 = c.kv_dtype == FA2_DTYPE_FP8_E4M3;
    int kv_capacity = c.kv_capacity;
    if (paged) {
        if (c.n_pages <= 0 || c.page_size <= 0 || c.max_pages <= 0 || c.page_size % kDecodeTile) return FA2_ERR_INVALID_SHAPE;
        if ((long long)c.max_pages * c.page_size > 0x7fffffffLL - (kDecodeMaxSplits + 2) * kDecodeKB) return FA2_ERR_INVALID_SHAPE;
        if (c.n_splits < 0 || c.n_splits > kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
        kv_capacity = c.max_pages * c.page_size;
    } else {
        if (kv_capacity <= 0) return FA2_ERR_INVALID_SHAPE;
        if (c.n_splits < 0 || c.n_splits > kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
        if ((long long)kv_capacity * c.head_dim * (fp8 ? 1 : 2) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    }
    if (c.window_left < -1) return FA2_ERR_INVALID_SHAPE;
    if ((long long)c.total_q * c.H_q > 0x7fffffffLL - kExtendRows) return FA2_ERR_INVALID_SHAPE;      // the rows of O and L
    if (c.head_dim != 64 && c.head_dim != 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    if (c.dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (!fp8 && (c.kv_dtype != FA2_DTYPE_BF16 || c.k_descale || c.v_descale)) return FA2_ERR_UNSUPPORTED_DTYPE;
    const int n_splits = c.n_splits ? c.n_splits
                                    : fa2_extend_ragged_num_splits(c.B, c.H_q, c.H_kv, c.total_q, kv_capacity, c.head_dim, c.window_left);
    const long long max_blocks = extend_ragged_max_blocks(c.B, c.H_q, c.H_kv, c.total_q);
    if (max_blocks * c.H_kv > 0x7fffffffLL / n_splits) return FA2_ERR_INVALID_SHAPE;
    const size_t need = n_splits > 1 ? ragged_partials_bytes(c.H_q, c.total_q, c.head_dim, n_splits) : 0;
    if (n_splits > 1 && !need) return FA2_ERR_INVALID_SHAPE;
    if (c.plan_bytes < fa2_extend_ragged_plan_bytes(c.B, c.H_q, c.H_kv, c.total_q) || ((uintptr_t)c.plan & 15)) return FA2_ERR_WORKSPACE;
    if (n_splits > 1 && (!c.ws || c.ws_bytes < need || ((uintptr_t)c.ws & 15))) return FA2_ERR_WORKSPACE;
    if (c.window_left >= 0 && !c.causal) return FA2_ERR_UNSUPPORTED;      // (whatever the capacity: the window is a causal one)
    ExtendRaggedArgs x{};
    DecodeArgs& a = x.a;
    a.Q = c.Q; a.K = c.K; a.V = c.V; a.seqlens = c.seqlens_k; a.sink = c.sink; a.O = c.O; a.L = c.L;
    a.wsO = (float*)c.ws;
    a.wsL = n_splits > 1 ? (float*)c.ws + (size_t)n_splits * c.total_q * c.H_q * c.head_dim : nullptr;
    a.B = c.B; a.Hq = c.H_q; a.Hkv = c.H_kv; a.Nq = 1; a.Ncap = kv_capacity; a.n_splits = n_splits;
    a.scale = c.scale; a.causal = c.causal ? 1 : 0;
    if (paged) { a.block_table = c.block_table; a.n_pages = c.n_pages; a.page_size = c.page_size; a.max_pages = c.max_pages; }
    a.kv_fp8 = fp8; a.k_descale = c.k_descale; a.v_descale = c.v_descale;
    a.window_left = ragged_window(c.window_left, kv_capacity);
    x.plan = (const int*)c.plan; x.T = c.total_q; x.max_blocks = (int)max_blocks; x.q_stride = c.q_stride;
    return ragged_hip_status(launch_extend_ragged(x, c.head_dim, (hipStream_t)c.stream));
}

}  // namespace
}  // namespace fa2

extern "C" {

long long fa2_extend_ragged_max_blocks(int B, int H_q, int H_kv, int total_q)
{
    if (!fa2::ragged_dims(B, H_q, H_kv, total_q)) return 0;
    return fa2::extend_ragged_max_blocks(B, H_q, H_kv, total_q);
}

size_t fa2_extend_ragged_plan_bytes(int B, int H_q, int H_kv, int total_q)
{
    if (!fa2::ragged_dims(B, H_q, H_kv, total_q)) return 0;
    const size_t ints = fa2::kRaggedPlanHeader + 2 * (size_t)B + 2 * (size_t)fa2::extend_ragged_max_blocks(B, H_q, H_kv, total_q);
    return (ints * sizeof(int) + 15) & ~(size_t)15;
}

int fa2_extend_ragged_plan(const int* cu_seqlens_q, int B, int H_q, int H_kv, int total_q, void* plan, size_t plan_bytes, void* stream)
{
    if (!cu_seqlens_q || !plan) return FA2_ERR_NULL_POINTER;
    if (!fa2::ragged_dims(B, H_q, H_kv, total_q)) return FA2_ERR_INVALID_SHAPE;
    if (fa2::extend_ragged_max_blocks(B, H_q, H_kv, total_q) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    if (plan_bytes < fa2_extend_ragged_plan_bytes(B, H_q, H_kv, total_q) || ((uintptr_t)plan & 15)) return FA2_ERR_WORKSPACE;
    return fa2::ragged_hip_status(fa2::launch_extend_ragged_plan(cu_seqlens_q, B, H_q / H_kv, total_q, (int*)plan, (hipStream_t)stream));
}

int fa2_extend_ragged_num_splits(int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, int window_left)
{
    if (!fa2::ragged_dims(B, H_q, H_kv, total_q) || kv_capacity <= 0) return 1;
    const int w = fa2::ragged_window(window_left, kv_capacity);
    const long long span = w < 0 ? kv_capacity : std::min<long long>(kv_capacity, (long long)w + total_q + (fa2::kDecodeKB - 1));
    const long long blocks = ((long long)(H_q / H_kv) * total_q + fa2::kExtendRows - 1) / fa2::kExtendRows;
    const long long groups = H_kv * std::max<long long>(std::min(B, total_q), blocks);      // the workgroups of a full batch, at least
    const long long fill = (fa2::kDecodeCUs + groups - 1) / groups;
    const long long room = std::max<long long>(1, span / fa2::kDecodeMinSplitKeys);
    return (int)std::min<long long>(std::min(fill, room), fa2::kDecodeMaxSplits);
}

size_t fa2_extend_ragged_workspace_bytes(int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, int n_splits,
                                         int window_left)
{
    if (!fa2::ragged_dims(B, H_q, H_kv, total_q) || kv_capacity <= 0 || head_dim <= 0) return 0;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return 0;
    if (n_splits == 0) n_splits = fa2_extend_ragged_num_splits(B, H_q, H_kv, total_q, kv_capacity, head_dim, window_left);
    if (n_splits == 1) return 0;
    return fa2::ragged_partials_bytes(H_q, total_q, head_dim, n_splits);
}

int fa2_forward_extend_ragged(const void* Q, long long q_token_stride, const void* K_cache, const void* V_cache,
                              const void* plan, size_t plan_bytes, const int* seqlens_k, const float* sink,
                              const float* k_descale, const float* v_descale, void* O, float* L,
                              int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, float softmax_scale,
                              int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes,
                              void* stream, int window_left)
{
    return fa2::ragged_run({Q, q_token_stride, K_cache, V_cache, nullptr, plan, plan_bytes, seqlens_k, sink, k_descale, v_descale, O, L,
                            B, H_q, H_kv, total_q, kv_capacity, 0, 0, 0, head_dim, softmax_scale, dtype, kv_dtype, causal, n_splits,
                            workspace, workspace_bytes, stream, window_left}, false);
}

int fa2_forward_extend_ragged_paged(const void* Q, long long q_token_stride, const void* K_pages, const void* V_pages,
                                    const int* block_table, const void* plan, size_t plan_bytes, const int* seqlens_k,
                                    const float* sink, const float* k_descale, const float* v_descale, void* O, float* L,
                                    int B, int H_q, int H_kv, int total_q, int n_pages, int page_size, int max_pages_per_seq,
                                    int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                                    void* workspace, size_t workspace_bytes, void* stream, int window_left)
{
    return fa2::ragged_run({Q, q_token_stride, K_pages, V_pages, block_table, plan, plan_bytes, seqlens_k, sink, k_descale, v_descale, O, L,
                            B, H_q, H_kv, total_q, 0, n_pages, page_size, max_pages_per_seq, head_dim, softmax_scale, dtype, kv_dtype,
                            causal, n_splits, workspace, workspace_bytes, stream, window_left}, true);
}

}  // extern "C"
