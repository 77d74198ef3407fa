// fa2_extend.hip -- the C entry points of extend attention (include/fa2_extend_mi355x.h): the decode calls for any number of
// query rows per K/V head.  Host code only: M = (H_q / H_kv) q_len <= 32 IS the sibling's call (fa2_forward_decode_window /
// _paged_window, fa2_capi.cpp), anything larger is checked here in the siblings' order and goes to launch_extend (fa2_decode.hip,
// extend_split_body).  Nothing here reads a length, a table or a descale.
#include "fa2_extend_mi355x.h"
#include "fa2_launch.h"

#include <algorithm>
#include <stdint.h>

namespace fa2 {
namespace {

inline int extend_hip_status(hipError_t e) { return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e; }

// more rows per K/V head than the siblings take; false for arguments the siblings refuse anyway (they say why)
inline bool extend_rows(int H_q, int H_kv, int q_len)
{
    return H_q > 0 && H_kv > 0 && q_len > 0 && H_q % H_kv == 0 && (long long)(H_q / H_kv) * q_len > kDecodeMaxRows;
}

inline long long extend_row_blocks(int H_q, int H_kv, int q_len)
{
    return ((long long)(H_q / H_kv) * q_len + kExtendRows - 1) / kExtendRows;
}

// the window a call runs with: -1 unless it can exclude a key of a full cache (the siblings' rule)
inline int extend_window(int window_left, int kv_capacity)
{
    return window_left < 0 || window_left >= kv_capacity - 1 ? -1 : window_left;
}

// n_splits B H_q q_len (head_dim + 1) floats rounded up to 256 bytes; 0: it does not fit
inline size_t extend_partials_bytes(int B, int H_q, int q_len, int head_dim, int n_splits)
{
    const unsigned __int128 bytes = (unsigned __int128)n_splits * B * H_q * q_len * ((unsigned)head_dim + 1) * sizeof(float);
    if (bytes > SIZE_MAX / 2) return 0;
    return ((size_t)bytes + 255) & ~(size_t)255;
}

struct ExtendCall {
    const void* Q; const void* K; const void* V; const int* block_table; const int* seqlens_k; const float* sink;
    const float* k_descale; const float* v_descale; void* O; float* L;
    int B, H_q, H_kv, q_len, kv_capacity, n_pages, page_size, max_pages, head_dim;
    float scale;
    int dtype, kv_dtype, causal, n_splits;
    void* ws; size_t ws_bytes; void* stream;
    int window_left;
};

// M > 32: the siblings' checks in the siblings' order (decode_contiguous / decode_paged, fa2_capi.cpp), without the row limit
int extend_run(const ExtendCall& c, bool paged)
{
    if (!c.Q || !c.K || !c.V || !c.O || !c.L || (paged && !c.block_table)) return FA2_ERR_NULL_POINTER;
    if (c.B <= 0 || c.H_q <= 0 || c.q_len <= 0 || c.head_dim <= 0 || !(c.scale > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    if ((long long)c.B * c.H_q > 0x7fffffffLL / 64 || (long long)c.q_len * c.head_dim * 4 > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    if (c.H_kv <= 0 || c.H_q % c.H_kv) return FA2_ERR_INVALID_SHAPE;
    const bool fp8 = c.kv_dtype == FA2_DTYPE_FP8_E4M3;
    int kv_capacity = c.kv_capacity;
    if (paged) {
        if (c.n_pages <= 0 || c.page_size <= 0 || c.max_pages <= 0 || c.page_size % kDecodeTile) return FA2_ERR_INVALID_SHAPE;
        // key indices are ints, and the kernel forms begin = split chunk <= len + n_splits kDecodeKB and kb + 4 kDecodeKB
        if ((long long)c.max_pages * c.page_size > 0x7fffffffLL - (kDecodeMaxSplits + 2) * kDecodeKB) return FA2_ERR_INVALID_SHAPE;
        if (c.n_splits < 0 || c.n_splits > kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
        kv_capacity = c.max_pages * c.page_size;
    } else {
        if (kv_capacity <= 0) return FA2_ERR_INVALID_SHAPE;
        if (c.n_splits < 0 || c.n_splits > kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
        // one (b, head) slab, one buffer resource: 2 bytes per element, 1 in an e4m3 cache
        if ((long long)kv_capacity * c.head_dim * (fp8 ? 1 : 2) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    }
    if (c.window_left < -1) return FA2_ERR_INVALID_SHAPE;
    if ((long long)c.B * c.H_q * c.q_len > 0x7fffffffLL - kExtendRows) return FA2_ERR_INVALID_SHAPE;      // the rows of O and L
    if (c.head_dim != 64 && c.head_dim != 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    if (c.dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (!fp8 && (c.kv_dtype != FA2_DTYPE_BF16 || c.k_descale || c.v_descale)) return FA2_ERR_UNSUPPORTED_DTYPE;
    const int n_splits =
        c.n_splits ? c.n_splits : fa2_extend_num_splits(c.B, c.H_q, c.H_kv, c.q_len, kv_capacity, c.head_dim, c.window_left);
    if ((long long)c.B * c.H_kv * extend_row_blocks(c.H_q, c.H_kv, c.q_len) > 0x7fffffffLL / n_splits) return FA2_ERR_INVALID_SHAPE;
    const size_t need = n_splits > 1 ? extend_partials_bytes(c.B, c.H_q, c.q_len, c.head_dim, n_splits) : 0;
    if (n_splits > 1 && !need) return FA2_ERR_INVALID_SHAPE;
    if (n_splits > 1 && (!c.ws || c.ws_bytes < need || ((uintptr_t)c.ws & 15))) return FA2_ERR_WORKSPACE;
    if (c.window_left >= 0 && !c.causal) return FA2_ERR_UNSUPPORTED;      // (whatever the capacity: the window is a causal one)
    DecodeArgs a{};
    a.Q = c.Q; a.K = c.K; a.V = c.V; a.seqlens = c.seqlens_k; a.sink = c.sink; a.O = c.O; a.L = c.L;
    a.wsO = (float*)c.ws;
    a.wsL = n_splits > 1 ? (float*)c.ws + (size_t)n_splits * c.B * c.H_q * c.q_len * c.head_dim : nullptr;
    a.B = c.B; a.Hq = c.H_q; a.Hkv = c.H_kv; a.Nq = c.q_len; a.Ncap = kv_capacity; a.n_splits = n_splits;
    a.scale = c.scale; a.causal = c.causal ? 1 : 0;
    if (paged) { a.block_table = c.block_table; a.n_pages = c.n_pages; a.page_size = c.page_size; a.max_pages = c.max_pages; }
    a.kv_fp8 = fp8; a.k_descale = c.k_descale; a.v_descale = c.v_descale;
    a.window_left = extend_window(c.window_left, kv_capacity);
    return extend_hip_status(launch_extend(a, c.head_dim, (hipStream_t)c.stream));
}

}  // namespace
}  // namespace fa2

extern "C" {

int fa2_extend_num_splits(int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, int window_left)
{
    if (!fa2::extend_rows(H_q, H_kv, q_len)) return fa2_decode_window_num_splits(B, H_kv, q_len, kv_capacity, head_dim, window_left);
    if (B <= 0 || kv_capacity <= 0) return 1;
    const int w = fa2::extend_window(window_left, kv_capacity);
    const long long span = w < 0 ? kv_capacity : std::min<long long>(kv_capacity, (long long)w + q_len + (fa2::kDecodeKB - 1));
    const long long groups = (long long)B * H_kv * fa2::extend_row_blocks(H_q, H_kv, q_len);      // (three ints and a long long: no overflow)
    const long long fill = (fa2::kDecodeCUs + groups - 1) / groups;             // smallest s with groups x s >= the CU count
    const long long room = std::max<long long>(1, span / fa2::kDecodeMinSplitKeys);
    return (int)std::min<long long>(std::min(fill, room), fa2::kDecodeMaxSplits);
}

size_t fa2_extend_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, int n_splits, int window_left)
{
    if (B <= 0 || H_q <= 0 || H_kv <= 0 || q_len <= 0 || kv_capacity <= 0 || head_dim <= 0) return 0;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return 0;
    if (n_splits == 0) n_splits = fa2_extend_num_splits(B, H_q, H_kv, q_len, kv_capacity, head_dim, window_left);
    if (n_splits == 1) return 0;
    return fa2::extend_partials_bytes(B, H_q, q_len, head_dim, n_splits);
}

int fa2_forward_extend(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                       const float* k_descale, const float* v_descale, void* O, float* L,
                       int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                       int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream,
                       int window_left)
{
    if (!fa2::extend_rows(H_q, H_kv, q_len))
        return fa2_forward_decode_window(Q, K_cache, V_cache, seqlens_k, sink, k_descale, v_descale, O, L, B, H_q, H_kv, q_len, kv_capacity,
                                         head_dim, softmax_scale, dtype, kv_dtype, causal, n_splits, workspace, workspace_bytes, stream,
                                         window_left);
    return fa2::extend_run({Q, K_cache, V_cache, nullptr, seqlens_k, sink, k_descale, v_descale, O, L, B, H_q, H_kv, q_len, kv_capacity,
                            0, 0, 0, head_dim, softmax_scale, dtype, kv_dtype, causal, n_splits, workspace, workspace_bytes, stream,
                            window_left}, false);
}

int fa2_forward_extend_paged(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                             const int* seqlens_k, const float* sink, const float* k_descale, const float* v_descale,
                             void* O, float* L,
                             int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                             int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                             void* workspace, size_t workspace_bytes, void* stream, int window_left)
{
    if (!fa2::extend_rows(H_q, H_kv, q_len))
        return fa2_forward_decode_paged_window(Q, K_pages, V_pages, block_table, seqlens_k, sink, k_descale, v_descale, O, L, B, H_q, H_kv,
                                               q_len, n_pages, page_size, max_pages_per_seq, head_dim, softmax_scale, dtype, kv_dtype,
                                               causal, n_splits, workspace, workspace_bytes, stream, window_left);
    return fa2::extend_run({Q, K_pages, V_pages, block_table, seqlens_k, sink, k_descale, v_descale, O, L, B, H_q, H_kv, q_len, 0,
                            n_pages, page_size, max_pages_per_seq, head_dim, softmax_scale, dtype, kv_dtype, causal, n_splits, workspace,
                            workspace_bytes, stream, window_left}, true);
}

}  // extern "C"
