// fa2_norm_rope_append_ragged.hip -- the ragged rotary-embedding KV-cache append WITH A PER-HEAD RMSNorm of every new Q row and
// K row in front of the rotation (fa2_norm_rope_kv_append_ragged, _paged; include/fa2_rope_norm_mi355x.h): what models that
// normalise queries and keys per head before the rotation (Qwen3, Gemma 3) need between the fused QKV projection and attention,
// in the ONE launch of fa2_rope_append_ragged.hip.  V is copied untouched.
//
// The unit loop is fa2_rope_ragged_unit.h, the sibling's, instantiated WITH the norm of fa2_qk_norm.h: the same work split, grid
// cap and two passes per unit, the same ownership, addresses, write-or-drop rule and rotation.  The norm works on the registers
// the loop already holds; its butterfly over a row's d / 8 lanes is ds_swizzle, a lane permute (no LDS is allocated), and each lane's weights
// are loaded once per wave.  The call is bit for bit the sibling applied to the normalised bf16 tensors.
#include "fa2_rope_norm_mi355x.h"
#include "fa2_rope_ragged_unit.h"

#include <cmath>

namespace fa2 {

namespace {

template <int D, bool FP8, bool PAGED, bool INTERLEAVED>
__global__ __launch_bounds__(256) void fa2_norm_rope_append_ragged_kernel(const RopeNormRaggedArgs a)
{
    rope_ragged_units<D, FP8, PAGED, INTERLEAVED, true>(a);
}

template <int D, bool FP8, bool PAGED, bool INTERLEAVED>
hipError_t norm_rope_ragged_launch(const RopeNormRaggedArgs& a, hipStream_t stream)
{
    return rope_ragged_launch_units<D>(a, fa2_norm_rope_append_ragged_kernel<D, FP8, PAGED, INTERLEAVED>, stream);
}

template <int D, bool PAGED>
hipError_t norm_rope_ragged_pick(const RopeNormRaggedArgs& a, bool fp8, bool interleaved, hipStream_t stream)
{
    if (fp8)
        return interleaved ? norm_rope_ragged_launch<D, true, PAGED, true>(a, stream) : norm_rope_ragged_launch<D, true, PAGED, false>(a, stream);
    return interleaved ? norm_rope_ragged_launch<D, false, PAGED, true>(a, stream) : norm_rope_ragged_launch<D, false, PAGED, false>(a, stream);
}

template <bool PAGED>
hipError_t norm_rope_ragged_dispatch(const RopeNormRaggedArgs& a, int d, bool fp8, bool interleaved, hipStream_t stream)
{
    if (d == 128) return norm_rope_ragged_pick<128, PAGED>(a, fp8, interleaved, stream);
    if (d == 64) return norm_rope_ragged_pick<64, PAGED>(a, fp8, interleaved, stream);
    return hipErrorInvalidValue;
}

// the weights' pointers: k_weight always, q_weight wherever there are Q heads
inline bool norm_rope_null(const float* q_weight, const float* k_weight, int H_q) { return !k_weight || (!q_weight && H_q > 0); }

// eps finite and > 0, the weights 16-byte aligned: the sibling's FA2_ERR_INVALID_SHAPE class
inline bool norm_rope_bad(const float* q_weight, const float* k_weight, float eps)
{
    return !std::isfinite(eps) || !(eps > 0.0f) || rope_ragged_misaligned(q_weight) || rope_ragged_misaligned(k_weight);
}

}  // namespace

}  // namespace fa2

extern "C" {

int fa2_norm_rope_kv_append_ragged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                                   const float* cos_table, const float* sin_table, const float* q_weight, const float* k_weight,
                                   float eps, const void* plan, size_t plan_bytes,
                                   const int* seqlens_k, const float* k_descale, const float* v_descale,
                                   int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim,
                                   int rot_dim, int n_positions, int interleaved,
                                   long long q_stride_t, long long q_stride_h, long long new_stride_t, long long new_stride_h,
                                   int dtype, int kv_dtype, void* stream)
{
    if (fa2::rope_ragged_null(Q, Q_out, H_q, K_new, V_new, K_cache, V_cache, cos_table, sin_table, rot_dim, plan, seqlens_k) ||
        fa2::norm_rope_null(q_weight, k_weight, H_q))
        return FA2_ERR_NULL_POINTER;
    if (fa2::rope_ragged_bad_contiguous(B, H_q, H_kv, total_q, kv_capacity, head_dim, kv_dtype)) return FA2_ERR_INVALID_SHAPE;
    if (fa2::norm_rope_bad(q_weight, k_weight, eps)) return FA2_ERR_INVALID_SHAPE;
    fa2::RopeNormRaggedArgs a{};
    a.Q = Q; a.Qout = Q_out; a.Knew = K_new; a.Vnew = V_new; a.K = K_cache; a.V = V_cache;
    a.cos = rot_dim ? cos_table : nullptr; a.sin = rot_dim ? sin_table : nullptr;
    a.plan = (const int*)plan; a.seqlens = seqlens_k; a.k_descale = k_descale; a.v_descale = v_descale;
    a.B = B; a.Hq = Q ? H_q : 0; a.Hkv = H_kv; a.T = total_q; a.Ncap = kv_capacity; a.half = rot_dim / 2;
    a.qt = q_stride_t; a.qh = q_stride_h; a.st = new_stride_t; a.sh = new_stride_h;
    a.q_weight = a.Hq > 0 ? q_weight : k_weight; a.k_weight = k_weight; a.eps = eps;
    if (const int st = fa2::rope_ragged_check(a, kv_capacity, head_dim, rot_dim, n_positions, interleaved, dtype, kv_dtype, plan_bytes))
        return st;
    return fa2::rope_ragged_hip_status(fa2::norm_rope_ragged_dispatch<false>(a, head_dim, kv_dtype == FA2_DTYPE_FP8_E4M3, interleaved != 0,
                                                                             (hipStream_t)stream));
}

int fa2_norm_rope_kv_append_ragged_paged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                                         const int* block_table, const float* cos_table, const float* sin_table,
                                         const float* q_weight, const float* k_weight, float eps,
                                         const void* plan, size_t plan_bytes, const int* seqlens_k,
                                         const float* k_descale, const float* v_descale,
                                         int B, int H_q, int H_kv, int total_q, int n_pages, int page_size,
                                         int max_pages_per_seq, int head_dim,
                                         int rot_dim, int n_positions, int interleaved,
                                         long long q_stride_t, long long q_stride_h, long long new_stride_t, long long new_stride_h,
                                         int dtype, int kv_dtype, void* stream)
{
    if (fa2::rope_ragged_null(Q, Q_out, H_q, K_new, V_new, K_pages, V_pages, cos_table, sin_table, rot_dim, plan, seqlens_k) || !block_table ||
        fa2::norm_rope_null(q_weight, k_weight, H_q))
        return FA2_ERR_NULL_POINTER;
    if (fa2::rope_ragged_bad_paged(B, H_q, H_kv, total_q, n_pages, page_size, max_pages_per_seq, head_dim)) return FA2_ERR_INVALID_SHAPE;
    if (fa2::norm_rope_bad(q_weight, k_weight, eps)) return FA2_ERR_INVALID_SHAPE;
    fa2::RopeNormRaggedArgs a{};
    a.Q = Q; a.Qout = Q_out; a.Knew = K_new; a.Vnew = V_new; a.K = K_pages; a.V = V_pages;
    a.cos = rot_dim ? cos_table : nullptr; a.sin = rot_dim ? sin_table : nullptr;
    a.plan = (const int*)plan; a.seqlens = seqlens_k; a.block_table = block_table; a.k_descale = k_descale; a.v_descale = v_descale;
    a.B = B; a.Hq = Q ? H_q : 0; a.Hkv = H_kv; a.T = total_q; a.Ncap = max_pages_per_seq * page_size; a.half = rot_dim / 2;
    a.n_pages = n_pages; a.page_size = page_size; a.max_pages = max_pages_per_seq;
    a.qt = q_stride_t; a.qh = q_stride_h; a.st = new_stride_t; a.sh = new_stride_h;
    a.q_weight = a.Hq > 0 ? q_weight : k_weight; a.k_weight = k_weight; a.eps = eps;
    if (const int st = fa2::rope_ragged_check(a, a.Ncap, head_dim, rot_dim, n_positions, interleaved, dtype, kv_dtype, plan_bytes))
        return st;
    return fa2::rope_ragged_hip_status(fa2::norm_rope_ragged_dispatch<true>(a, head_dim, kv_dtype == FA2_DTYPE_FP8_E4M3, interleaved != 0,
                                                                            (hipStream_t)stream));
}

}  // extern "C"
