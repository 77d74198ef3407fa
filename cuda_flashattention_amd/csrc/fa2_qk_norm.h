// fa2_qk_norm.h -- the per-head RMSNorm in front of the rotation of fa2_norm_rope_kv_append_ragged, _paged
// (fa2_norm_rope_append_ragged.hip; include/fa2_rope_norm_mi355x.h, ARITHMETIC).  A row of d bf16 elements lies in d / 8 adjacent
// lanes, eight elements a lane; every step below is one IEEE fp32 operation, in the header's order:
//   q_i = fl(x_i * x_i); the lane's eight summed left to right; a butterfly over the row's lanes (s += s[lane ^ m], m = 1, 2, 4
//   and 8 at d = 128: fp32 addition commutes, so every lane of the row ends with the same bits);
//   r = fl(1 / fl(sqrt(fl(fl(s * (1 / d)) + eps)))), sqrtf and / correctly rounded under the shipped flags, never a native rsqrt;
//   n_i = bf16(fl(fl(x_i * r) * w_i)), ONE rounding to bf16, to nearest even.
// `#pragma clang fp contract(off)` in every function, as in fa2_rope_rotate.h: hipcc contracts a*b + c into a fused multiply-add
// by default, which rounds once less and changes bits.  The butterfly is ds_swizzle (lane permutes; no LDS is allocated) and
// must be reached by EVERY lane of the wave: qk_norm_rstd is called outside any branch that depends on the lane.
#ifndef FA2_QK_NORM_H
#define FA2_QK_NORM_H

#include "fa2_common.h"
#include "fa2_rope_rotate.h"

namespace fa2 {

namespace {

// steps 1 and 2: the sum of the squares of a lane's eight elements, left to right
__device__ __forceinline__ float qk_norm_sumsq8(const u32x4& x)
{
#pragma clang fp contract(off)
    float s = rope_lo(x[0]) * rope_lo(x[0]);
    s = s + rope_hi(x[0]) * rope_hi(x[0]);
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        s = s + rope_lo(x[i]) * rope_lo(x[i]);
        s = s + rope_hi(x[i]) * rope_hi(x[i]);
    }
    return s;
}

// the value of lane ^ m, m < 32: ds_swizzle in its bit mode (and 0x1f, or 0, xor m) -- a lane permute, no LDS is touched
template <int M>
__device__ __forceinline__ float qk_norm_xor_lane(float v)
{
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (M << 10) | 0x1f));
}

// steps 3 and 4: the row's sum over its D / 8 lanes, then r.  Every lane of the wave calls this.
template <int D>
__device__ __forceinline__ float qk_norm_rstd(float s, float eps)
{
#pragma clang fp contract(off)
    s = s + qk_norm_xor_lane<1>(s);
    s = s + qk_norm_xor_lane<2>(s);
    s = s + qk_norm_xor_lane<4>(s);
    if constexpr (D == 128) s = s + qk_norm_xor_lane<8>(s);
    const float mean = s * (1.0f / D);      // 1 / D is a power of two
    const float v = mean + eps;
    return 1.0f / sqrtf(v);
}

// step 5: eight elements scaled by r and by their eight weights, rounded once to bf16
__device__ __forceinline__ u32x4 qk_norm_scale8(const u32x4& x, float r, const f32x4& w0, const f32x4& w1)
{
#pragma clang fp contract(off)
    const float w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
    u32x4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = rope_lo(x[i]) * r, b = rope_hi(x[i]) * r;
        y[i] = rope_pack(a * w[2 * i], b * w[2 * i + 1]);
    }
    return y;
}

}  // namespace

}  // namespace fa2

#endif  // FA2_QK_NORM_H
