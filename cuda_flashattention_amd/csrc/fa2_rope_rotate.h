// fa2_rope_rotate.h -- the rotation of the rotary-embedding appends (fa2_rope_append.hip, fa2_rope_append_ragged.hip;
// include/fa2_rope_mi355x.h, ARITHMETIC): bf16 words widened to fp32, rotated, rounded back, eight elements of a lane at a time.
// Device code, included by both kernel files, so one expression serves the uniform and the ragged call bit for bit.
// Each product and each sum is one fp32 rounding: `#pragma clang fp contract(off)` in the two rotation functions (hipcc contracts
// a*b + c*d into a fused multiply-add by default, which rounds once less and changes bits).  x1*c - x2*s of a rotate-half row is
// formed as x1*c + (-x2)*s: the negation is exact, so the bits are the same, and one function serves both halves of the row.
#ifndef FA2_ROPE_ROTATE_H
#define FA2_ROPE_ROTATE_H

#include "fa2_common.h"

namespace fa2 {

namespace {

typedef __attribute__((ext_vector_type(2))) __bf16 rope_bf16x2;

__device__ __forceinline__ float rope_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float rope_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// two fp32 -> two bf16 in one word, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t rope_pack(float lo, float hi)
{
    const rope_bf16x2 v{(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

// Rotate-half: eight elements x of one half of a row, their partners p in the other half WITH THE SIGN ALREADY SET (negated for
// the first half), the eight table columns they share: y = bf16(fl(fl(x*cos) + fl(p*sin))).
__device__ __forceinline__ u32x4 rope_rotate_half8(const u32x4& x, const u32x4& p, const f32x4& c0, const f32x4& c1,
                                                   const f32x4& s0, const f32x4& s1)
{
#pragma clang fp contract(off)
    const float cs[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    const float sn[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
    u32x4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a0 = rope_lo(x[i]) * cs[2 * i], b0 = rope_lo(p[i]) * sn[2 * i];
        const float a1 = rope_hi(x[i]) * cs[2 * i + 1], b1 = rope_hi(p[i]) * sn[2 * i + 1];
        y[i] = rope_pack(a0 + b0, a1 + b1);
    }
    return y;
}

// Interleaved: word i of the chunk is the pair (x1, x2) of table column 4 c + i: y1 = x1*cos - x2*sin, y2 = x2*cos + x1*sin.
__device__ __forceinline__ u32x4 rope_rotate_pairs8(const u32x4& x, const f32x4& cs, const f32x4& sn)
{
#pragma clang fp contract(off)
    u32x4 y;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x1 = rope_lo(x[i]), x2 = rope_hi(x[i]);
        const float a1 = x1 * cs[i], b1 = x2 * sn[i];
        const float a2 = x2 * cs[i], b2 = x1 * sn[i];
        y[i] = rope_pack(a1 - b1, a2 + b2);
    }
    return y;
}

}  // namespace

}  // namespace fa2

#endif  // FA2_ROPE_ROTATE_H
