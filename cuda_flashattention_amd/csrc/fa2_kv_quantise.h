// fa2_kv_quantise.h -- the e4m3 quantiser of the KV-cache writers (fa2_kv_append.hip, fa2_rope_append.hip): eight bf16 of a
// row -> eight OCP e4m3 codes, clamp(float(x) / descale, +-448) rounded to nearest even.  One definition, so the two writers
// store the same byte for the same bf16 value and descale (include/fa2_kvcache_mi355x.h, VALUES).
// x -> float (exact), a correctly rounded fp32 division by the head's descale, v_med3_f32 against +-448 -- which returns
// a bound for a NaN operand, hence the select that keeps the NaN --, then v_cvt_pk_fp8_f32 (round to nearest even; NaN -> 0x7F
// or 0xFF).  +-inf is clamped to +-448; -0.0 / descale = -0.0 keeps its sign through all three.
#ifndef FA2_KV_QUANTISE_H
#define FA2_KV_QUANTISE_H

#include "fa2_common.h"

namespace fa2 {

namespace {

constexpr float kE4m3Max = 448.0f;

__device__ __forceinline__ float kv_e4m3_operand(float x, float descale)
{
    const float y = x / descale;
    const float c = __builtin_amdgcn_fmed3f(y, -kE4m3Max, kE4m3Max);
    return y != y ? y : c;
}

// Eight bf16 (four words, ascending) -> eight e4m3 codes (two words, ascending bytes).
__device__ __forceinline__ u32x2 kv_quantise8(const u32x4& w, float descale)
{
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = kv_e4m3_operand(__uint_as_float(w[i] << 16), descale);
        f[2 * i + 1] = kv_e4m3_operand(__uint_as_float(w[i] & 0xffff0000u), descale);
    }
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    return u32x2{(uint32_t)lo, (uint32_t)hi};
}

}  // namespace

}  // namespace fa2

#endif  // FA2_KV_QUANTISE_H
