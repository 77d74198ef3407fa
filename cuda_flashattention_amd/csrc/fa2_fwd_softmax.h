// fa2_fwd_softmax.h -- what the two generated-body forwards (fa2_fwd1_bf16.hip, fa2_fwd_fp8.hip) do identically in compiler
// code around their bodies: the rare new-reference update of the lazy online softmax, the deferred O^T rescale, the tail of
// the ring driver and the bf16 output of eight accumulator registers.  Register numbers, register-file shape and clobber class
// (fa2_regfile.h) are the caller's.
#pragma once
#include "fa2_regfile.h"

namespace fa2 {

constexpr float kFwdRescaleThr = 6.0f;      // natural-log units of the scaled score: a lane asks for a new reference above reference + 6

template <int I> using Int = std::integral_constant<int, I>;

// A row block's softmax state in the registers its bodies name, rewritten for the reference m_new: mb = m_new log2 e (0 while
// -inf: a row with no visible key yet keeps p = 0), thr = the raw score above which a lane asks for a new reference, and the
// two partial row sums (ST_L, ST_L + 1) scaled by alpha.
template <int RF, int CL, int ST_L, int ST_MB, int ST_TH>
__device__ __forceinline__ void fwd_write_reference(float m_new, float alpha, float inv_scale)
{
    vset<RF, CL, ST_MB>(m_new == -INFINITY ? 0.0f : m_new * kLog2e);
    vset<RF, CL, ST_TH>((m_new + kFwdRescaleThr) * inv_scale);
    vset<RF, CL, ST_L>(vget<ST_L>() * alpha);
    vset<RF, CL, ST_L + 1>(vget<ST_L + 1>() * alpha);
}

// The update proper, in two steps.  `mx` is the row's maximum over the new keys (scaled, natural units), m_run its reference.
// FA2_FWD_NEW_REFERENCE declares m_new (the reference, moved if any row of the wave passed its threshold), alpha (what the
// sums and O^T scale by) and sc ("O^T needs the rescale": some row of the wave already accumulated something at an older
// reference); the caller then passes m_new and alpha to fwd_write_reference.  At this point O^T holds the products through
// block j-2 and P(j-1) is packed at the old reference: the sums are rescaled at once, O^T one body later (fwd_rescale_o).
// (A macro, and FA2_FWD_TAIL_TILES below: hipcc simplifies the body of a function on its own before it inlines it, and the
// branch structure `sc` gets that way -- or a tile lambda called through one more frame -- changes the register allocation
// of the whole fp8 kernel: ~10 000 of its 28 799 lines of assembly.  tools/asm_identity.py is the check.)
#define FA2_FWD_NEW_REFERENCE(m_run, mx)                                                                          \
    const bool grow = (mx) > (m_run) + kFwdRescaleThr; /* also true from m_run = -inf */                           \
    const bool any_grow = __any(grow);                                                                             \
    const float m_new = any_grow ? fmaxf(m_run, mx) : (m_run);                                                     \
    const bool sc = any_grow && __any((m_run) != -INFINITY && m_new != (m_run));                                   \
    const float alpha = m_new == -INFINITY ? 1.0f : __builtin_amdgcn_exp2f(((m_run) - m_new) * kLog2e)

// The deferred rescale: a[A0 : A0 + 4 N4) *= alpha (the caller has executed mfma_acc_settle()).
template <int RF, int CL, int A0, int N4>
__device__ __forceinline__ void fwd_rescale_o(float alpha)
{
    static_for<N4>([&](auto R4) { ascale4<RF, CL, A0 + 4 * decltype(R4)::value>(alpha); });
}

// The tail of the ring driver: tiles t .. ntl - 1 through the general bodies, run_tile(ring slot, flavour 1, tile); t is a
// multiple of the ring depth on entry.
#define FA2_FWD_TAIL_TILES(run_tile, t, ntl)       \
    for (; t < ntl; t += 4) {                      \
        run_tile(Int<0>{}, Int<1>{}, t);           \
        if (t + 1 >= ntl) break;                   \
        run_tile(Int<1>{}, Int<1>{}, t + 1);       \
        if (t + 2 >= ntl) break;                   \
        run_tile(Int<2>{}, Int<1>{}, t + 2);       \
        if (t + 3 >= ntl) break;                   \
        run_tile(Int<3>{}, Int<1>{}, t + 3);       \
    }

// Output of a[R : R+7] (two register quads of one 32-column tile of O^T), scaled by inv.  A lane holds 4 consecutive columns of
// its row per quad, its partner lane (+32) the next 4: for the bf16 output one v_permlane32_swap per packed dword pairs them
// up, and what comes back is the lane's own 16 contiguous bytes: columns 16 gp + 8 h .. of the tile.  (The store and its row
// guard stay with the caller: as a bool argument the guard is evaluated ahead of the packing and moves registers.)
template <int R>
__device__ __forceinline__ void fwd_read_o8(float inv, f32x4& v, f32x4& w)
{
    v[0] = aread<R>() * inv; v[1] = aread<R + 1>() * inv; v[2] = aread<R + 2>() * inv; v[3] = aread<R + 3>() * inv;
    w[0] = aread<R + 4>() * inv; w[1] = aread<R + 5>() * inv; w[2] = aread<R + 6>() * inv; w[3] = aread<R + 7>() * inv;
}
__device__ __forceinline__ u32x4 fwd_pack_o8_bf16(const f32x4& v, const f32x4& w)
{
    bf16x4 x, y;
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[e] = (__bf16)v[e]; y[e] = (__bf16)w[e]; }
    const u32x2 xu = __builtin_bit_cast(u32x2, x), yu = __builtin_bit_cast(u32x2, y);
    const auto s0 = __builtin_amdgcn_permlane32_swap(xu[0], yu[0], false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(xu[1], yu[1], false, false);
    return u32x4{s0[0], s1[0], s0[1], s1[1]};
}

}  // namespace fa2
