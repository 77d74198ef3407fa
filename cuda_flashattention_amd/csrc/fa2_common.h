// fa2_common.h -- device-side building blocks shared by the gfx950 FA2 kernels.
//
// Everything here is written for CDNA4 / gfx950 only: wave64, v_mfma_f32_32x32x16_bf16,
// ds_read_b64_tr_b16, v_permlane32_swap, 160 KiB LDS per CU.  There is no other target.
//
// It replaces the reference's scalar device helpers -- warp_reduce_sum / warp_reduce_max
// (src/util/cuda_helper.h:21-37) and load_Q_tile / process_kv_block
// (src/util/attention_helper.h:6-132) -- with MFMA fragments: the per-row reductions those
// helpers do with 32-lane shuffle butterflies become in-lane reductions over an MFMA
// accumulator column plus ONE cross-half permlane32_swap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace fa2 {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr float kLog2e = 1.4426950408889634f;

// ---------------------------------------------------------------------------------------
// LDS image of a [rows][D] bf16 tile that serves BOTH kinds of MFMA operand read:
//   * row reads   (ds_read_b128, 8 consecutive elements of one row), and
//   * transposed reads (ds_read_b64_tr_b16, 4 rows x 16 columns delivered column-major).
// `ch` is the 16-byte chunk index inside the row.  The XOR spreads a 16-lane b128 group
// (16 different rows, same chunk) over all 16 slots of the 256-B bank row, and a 32-lane
// tr-read half (4 rows x 4 chunks) over all 64 banks: both conflict-free under the gfx950
// bank rules (tools/lds_bank_sim.py checks exactly this function).
// ---------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ int lds_off(int row, int ch)
{
    static_assert(D == 64 || D == 128, "head_dim must be 64 or 128");
    if constexpr (D == 128)
        return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
    else
        return 128 * row + 16 * (ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)));
}

// LDS-DMA writes a wave's 1 KiB piece (64 / (D / 8) rows starting at tile row `row0`) LINEARLY: lane l -> row l / CPR, slot
// l % CPR.  For the result to be the lds_off image the slot must receive chunk (slot ^ swizzle(row)), so the SOURCE offset of
// the lane is permuted.  The swizzle depends on the row modulo 16 only: one per-lane offset serves every piece of the wave.
template <int D>
__device__ __forceinline__ int lds_dma_off(int row0, int lane)
{
    constexpr int ROWB = 2 * D, CPR = D / 8;
    const int drow = lane / CPR, dslot = lane % CPR, prow = row0 + drow;
    return drow * ROWB + 16 * ((lds_off<D>(prow, dslot) - ROWB * prow) >> 4);
}

template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
// f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N-1>{})
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f)
{
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ float half_max(float x)
{
    const uint32_t u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

__device__ __forceinline__ float half_sum(float x)
{
    const uint32_t u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Accumulator row (0..31) held in register r of lane-half h of a 32x32 MFMA result.
__device__ __forceinline__ constexpr int acc_row(int r, int h)
{
    return (r & 3) + 8 * (r >> 2) + 4 * h;
}

// XCD-aware work mapping.  Workgroups are dealt round-robin over the 8 XCDs (bid % 8 labels
// the group sharing an L2).  All row-blocks of one head re-read that head's K and V, so the
// j-th workgroup of XCD-group x is given head (j / nrb) * 8 + x: the 32 CUs of one XCD work
// through the row-blocks of ONE head at a time and its K/V stay in that XCD's 4 MiB L2.
// Falls back to the plain order when the head count is not a multiple of 8 (still bijective).
__device__ __forceinline__ void map_block(int bid, int n_heads, int nrb, int& head, int& rb)
{
    if ((n_heads & 7) == 0) {
        const int x = bid & 7, j = bid >> 3;
        head = (j / nrb) * 8 + x;
        rb = j % nrb;
    } else {
        head = bid / nrb;
        rb = bid % nrb;
    }
}

// One entry of a table that every lane of the workgroup reads at the same index (the packed launches' work items), word by
// word through readfirstlane: the values are wave-uniform and the compiler knows it -- they end up in buffer resources and
// in branches around workgroup barriers.
template <typename Item>
__device__ __forceinline__ Item uniform_item(const Item* items, int i)
{
    static_assert(sizeof(Item) % sizeof(int) == 0 && alignof(Item) == alignof(int), "a table of ints");
    constexpr int W = sizeof(Item) / sizeof(int);
    const int* src = reinterpret_cast<const int*>(items + i);
    int w[W];
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = __builtin_amdgcn_readfirstlane(src[k]);
    Item it;
    __builtin_memcpy(&it, w, sizeof(Item));
    return it;
}

}  // namespace fa2