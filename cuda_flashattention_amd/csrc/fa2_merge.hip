// fa2_merge.hip -- merging partial attention results (fa2_merge_states / fa2_merge_states_backward, include/fa2_mi355x.h).
//
// n <= 8 parts (O_i bf16 [R][d], L_i fp32 [R]) computed over disjoint key sets become the attention over their union:
//     L = log sum_i exp L_i,    O = sum_i exp(L_i - L) O_i
// and, backward, with w_i = exp(L_i - L):
//     dO_i = w_i dO,    dL_i = w_i (dL + rowsum(dO o (O_i - O)))
// (dL_i: the part's O_i enters O with weight w_i, d w_i / d L_i = w_i (1 - w_i), d w_j / d L_i = -w_i w_j, and sum_j w_j O_j = O.)
// Both kernels are HBM-bound streams: a row is owned by d / 8 lanes (8 at d = 64, 16 at d = 128), a lane moves 16 bytes of every
// tensor, lane i of a row reads L_i once and the row's lanes pass it round by shuffles.  No LDS, no atomics, fp32 arithmetic in a
// fixed order (ascending i): the same bits on every run.  The part pointers travel by value in the argument block.
// -inf: a part whose L_i is -inf on a row saw no key there; it is left out of the row by a SELECT (its O_i may hold anything, a
// NaN included) and gets dO_i = 0, dL_i = 0.  A row on which every part is -inf has O = 0, L = -inf.
#include "fa2_common.h"
#include "fa2_launch.h"

namespace fa2 {

constexpr float kLn2 = 0.6931471805599453f;

// which[sub] for a lane-varying sub < 8 as a chain of selects (an indexed read of the argument block would go through scratch)
template <typename T>
__device__ __forceinline__ T* pick(T* const (&p)[kMergeMaxParts], int sub)
{
    T* r = p[0];
#pragma unroll
    for (int i = 1; i < kMergeMaxParts; ++i) r = sub == i ? p[i] : r;
    return r;
}

template <int D>
__global__ void __launch_bounds__(256) fa2_merge_fwd_kernel(MergeArgs a)
{
    constexpr int LPR = D / 8;                                   // lanes per row
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = t / LPR;
    const int sub = (int)(t % LPR);
    const bool live = row < a.rows;                              // (a row's lanes share it: LPR divides 64)
    const size_t at = row * D + sub * 8;
    float li = -INFINITY;
    if (live && sub < a.n) li = pick(a.L, sub)[row];
    float m = li;
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, LPR));
    const float m0 = m == -INFINITY ? 0.0f : m;
    bf16x8 o[kMergeMaxParts] = {};
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n && live) o[i] = *reinterpret_cast<const bf16x8*>((const __bf16*)a.O[i] + at);
    // -0 + x = x for every x, a zero of either sign included: one part alone comes out with the bits it came in with
    float acc[8], sum = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = -0.0f;
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i) {
        if (i < a.n) {
            const float l = __shfl(li, i, LPR);
            const bool has = l != -INFINITY;
            const float w = __builtin_amdgcn_exp2f((l - m0) * kLog2e);
            sum += has ? w : 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = has ? acc[e] + w * (float)o[i][e] : acc[e];
        }
    }
    if (!live) return;
    const bool none = m == -INFINITY;
    const float inv = 1.0f / sum;                                // exp(m - L): the weights above are relative to m.  1 part: 1 / 1
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (__bf16)(none ? 0.0f : acc[e] * inv);
    *reinterpret_cast<bf16x8*>((__bf16*)a.Oout + at) = r;
    if (sub == 0) a.Lout[row] = none ? -INFINITY : m + __builtin_amdgcn_logf(sum) * kLn2;      // (v_log_f32 is log2; 1 part: + 0)
}

template <int D>
__global__ void __launch_bounds__(256) fa2_merge_bwd_kernel(MergeBwdArgs b)
{
    constexpr int LPR = D / 8;
    const MergeArgs& a = b.m;                                    // here Oout / Lout are the merged O and L, read
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = t / LPR;
    const int sub = (int)(t % LPR);
    const bool live = row < a.rows;
    const size_t at = row * D + sub * 8;
    float li = -INFINITY, L = -INFINITY, gl = 0.0f;
    bf16x8 go = {}, om = {};
    if (live) {
        if (sub < a.n) li = pick(a.L, sub)[row];
        L = a.Lout[row];
        if (b.dL) gl = b.dL[row];
        go = *reinterpret_cast<const bf16x8*>((const __bf16*)b.dO + at);
        om = *reinterpret_cast<const bf16x8*>((const __bf16*)a.Oout + at);
    }
    bf16x8 o[kMergeMaxParts] = {};
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i)
        if (i < a.n && live) o[i] = *reinterpret_cast<const bf16x8*>((const __bf16*)a.O[i] + at);
    const float L0 = L == -INFINITY ? 0.0f : L;
    float mine = 0.0f;                                           // dL_sub of this row, kept by lane sub
#pragma unroll
    for (int i = 0; i < kMergeMaxParts; ++i) {
        if (i < a.n) {
            const float l = __shfl(li, i, LPR);
            const bool has = l != -INFINITY && L != -INFINITY;
            const float w = has ? __builtin_amdgcn_exp2f((l - L0) * kLog2e) : 0.0f;
            float s = 0.0f;
            bf16x8 r;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float g = (float)go[e];
                s += g * ((float)o[i][e] - (float)om[e]);
                r[e] = (__bf16)(has ? w * g : 0.0f);
            }
#pragma unroll
            for (int off = LPR / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, LPR);
            if (live) *reinterpret_cast<bf16x8*>((__bf16*)b.dO_parts[i] + at) = r;
            const float v = has ? w * (gl + s) : 0.0f;            // a select: an absent part's O_i (s) may be a NaN
            mine = sub == i ? v : mine;
        }
    }
    if (live && sub < a.n) pick(b.dL_parts, sub)[row] = mine;
}

static hipError_t merge_grid(size_t rows, int d, unsigned* grid)
{
    if (d != 64 && d != 128) return hipErrorInvalidValue;
    const size_t blocks = (rows * (size_t)(d / 8) + 255) / 256;
    if (rows == 0 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    *grid = (unsigned)blocks;
    return hipSuccess;
}

hipError_t launch_merge_fwd(const MergeArgs& a, int d, hipStream_t stream)
{
    unsigned grid = 0;
    const hipError_t e = merge_grid(a.rows, d, &grid);
    if (e != hipSuccess || a.n < 1 || a.n > kMergeMaxParts) return hipErrorInvalidValue;
    if (d == 128) hipLaunchKernelGGL(fa2_merge_fwd_kernel<128>, dim3(grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(fa2_merge_fwd_kernel<64>, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_merge_bwd(const MergeBwdArgs& b, int d, hipStream_t stream)
{
    unsigned grid = 0;
    const hipError_t e = merge_grid(b.m.rows, d, &grid);
    if (e != hipSuccess || b.m.n < 1 || b.m.n > kMergeMaxParts) return hipErrorInvalidValue;
    if (d == 128) hipLaunchKernelGGL(fa2_merge_bwd_kernel<128>, dim3(grid), dim3(256), 0, stream, b);
    else hipLaunchKernelGGL(fa2_merge_bwd_kernel<64>, dim3(grid), dim3(256), 0, stream, b);
    return hipGetLastError();
}

}  // namespace fa2
