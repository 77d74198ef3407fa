// fa2_rope_ragged_unit.h -- the unit loop of the ragged rotary-embedding KV-cache appends, and the host checks they share:
// fa2_rope_append_ragged.hip (fa2_rope_kv_append_ragged, _paged; include/fa2_rope_ragged_mi355x.h) instantiates it with
// NORM = false, fa2_norm_rope_append_ragged.hip (fa2_norm_rope_kv_append_ragged, _paged; include/fa2_rope_norm_mi355x.h) with
// NORM = true: the per-head RMSNorm of fa2_qk_norm.h on every new Q row and K row, in front of the rotation.  NORM is a
// compile-time switch: with it off nothing of the norm is left in the kernel.  ONE loop serves both, so ownership, addresses,
// the write-or-drop rule, Q_out's zero rows and the rotation are the same code in both calls.
//
// WORK SPLIT.  fa2_rope_append_kernel's: a row of d elements is d / 8 lanes of 16 bytes, a wave holds 64 / (d / 8) rows per pass
// and makes kRopePasses passes per unit, all loads of a unit issued before its first store.  A unit is (head j, a group of TPU
// consecutive PACKED tokens); j < H_kv is a K/V head, the others are Q heads.  j is WAVE-UNIFORM: the branch between the two kinds
// of head is a scalar one and the descales are scalar loads.  The owning sequence is NOT: a group may straddle several sequences
// and tokens no sequence owns, so each lane finds its token's owner itself (fa2_rope_ragged_owner.h: a search of ceil(log2 B)
// steps over the plan's pairs, the count a host value) and loads seqlens_k[b] with a vector load.  The grid depends on host
// values only and is capped; a wave strides over the rest.  Plain compiler code: no LDS, no atomics, no inline assembly.
// THE PLAN IS THE SAFETY CONTRACT.  A header that does not name the call's B and T (and G, with Q heads) ends every wave before
// its first store.  Ownership comes from ragged_owner and nothing else: whatever the pairs hold, an owner has 0 <= b < B and
// 0 <= i < q_b <= T, and only the B pairs are read.  A cache destination is formed by fa2_kv_append_addr.h and nothing else; a
// table row is read only for a position that passed 0 <= pos < capacity (the host has checked capacity <= n_positions); a Q_out
// row is a function of (t, head) alone, t < T.  No loop bound comes from device memory.
// ROTATION.  fa2_rope_rotate.h, the uniform call's, so a row's bits are that call's.
// NORM.  A row's lanes share its token and its head, so they are live together.  A lane that is not live holds zeros and takes
// part in the butterfly all the same (the shuffles stand outside every branch on `live`); its result is never stored.  The
// weights are constant along a lane column: each lane loads its eight of q_weight and of k_weight, and its rotate-half partner's
// eight, ONCE, before the unit loop (a call without Q heads gets q_weight = k_weight from the host).  The partner's raw chunk gets the row's r and the partner's weights: the bits the partner
// lane computes for itself, without a shuffle.
#ifndef FA2_ROPE_RAGGED_UNIT_H
#define FA2_ROPE_RAGGED_UNIT_H

#include "fa2_common.h"
#include "fa2_kv_append_addr.h"
#include "fa2_kv_quantise.h"
#include "fa2_launch.h"
#include "fa2_mi355x.h"
#include "fa2_qk_norm.h"
#include "fa2_rope_ragged_owner.h"
#include "fa2_rope_rotate.h"

#include <algorithm>

namespace fa2 {

namespace {

constexpr int kRopePasses = 2;           // rows of a lane per unit: both passes' loads are issued before the first store
constexpr int kRopeMaxBlocks = 2048;     // 256 CUs x 8 workgroups of 4 waves: a memory-bound grid is capped and strides
// what a wave reads once per unit, at a wave-uniform address: the constant address space makes these scalar loads
typedef __attribute__((address_space(4))) int rope_const_int;
typedef __attribute__((address_space(4))) float rope_const_float;

struct RopeRaggedArgs {
    const void* Q; void* Qout; const void* Knew; const void* Vnew; void* K; void* V;
    const float* cos; const float* sin;
    const int* plan; const int* seqlens; const int* block_table; const float* k_descale; const float* v_descale;
    int B, Hq, Hkv, T, Ncap;                     // Ncap: kv_capacity, or max_pages x page_size
    int n_pages, page_size, max_pages;           // paged only
    int half;                                    // rot_dim / 2: the tables' row length, a multiple of 8; 0: no rotation
    int iters;                                   // the owner search's steps: ragged_owner_iters(B)
    unsigned groups, units;                      // token groups of a head; (H_kv + H_q) x groups (rope_ragged_launch)
    long long qt, qh;                            // Q's element strides: token, head
    long long st, sh;                            // K_new's and V_new's
};

// the norm's own arguments behind the append's: only a NORM kernel takes (and reads) them
struct RopeNormRaggedArgs : RopeRaggedArgs {
    const float* q_weight; const float* k_weight;      // fp32 [head_dim]; without Q heads the host sets q_weight = k_weight
    float eps;
};

template <int D, bool FP8, bool PAGED, bool INTERLEAVED, bool NORM, class Args>
__device__ __forceinline__ void rope_ragged_units(const Args a)
{
    constexpr int LPR = D / 8;                  // lanes of a row
    constexpr int ROWS = 64 / LPR;              // rows of a wave's pass
    constexpr int TPU = ROWS * kRopePasses;     // tokens of a unit
    // the plan is the contract: a header built for another batch ends the wave before it touches anything
    const rope_const_int* const head = (const rope_const_int*)a.plan;
    if (head[0] != a.B || head[2] != a.T) return;
    if (a.Hq > 0 && head[1] != a.Hq / a.Hkv) return;
    const int* const pseq = a.plan + kRaggedPlanHeader;      // B pairs (start_b, q_b): the host checked plan_bytes
    const int lane = threadIdx.x & 63;
    const int r = lane / LPR, c = lane % LPR;
    const bool rotates = 4 * c < a.half;        // this lane's chunk lies inside rot_dim (8 c < rot_dim)
    const bool first = 8 * c < a.half;          // rotate-half: inside the first half, the x1 of its pairs
    // the lane's eight table columns (rotate-half) or four (interleaved), and its partner's chunk
    const int col = INTERLEAVED ? 4 * c : (first ? 8 * c : 8 * c - a.half);
    const int partner = first ? a.half : -a.half;
    if constexpr (NORM) {
        // what every entry point has checked on the host, said to the compiler: a known sign spares a scalar register the sign
        // word of each 64-bit product below, and the NORM kernels have none to spare (tests/test_qk_norm_isa.py: no spill)
        __builtin_assume(a.B > 0 && a.Hkv > 0 && a.Hq >= 0 && a.T > 0 && a.Ncap > 0);
        if constexpr (PAGED) __builtin_assume(a.n_pages > 0 && a.page_size > 0 && a.max_pages > 0);
    }
    // NORM: the lane's eight weights of each kind of head and, rotate-half, its partner's eight, once per wave
    f32x4 wq[2], wk[2], wqp[2], wkp[2];
    if constexpr (NORM) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // (a call without Q heads has q_weight = k_weight, set by the host: no branch on H_q here)
            wk[i] = *reinterpret_cast<const f32x4*>(a.k_weight + 8 * c + 4 * i);
            wq[i] = *reinterpret_cast<const f32x4*>(a.q_weight + 8 * c + 4 * i);
            wqp[i] = wkp[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (!INTERLEAVED) {
                if (rotates) {      // 0 <= 8 c + partner < rot_dim <= d
                    wkp[i] = *reinterpret_cast<const f32x4*>(a.k_weight + 8 * c + partner + 4 * i);
                    wqp[i] = *reinterpret_cast<const f32x4*>(a.q_weight + 8 * c + partner + 4 * i);
                }
            }
        }
    }
    // host values: (H_kv + H_q) x T is below 2^31 (rope_ragged_check) and the grid is capped, so u + step stays below 2^32
    const unsigned groups = a.groups, units = a.units;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned step = gridDim.x * 4u;
    for (unsigned u = wave; u < units; u += step) {
        const int g = (int)(u % groups), j = (int)(u / groups);
        const bool is_q = j >= a.Hkv;                                                // wave-uniform
        const int h = is_q ? j - a.Hkv : j;
        float kd = 1.0f, vd = 1.0f;
        if constexpr (FP8) {
            if (!is_q) {
                if (a.k_descale) kd = ((const rope_const_float*)a.k_descale)[h];
                if (a.v_descale) vd = ((const rope_const_float*)a.v_descale)[h];
            }
        }
        const __bf16* xsrc = (const __bf16*)(is_q ? a.Q : a.Knew);
        const long long row0 = (long long)h * (is_q ? a.qh : a.sh);
        const long long tstride = is_q ? a.qt : a.st;
        long long dst[kRopePasses];               // where the row goes (a cache, or Q_out), or dropped
        bool live[kRopePasses];                   // its position has a table row: it was loaded and is rotated
        u32x4 x[kRopePasses], xp[kRopePasses], v[kRopePasses];
        f32x4 c0[kRopePasses], c1[kRopePasses], s0[kRopePasses], s1[kRopePasses];
#pragma unroll
        for (int p = 0; p < kRopePasses; ++p) {
            const unsigned t = (unsigned)g * TPU + p * ROWS + r;      // unsigned: the last group may pass T, up to INT_MAX, by TPU - 1
            const bool in = t < (unsigned)a.T;
            int pos = -1, b = 0;
            if (in) {
                const RaggedOwner own = ragged_owner(pseq, a.B, a.iters, a.T, (int)t);
                if (own.b >= 0) {
                    b = own.b;
                    pos = kv_append_pos(a.seqlens[own.b], own.q, own.i, a.Ncap);
                }
            }
            long long to = kKvAppendDropped;
            if (is_q) {
                if (in) to = ((long long)t * a.Hq + h) * D;      // every row of Q_out is written
            } else if constexpr (PAGED) {
                if (pos >= 0) {
                    const int entry = a.block_table[(long long)b * a.max_pages + kv_append_table_index(pos, a.page_size)];
                    to = kv_append_offset_paged(pos, entry, a.n_pages, h, a.Hkv, a.page_size, D);
                }
            } else {
                to = kv_append_offset(pos, b, h, a.Hkv, a.Ncap, D);      // dropped for pos = -1
            }
            dst[p] = to;
            live[p] = to >= 0 && pos >= 0;
            const long long src = row0 + (long long)t * tstride + 8 * c;
            if constexpr (NORM) x[p] = xp[p] = u32x4{0u, 0u, 0u, 0u};      // a lane that is not live adds +0.0 to the butterfly
            if (live[p]) {
                x[p] = *reinterpret_cast<const u32x4*>(xsrc + src);
                if (!is_q) v[p] = *reinterpret_cast<const u32x4*>((const __bf16*)a.Vnew + src);      // K_new's strides are V_new's
            }
            if (live[p] && rotates) {
                const long long at = (long long)pos * a.half + col;      // pos < capacity <= n_positions (host-checked)
                c0[p] = *reinterpret_cast<const f32x4*>(a.cos + at);
                s0[p] = *reinterpret_cast<const f32x4*>(a.sin + at);
                if constexpr (!INTERLEAVED) {
                    c1[p] = *reinterpret_cast<const f32x4*>(a.cos + at + 4);
                    s1[p] = *reinterpret_cast<const f32x4*>(a.sin + at + 4);
                    xp[p] = *reinterpret_cast<const u32x4*>(xsrc + src + partner);
                }
            }
        }
        if constexpr (NORM) {
            // the row n the rotation works on: x and, rotate-half, the partner's chunk, normalised and rounded to bf16.  No branch
            // on the lane in here: a chunk past rot_dim has a partner chunk of zeros, scaled for nothing
            const f32x4 w0 = is_q ? wq[0] : wk[0], w1 = is_q ? wq[1] : wk[1];
            const f32x4 p0 = is_q ? wqp[0] : wkp[0], p1 = is_q ? wqp[1] : wkp[1];
#pragma unroll
            for (int p = 0; p < kRopePasses; ++p) {
                const float rstd = qk_norm_rstd<D>(qk_norm_sumsq8(x[p]), a.eps);      // every lane: the butterfly is in here
                x[p] = qk_norm_scale8(x[p], rstd, w0, w1);
                if constexpr (!INTERLEAVED) xp[p] = qk_norm_scale8(xp[p], rstd, p0, p1);
            }
        }
#pragma unroll
        for (int p = 0; p < kRopePasses; ++p) {
            if (dst[p] < 0) continue;
            u32x4 y = u32x4{0u, 0u, 0u, 0u};      // a Q row no sequence owns, or whose position has no table row: +0.0 throughout
            if (live[p]) {
                y = x[p];                          // past rot_dim: the source bits (NORM: the normalised row's)
                if (rotates) {
                    if constexpr (INTERLEAVED) {
                        y = rope_rotate_pairs8(x[p], c0[p], s0[p]);
                    } else {
                        const uint32_t sign = first ? 0x80008000u : 0u;
                        const u32x4 q = u32x4{xp[p][0] ^ sign, xp[p][1] ^ sign, xp[p][2] ^ sign, xp[p][3] ^ sign};
                        y = rope_rotate_half8(x[p], q, c0[p], c1[p], s0[p], s1[p]);
                    }
                }
            }
            const long long at = dst[p] + 8 * c;
            if (is_q) {
                *reinterpret_cast<u32x4*>((__bf16*)a.Qout + at) = y;
            } else if constexpr (FP8) {
                *reinterpret_cast<u32x2*>((uint8_t*)a.K + at) = kv_quantise8(y, kd);
                *reinterpret_cast<u32x2*>((uint8_t*)a.V + at) = kv_quantise8(v[p], vd);
            } else {
                *reinterpret_cast<u32x4*>((__bf16*)a.K + at) = y;
                *reinterpret_cast<u32x4*>((__bf16*)a.V + at) = v[p];
            }
        }
    }
}

// The grid of a kernel that runs rope_ragged_units<D, ...>: host values only.
template <int D, class Args, class Kernel>
hipError_t rope_ragged_launch_units(Args a, Kernel kernel, hipStream_t stream)
{
    constexpr int TPU = 64 / (D / 8) * kRopePasses;
    a.groups = (unsigned)(((long long)a.T + TPU - 1) / TPU);
    const long long units = (long long)(a.Hkv + a.Hq) * a.groups;
    a.units = (unsigned)units;
    a.iters = ragged_owner_iters(a.B);
    const unsigned grid = (unsigned)std::min<long long>((units + 3) / 4, kRopeMaxBlocks);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

inline int rope_ragged_hip_status(hipError_t e) { return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e; }

inline bool rope_ragged_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

inline bool rope_ragged_bad_stride(long long s) { return s < 0 || s % 8 != 0; }

// The pointers of the entry points: the tables are needed by a rotation only, Q and Q_out come as a pair, and only a call
// without Q heads may leave them out.
inline bool rope_ragged_null(const void* Q, const void* Q_out, int H_q, const void* K_new, const void* V_new, const void* K, const void* V,
                             const float* cos_table, const float* sin_table, int rot_dim, const void* plan, const int* seqlens_k)
{
    if (!K_new || !V_new || !K || !V || !seqlens_k || !plan) return true;
    if (rot_dim != 0 && (!cos_table || !sin_table)) return true;
    return (!Q != !Q_out) || (!Q && H_q != 0);
}

// The contiguous entry points' own shape rules, behind their NULL pointers.
inline bool rope_ragged_bad_contiguous(int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, int kv_dtype)
{
    if (B <= 0 || H_kv <= 0 || total_q <= 0 || kv_capacity <= 0 || head_dim <= 0 || H_q < 0 || H_q % H_kv) return true;
    // the decode calls' (b, head) slab limit: 2 bytes per element, 1 in an e4m3 cache
    return (long long)kv_capacity * head_dim * (kv_dtype == FA2_DTYPE_FP8_E4M3 ? 1 : 2) > 0x7fffffffLL;
}

// The paged entry points'.
inline bool rope_ragged_bad_paged(int B, int H_q, int H_kv, int total_q, int n_pages, int page_size, int max_pages_per_seq, int head_dim)
{
    if (B <= 0 || H_kv <= 0 || total_q <= 0 || n_pages <= 0 || page_size <= 0 || max_pages_per_seq <= 0 || head_dim <= 0 || H_q < 0 ||
        H_q % H_kv)
        return true;
    if (page_size % kDecodeTile) return true;
    // the paged decode's capacity limit: what this call writes, that call must be able to read
    return (long long)max_pages_per_seq * page_size > 0x7fffffffLL - (kDecodeMaxSplits + 2) * kDecodeKB;
}

// Everything the entry points check after their NULL pointers and their own capacity rules, in the header's order; capacity is
// kv_capacity or max_pages_per_seq x page_size.  The plan comes last, as the ragged extend's does.
inline int rope_ragged_check(const RopeRaggedArgs& a, long long capacity, int head_dim, int rot_dim, int n_positions, int interleaved,
                             int dtype, int kv_dtype, size_t plan_bytes)
{
    if (rot_dim != 0 && (rot_dim < 16 || rot_dim % 16 || rot_dim > head_dim)) return FA2_ERR_INVALID_SHAPE;
    if (rot_dim != 0 && n_positions < capacity) return FA2_ERR_INVALID_SHAPE;
    if (interleaved != 0 && interleaved != 1) return FA2_ERR_INVALID_SHAPE;
    if (((long long)a.Hq + a.Hkv) * a.T > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;      // the units are counted in 32 bits
    if (rope_ragged_bad_stride(a.qt) || rope_ragged_bad_stride(a.qh)) return FA2_ERR_INVALID_SHAPE;
    if (rope_ragged_bad_stride(a.st) || rope_ragged_bad_stride(a.sh)) return FA2_ERR_INVALID_SHAPE;
    if (rope_ragged_misaligned(a.Q) || rope_ragged_misaligned(a.Qout) || rope_ragged_misaligned(a.Knew) || rope_ragged_misaligned(a.Vnew) ||
        rope_ragged_misaligned(a.K) || rope_ragged_misaligned(a.V) || rope_ragged_misaligned(a.cos) || rope_ragged_misaligned(a.sin))
        return FA2_ERR_INVALID_SHAPE;
    if (head_dim != 64 && head_dim != 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    if (dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype != FA2_DTYPE_BF16 && kv_dtype != FA2_DTYPE_FP8_E4M3) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype == FA2_DTYPE_BF16 && (a.k_descale || a.v_descale)) return FA2_ERR_UNSUPPORTED;
    if (plan_bytes < (kRaggedPlanHeader + 2 * (size_t)a.B) * sizeof(int) || rope_ragged_misaligned(a.plan)) return FA2_ERR_WORKSPACE;
    return FA2_OK;
}

}  // namespace

}  // namespace fa2

#endif  // FA2_ROPE_RAGGED_UNIT_H
