// fa2_rope_append.hip -- the rotary-embedding KV-cache append (fa2_rope_kv_append, fa2_rope_kv_append_paged;
// include/fa2_rope_mi355x.h): ONE launch rotates the n_new newest tokens' K and writes it into the cache, copies their V into
// the cache, and writes the step's rotated queries as [B][H_q][n_new][d], the decode's layout.  It is the append of
// fa2_kv_append.hip with a rotation in front of the K store and H_q more heads.
//
// WORK SPLIT.  The append's, over H_kv + H_q heads: a row of d elements is d / 8 lanes of 16 bytes, a wave holds 64 / (d / 8)
// rows per pass and makes kRopePasses passes per unit.  A unit is (sequence b, head j, a group of tokens); j < H_kv is a K/V head
// (rotate and store K, store V), the others are Q heads (rotate into Q_out).  b and j are WAVE-UNIFORM: the branch between the
// two kinds of head is a scalar one, and seqlens_k[b] and the descales are scalar loads.  The grid depends on host values only
// and is capped; a wave strides over the rest.  Plain compiler code: no LDS, no atomics, no inline assembly, no communication
// between workgroups; every byte written is a function of the inputs alone.
// ADDRESSES.  A cache destination is formed by fa2_kv_append_addr.h and nothing else, exactly as the append forms it.  A table
// row is read only for a position that passed 0 <= pos < capacity, and the host has checked capacity <= n_positions.  A Q_out
// row is a function of (b, head, t) alone, t < n_new.  No loop bound comes from device memory.
// ROTATION.  fa2_rope_rotate.h, shared with the ragged call (fa2_rope_append_ragged.hip): each product and each sum is one fp32
// rounding.  The partner of a rotate-half lane's chunk is the whole chunk of lane c +- rot_dim / 16, fetched with a SECOND
// 16-byte load; an interleaved lane holds its four pairs itself.
#include "fa2_common.h"
#include "fa2_kv_append_addr.h"
#include "fa2_kv_quantise.h"
#include "fa2_launch.h"
#include "fa2_rope_mi355x.h"
#include "fa2_rope_rotate.h"

#include <algorithm>

namespace fa2 {

namespace {

constexpr int kRopePasses = 2;           // rows of a lane per unit: both passes' loads are issued before the first store
constexpr int kRopeMaxBlocks = 2048;     // 256 CUs x 8 workgroups of 4 waves: a memory-bound grid is capped and strides
// what a wave reads once per unit, at a wave-uniform address: the constant address space makes these scalar loads
typedef __attribute__((address_space(4))) int rope_const_int;
typedef __attribute__((address_space(4))) float rope_const_float;

struct RopeAppendArgs {
    const void* Q; void* Qout; const void* Knew; const void* Vnew; void* K; void* V;
    const float* cos; const float* sin;
    const int* seqlens; const int* block_table; const float* k_descale; const float* v_descale;
    int B, Hq, Hkv, n_new, Ncap;                 // Ncap: kv_capacity, or max_pages x page_size
    int n_pages, page_size, max_pages;           // paged only
    int half;                                    // rot_dim / 2: the tables' row length, a multiple of 8
    unsigned groups, units;                      // token groups of a (sequence, head); B x (H_kv + H_q) x groups (rope_append_launch)
    long long qb, qh, qt;                        // Q's element strides: batch, head, token
    long long sb, sh, st;                        // K_new's and V_new's
};

template <int D, bool FP8, bool PAGED, bool INTERLEAVED>
__global__ __launch_bounds__(256) void fa2_rope_append_kernel(const RopeAppendArgs a)
{
    constexpr int LPR = D / 8;                  // lanes of a row
    constexpr int ROWS = 64 / LPR;              // rows of a wave's pass
    constexpr int TPU = ROWS * kRopePasses;     // tokens of a unit
    const int lane = threadIdx.x & 63;
    const int r = lane / LPR, c = lane % LPR;
    const int heads = a.Hkv + a.Hq;
    const bool rotates = 4 * c < a.half;        // this lane's chunk lies inside rot_dim (8 c < rot_dim)
    const bool first = 8 * c < a.half;          // rotate-half: inside the first half, the x1 of its pairs
    // the lane's eight table columns (rotate-half) or four (interleaved), and its partner's chunk
    const int col = INTERLEAVED ? 4 * c : (first ? 8 * c : 8 * c - a.half);
    const int partner = first ? a.half : -a.half;
    // host values: B x heads x n_new is below 2^31 (rope_check) and the grid is capped, so u + step stays below 2^32
    const unsigned groups = a.groups, units = a.units;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned step = gridDim.x * 4u;
    for (unsigned u = wave; u < units; u += step) {
        const int g = (int)(u % groups), bj = (int)(u / groups);
        const int j = bj % heads, b = bj / heads;
        const bool is_q = j >= a.Hkv;                                                // wave-uniform
        const int h = is_q ? j - a.Hkv : j;
        const int len = ((const rope_const_int*)a.seqlens)[b];
        float kd = 1.0f, vd = 1.0f;
        if constexpr (FP8) {
            if (!is_q) {
                if (a.k_descale) kd = ((const rope_const_float*)a.k_descale)[h];
                if (a.v_descale) vd = ((const rope_const_float*)a.v_descale)[h];
            }
        }
        const __bf16* xsrc = (const __bf16*)(is_q ? a.Q : a.Knew);
        const long long row0 = is_q ? (long long)b * a.qb + (long long)h * a.qh : (long long)b * a.sb + (long long)h * a.sh;
        const long long tstride = is_q ? a.qt : a.st;
        long long dst[kRopePasses];               // where the row goes (a cache, or Q_out), or dropped
        bool live[kRopePasses];                   // its position has a table row: it was loaded and is rotated
        u32x4 x[kRopePasses], xp[kRopePasses], v[kRopePasses];
        f32x4 c0[kRopePasses], c1[kRopePasses], s0[kRopePasses], s1[kRopePasses];
#pragma unroll
        for (int p = 0; p < kRopePasses; ++p) {
            const unsigned t = (unsigned)g * TPU + p * ROWS + r;      // unsigned: the last group may pass n_new, up to INT_MAX, by TPU - 1
            const bool in = t < (unsigned)a.n_new;
            const int pos = in ? kv_append_pos(len, a.n_new, (int)t, a.Ncap) : -1;
            long long to = kKvAppendDropped;
            if (is_q) {
                if (in) to = (((long long)b * a.Hq + h) * a.n_new + t) * D;      // every row of Q_out is written
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
#pragma unroll
        for (int p = 0; p < kRopePasses; ++p) {
            if (dst[p] < 0) continue;
            u32x4 y = u32x4{0u, 0u, 0u, 0u};      // a Q row whose position has no table row: +0.0 throughout
            if (live[p]) {
                y = x[p];                          // past rot_dim: the source bits
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

template <int D, bool FP8, bool PAGED, bool INTERLEAVED>
hipError_t rope_append_launch(RopeAppendArgs a, hipStream_t stream)
{
    constexpr int TPU = 64 / (D / 8) * kRopePasses;
    a.groups = (unsigned)(((long long)a.n_new + TPU - 1) / TPU);
    const long long units = (long long)a.B * (a.Hkv + a.Hq) * a.groups;
    a.units = (unsigned)units;
    const unsigned grid = (unsigned)std::min<long long>((units + 3) / 4, kRopeMaxBlocks);
    hipLaunchKernelGGL((fa2_rope_append_kernel<D, FP8, PAGED, INTERLEAVED>), dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <int D, bool PAGED>
hipError_t rope_append_pick(const RopeAppendArgs& a, bool fp8, bool interleaved, hipStream_t stream)
{
    if (fp8) return interleaved ? rope_append_launch<D, true, PAGED, true>(a, stream) : rope_append_launch<D, true, PAGED, false>(a, stream);
    return interleaved ? rope_append_launch<D, false, PAGED, true>(a, stream) : rope_append_launch<D, false, PAGED, false>(a, stream);
}

template <bool PAGED>
hipError_t rope_append_dispatch(const RopeAppendArgs& a, int d, bool fp8, bool interleaved, hipStream_t stream)
{
    if (d == 128) return rope_append_pick<128, PAGED>(a, fp8, interleaved, stream);
    if (d == 64) return rope_append_pick<64, PAGED>(a, fp8, interleaved, stream);
    return hipErrorInvalidValue;
}

inline int rope_hip_status(hipError_t e) { return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e; }

inline bool rope_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

inline bool rope_bad_stride(long long s) { return s < 0 || s % 8 != 0; }

// Everything both entry points check after their NULL pointers and their own capacity rules, in the header's order; capacity is
// kv_capacity or max_pages_per_seq x page_size.
int rope_check(const RopeAppendArgs& a, long long capacity, int head_dim, int rot_dim, int n_positions, int interleaved, int dtype,
               int kv_dtype)
{
    if (rot_dim < 16 || rot_dim % 16 || rot_dim > head_dim) return FA2_ERR_INVALID_SHAPE;
    if (n_positions < capacity) return FA2_ERR_INVALID_SHAPE;
    if (interleaved != 0 && interleaved != 1) return FA2_ERR_INVALID_SHAPE;
    const long long heads = (long long)a.B * ((long long)a.Hq + a.Hkv);                     // the units are counted in 32 bits
    if (heads > 0x7fffffffLL || heads * a.n_new > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    if (rope_bad_stride(a.qb) || rope_bad_stride(a.qh) || rope_bad_stride(a.qt)) return FA2_ERR_INVALID_SHAPE;
    if (rope_bad_stride(a.sb) || rope_bad_stride(a.sh) || rope_bad_stride(a.st)) return FA2_ERR_INVALID_SHAPE;
    if (rope_misaligned(a.Q) || rope_misaligned(a.Qout) || rope_misaligned(a.Knew) || rope_misaligned(a.Vnew) || rope_misaligned(a.K) ||
        rope_misaligned(a.V) || rope_misaligned(a.cos) || rope_misaligned(a.sin))
        return FA2_ERR_INVALID_SHAPE;
    if (head_dim != 64 && head_dim != 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    if (dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype != FA2_DTYPE_BF16 && kv_dtype != FA2_DTYPE_FP8_E4M3) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype == FA2_DTYPE_BF16 && (a.k_descale || a.v_descale)) return FA2_ERR_UNSUPPORTED;
    return FA2_OK;
}

// The pointers of both entry points: Q and Q_out come as a pair, and only a call without Q heads may leave them out.
inline bool rope_null(const void* Q, const void* Q_out, int H_q, const void* K_new, const void* V_new, const void* K, const void* V,
                      const float* cos_table, const float* sin_table, const int* seqlens_k)
{
    if (!K_new || !V_new || !K || !V || !cos_table || !sin_table || !seqlens_k) return true;
    return (!Q != !Q_out) || (!Q && H_q != 0);
}

}  // namespace

}  // namespace fa2

extern "C" {

int fa2_rope_kv_append(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                       const float* cos_table, const float* sin_table, const int* seqlens_k,
                       const float* k_descale, const float* v_descale,
                       int B, int H_q, int H_kv, int n_new, int kv_capacity, int head_dim,
                       int rot_dim, int n_positions, int interleaved,
                       long long q_stride_b, long long q_stride_h, long long q_stride_t,
                       long long new_stride_b, long long new_stride_h, long long new_stride_t,
                       int dtype, int kv_dtype, void* stream)
{
    if (fa2::rope_null(Q, Q_out, H_q, K_new, V_new, K_cache, V_cache, cos_table, sin_table, seqlens_k)) return FA2_ERR_NULL_POINTER;
    if (B <= 0 || H_kv <= 0 || n_new <= 0 || kv_capacity <= 0 || head_dim <= 0 || H_q < 0) return FA2_ERR_INVALID_SHAPE;
    // the decode calls' (b, head) slab limit: 2 bytes per element, 1 in an e4m3 cache
    if ((long long)kv_capacity * head_dim * (kv_dtype == FA2_DTYPE_FP8_E4M3 ? 1 : 2) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    fa2::RopeAppendArgs a{};
    a.Q = Q; a.Qout = Q_out; a.Knew = K_new; a.Vnew = V_new; a.K = K_cache; a.V = V_cache; a.cos = cos_table; a.sin = sin_table;
    a.seqlens = seqlens_k; a.k_descale = k_descale; a.v_descale = v_descale;
    a.B = B; a.Hq = Q ? H_q : 0; a.Hkv = H_kv; a.n_new = n_new; a.Ncap = kv_capacity; a.half = rot_dim / 2;
    a.qb = q_stride_b; a.qh = q_stride_h; a.qt = q_stride_t;
    a.sb = new_stride_b; a.sh = new_stride_h; a.st = new_stride_t;
    if (const int st = fa2::rope_check(a, kv_capacity, head_dim, rot_dim, n_positions, interleaved, dtype, kv_dtype)) return st;
    return fa2::rope_hip_status(fa2::rope_append_dispatch<false>(a, head_dim, kv_dtype == FA2_DTYPE_FP8_E4M3, interleaved != 0,
                                                                 (hipStream_t)stream));
}

int fa2_rope_kv_append_paged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                             const int* block_table, const float* cos_table, const float* sin_table, const int* seqlens_k,
                             const float* k_descale, const float* v_descale,
                             int B, int H_q, int H_kv, int n_new, int n_pages, int page_size,
                             int max_pages_per_seq, int head_dim,
                             int rot_dim, int n_positions, int interleaved,
                             long long q_stride_b, long long q_stride_h, long long q_stride_t,
                             long long new_stride_b, long long new_stride_h, long long new_stride_t,
                             int dtype, int kv_dtype, void* stream)
{
    if (fa2::rope_null(Q, Q_out, H_q, K_new, V_new, K_pages, V_pages, cos_table, sin_table, seqlens_k) || !block_table)
        return FA2_ERR_NULL_POINTER;
    if (B <= 0 || H_kv <= 0 || n_new <= 0 || n_pages <= 0 || page_size <= 0 || max_pages_per_seq <= 0 || head_dim <= 0 || H_q < 0)
        return FA2_ERR_INVALID_SHAPE;
    if (page_size % fa2::kDecodeTile) return FA2_ERR_INVALID_SHAPE;
    // the paged decode's capacity limit: what this call writes, that call must be able to read
    if ((long long)max_pages_per_seq * page_size > 0x7fffffffLL - (fa2::kDecodeMaxSplits + 2) * fa2::kDecodeKB) return FA2_ERR_INVALID_SHAPE;
    fa2::RopeAppendArgs a{};
    a.Q = Q; a.Qout = Q_out; a.Knew = K_new; a.Vnew = V_new; a.K = K_pages; a.V = V_pages; a.cos = cos_table; a.sin = sin_table;
    a.seqlens = seqlens_k; a.block_table = block_table; a.k_descale = k_descale; a.v_descale = v_descale;
    a.B = B; a.Hq = Q ? H_q : 0; a.Hkv = H_kv; a.n_new = n_new; a.Ncap = max_pages_per_seq * page_size; a.half = rot_dim / 2;
    a.n_pages = n_pages; a.page_size = page_size; a.max_pages = max_pages_per_seq;
    a.qb = q_stride_b; a.qh = q_stride_h; a.qt = q_stride_t;
    a.sb = new_stride_b; a.sh = new_stride_h; a.st = new_stride_t;
    if (const int st = fa2::rope_check(a, a.Ncap, head_dim, rot_dim, n_positions, interleaved, dtype, kv_dtype)) return st;
    return fa2::rope_hip_status(fa2::rope_append_dispatch<true>(a, head_dim, kv_dtype == FA2_DTYPE_FP8_E4M3, interleaved != 0,
                                                                (hipStream_t)stream));
}

}  // extern "C"
