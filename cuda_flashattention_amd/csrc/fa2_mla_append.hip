// fa2_mla_append.hip -- the MLA latent-cache append (fa2_mla_kv_append, fa2_mla_kv_append_paged; include/fa2_mla_append_mi355x.h):
// ONE launch writes the n_new newest tokens' rows of the 576-wide latent cache that fa2_mla_decode.hip reads --
// row[:512] = RMSNorm(c_kv; kv_weight, eps), row[512:] = rotate(k_pe, pos) -- and assembles the step's queries
// Q_out [B][H][n_new][576] = (q_nope copied, q_pe rotated), the decode's layout.  The contract is the uniform rotary append's
// (fa2_rope_append.hip): seqlens_k holds the lengths AFTER the append, pos = len - n_new + t, a row is written iff
// 0 <= pos < capacity and (paged) its table entry lies in [0, n_pages), every Q_out row is written (+0.0 for a dropped position).
//
// WORK SPLIT.  No LDS, no barriers, ONE WAVE PER UNIT, four waves per workgroup; the grid is sized from host values only and is
// capped, a wave strides over the units.  The units of a token (b, t) are one cache unit followed by ceil(H / 8) query units;
// b, t and the kind of unit are WAVE-UNIFORM, so seqlens_k[b] and the table entry are scalar loads and the branch between the
// two kinds is a scalar one.  The row width suits a wave: 512 bf16 = 1024 bytes = 64 lanes x 16 bytes.
// CACHE UNIT.  Lane l loads latent columns 8l .. 8l+7 (one coalesced 1 KiB request); lanes 0-7 also load rotary chunk c = l at
// column 512 + 8c and, rotate-half, the partner chunk c ^ 4, with table row pos.  qk_norm_sumsq8 on the latent chunk, then the
// butterfly over ALL 64 lanes: m <= 16 with ds_swizzle as fa2_qk_norm.h does, m = 32 with v_permlane32_swap (the two halves
// of the wave exchanged in registers; fp32 addition commutes, so each lane adds the two results in either order).  It is reached
// by every lane, outside any lane-dependent branch.  r = 1 / sqrt(s / 512 + eps), qk_norm_scale8 with the lane's eight weights
// (two f32x4 loads per wave, kept in registers across its units), one 16-byte store to the row; the eight rotary lanes rotate
// and store at byte 1024 of the row.  The destination is kv_append_offset / kv_append_offset_paged with h = 0, H_kv = 1,
// d = 576; the table entry is read only when pos >= 0, and a dropped row ends the unit before any load.
// QUERY UNIT (b, t, heads 8g .. 8g+7).  The 64 lanes do two jobs.  Copy: for each live head, lane l moves 16 bytes of q_nope
// into Q_out; all loads of the up to eight heads are issued before the first store (32 VGPRs in flight).  Rotation: lane
// 8 hh + c owns chunk c of q_pe of head 8g + hh, so the eight heads' rotary columns are rotated in ONE pass over the wave with
// the token's single cos/sin row, and stored at column 512 of each head's row.  A dropped position stores zeros instead: the
// selection is on pos, uniform per wave, and such a unit loads nothing.
// ADDRESSES.  A table row is read only for a position that passed 0 <= pos < capacity, and the host has checked
// capacity <= n_positions.  A Q_out row is a function of (b, head, t) alone.  No loop bound comes from device memory.
// ARITHMETIC.  fa2_qk_norm.h (steps 1-5 of fa2_rope_norm_mi355x.h at d = 512) and fa2_rope_rotate.h, unchanged: every product
// and sum one fp32 rounding, nothing contracted, one rounding to bf16.
// E4M3 LATENT CACHES (fa2_mla_kv_append_fp8kv / _paged_fp8kv, include/fa2_mla_fp8_mi355x.h): the same kernel at EB = 1.  A row is
// 640 bytes and fa2_kv_append_addr.h counts it in bytes (d = 640).  The cache unit rounds the norm to bf16 exactly as above and
// THEN quantises those eight values with kv_quantise8 (fa2_kv_quantise.h: a correctly rounded division by the cache's one descale,
// read on the device, the clamp to +-448, round to nearest even): 8 bytes a lane at byte 8 lane -- one coalesced 512-byte request --
// and the eight rotary lanes' bf16 at byte 512 + 16 c.  So the latent bytes are the quantisation of the bf16 call's latent columns
// and the rotary bytes are its rotary bytes.  The query units are the ones above.
#include "fa2_common.h"
#include "fa2_kv_append_addr.h"
#include "fa2_kv_quantise.h"
#include "fa2_launch.h"
#include "fa2_mla_append_mi355x.h"
#include "fa2_mla_fp8_mi355x.h"
#include "fa2_qk_norm.h"
#include "fa2_rope_rotate.h"

#include <algorithm>
#include <cmath>

namespace fa2 {

namespace {

constexpr int kMlaAppLatent = 512, kMlaAppRope = 64;      // the one accepted (kv_lora_rank, rope_dim)
constexpr int kMlaAppRow = kMlaAppLatent + kMlaAppRope;   // elements of a cache row and of a Q_out row
constexpr int kMlaAppHalf = kMlaAppRope / 2;              // the tables' row length
constexpr int kMlaAppHeads = 8;                           // heads of a query unit: 8 heads x 8 rotary chunks = 64 lanes
constexpr int kMlaAppMaxBlocks = 2048;                    // 256 CUs x 8 workgroups of 4 waves: a memory-bound grid is capped and strides
// what a wave reads once per unit, at a wave-uniform address: the constant address space makes these scalar loads
typedef __attribute__((address_space(4))) int mla_app_const_int;

struct MlaAppendArgs {
    const void* q_nope; const void* q_pe; void* Qout; const void* kv; void* C;
    const float* cos; const float* sin; const float* w;
    const int* seqlens; const int* block_table;
    float eps;
    int B, H, n_new, Ncap;                       // Ncap: kv_capacity, or max_pages x page_size
    int n_pages, page_size, max_pages;           // paged only
    unsigned upt, units;                         // units of a token: 1 + ceil(H / 8); B x n_new x upt (mla_append_launch)
    long long nb, nh, nt;                        // q_nope's element strides: batch, head, token
    long long pb, ph, pt;                        // q_pe's
    long long kb, kt;                            // kv_new's: batch, token
    const float* descale;                        // e4m3 latent columns: the cache holds y / *descale (DEVICE; NULL: 1)
};

// the value of lane ^ 32 added to the lane's own: v_permlane32_swap exchanges the upper half of its first operand with the
// lower half of its second, so one of the two results is the lane's own value and the other its partner's, in every lane
__device__ __forceinline__ float mla_app_add_xor32(float s)
{
#pragma clang fp contract(off)
    const auto both = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return __uint_as_float(both[0]) + __uint_as_float(both[1]);
}

// steps 3 and 4 of the norm at d = 512: the row is the whole wave.  Every lane of the wave calls this.
__device__ __forceinline__ float mla_app_rstd(float s, float eps)
{
#pragma clang fp contract(off)
    s = s + qk_norm_xor_lane<1>(s);
    s = s + qk_norm_xor_lane<2>(s);
    s = s + qk_norm_xor_lane<4>(s);
    s = s + qk_norm_xor_lane<8>(s);
    s = s + qk_norm_xor_lane<16>(s);
    s = mla_app_add_xor32(s);
    const float mean = s * (1.0f / kMlaAppLatent);      // 1 / 512 is a power of two
    const float v = mean + eps;
    return 1.0f / sqrtf(v);
}

// What a rotary lane holds: its chunk of eight, (rotate-half) its partner's, and its columns of table row pos.
struct MlaAppRot { u32x4 x, xp; f32x4 c0, c1, s0, s1; };

// src: the 64 rotary columns of one row; c: the lane's chunk of them, 0 .. 7; pos: a live position
template <bool INTERLEAVED>
__device__ __forceinline__ MlaAppRot mla_app_rot_load(const __bf16* src, int c, int pos, const float* cos, const float* sin)
{
    MlaAppRot v;
    // the lane's eight table columns (rotate-half: both halves of a pair share column i) or four (interleaved)
    const long long at = (long long)pos * kMlaAppHalf + (INTERLEAVED ? 4 * c : 8 * (c & 3));      // pos < capacity <= n_positions (host-checked)
    v.x = *reinterpret_cast<const u32x4*>(src + 8 * c);
    v.c0 = *reinterpret_cast<const f32x4*>(cos + at);
    v.s0 = *reinterpret_cast<const f32x4*>(sin + at);
    if constexpr (!INTERLEAVED) {
        v.c1 = *reinterpret_cast<const f32x4*>(cos + at + 4);
        v.s1 = *reinterpret_cast<const f32x4*>(sin + at + 4);
        v.xp = *reinterpret_cast<const u32x4*>(src + 8 * (c ^ 4));      // a SECOND 16-byte load, as fa2_rope_append.hip does
    }
    return v;
}

template <bool INTERLEAVED>
__device__ __forceinline__ u32x4 mla_app_rot(const MlaAppRot& v, int c)
{
    if constexpr (INTERLEAVED) {
        return rope_rotate_pairs8(v.x, v.c0, v.s0);
    } else {
        const uint32_t sign = c < 4 ? 0x80008000u : 0u;      // x1*c - x2*s as x1*c + (-x2)*s
        const u32x4 q = u32x4{v.xp[0] ^ sign, v.xp[1] ^ sign, v.xp[2] ^ sign, v.xp[3] ^ sign};
        return rope_rotate_half8(v.x, q, v.c0, v.c1, v.s0, v.s1);
    }
}

// EB: bytes per latent element of the cache row, 2 (bf16, everything above) or 1 (fa2_mla_kv_append_fp8kv / _paged_fp8kv).
template <bool PAGED, bool INTERLEAVED, int EB = 2>
__global__ __launch_bounds__(256) void fa2_mla_append_kernel(const MlaAppendArgs a)
{
    static_assert(EB == 1 || EB == 2, "bf16 or e4m3 latent columns");
    constexpr int ROWB = EB * kMlaAppLatent + 2 * kMlaAppRope;      // bytes of a cache row: 1152 or 640
    // the cache's descale, once per wave: a scalar load on the device, so that a captured graph sees the value of its replay
    float ds = 1.0f;
    if constexpr (EB == 1)
        if (a.descale) ds = __uint_as_float(__builtin_amdgcn_readfirstlane(*(const mla_app_const_int*)a.descale));
    const int lane = threadIdx.x & 63;
    const int c = lane & 7, hh = lane >> 3;      // a rotary lane's chunk; a query unit's head of that lane
    // the lane's eight weights, once per wave
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(a.w + 8 * lane);
    const f32x4 w1 = *reinterpret_cast<const f32x4*>(a.w + 8 * lane + 4);
    // host values: B x (H + 1) x n_new is below 2^31 (mla_append_check) and the grid is capped, so u + step stays below 2^32
    const unsigned upt = a.upt, units = a.units;
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned step = gridDim.x * 4u;
    for (unsigned u = wave; u < units; u += step) {
        const int k = (int)(u % upt), bt = (int)(u / upt);
        const int t = bt % a.n_new, b = bt / a.n_new;
        const int len = ((const mla_app_const_int*)a.seqlens)[b];
        const int pos = kv_append_pos(len, a.n_new, t, a.Ncap);      // wave-uniform
        if (k == 0) {
            // ---- the cache unit
            long long to = kKvAppendDropped;
            if constexpr (PAGED) {
                if (pos >= 0) {
                    const int entry = ((const mla_app_const_int*)a.block_table)[(long long)b * a.max_pages + kv_append_table_index(pos, a.page_size)];
                    to = kv_append_offset_paged(pos, entry, a.n_pages, 0, 1, a.page_size, EB == 2 ? kMlaAppRow : ROWB);
                }
            } else {
                to = kv_append_offset(pos, b, 0, 1, a.Ncap, EB == 2 ? kMlaAppRow : ROWB);      // dropped for pos = -1; EB = 1: in bytes
            }
            if (to < 0) continue;      // wave-uniform: the whole wave leaves together
            const __bf16* src = (const __bf16*)a.kv + (long long)b * a.kb + (long long)t * a.kt;
            const u32x4 x = *reinterpret_cast<const u32x4*>(src + 8 * lane);
            MlaAppRot rot;
            if (lane < 8) rot = mla_app_rot_load<INTERLEAVED>(src + kMlaAppLatent, c, pos, a.cos, a.sin);
            const float r = mla_app_rstd(qk_norm_sumsq8(x), a.eps);      // every lane
            if constexpr (EB == 2) {
            __bf16* row = (__bf16*)a.C + to;
            *reinterpret_cast<u32x4*>(row + 8 * lane) = qk_norm_scale8(x, r, w0, w1);
            if (lane < 8) *reinterpret_cast<u32x4*>(row + kMlaAppLatent + 8 * c) = mla_app_rot<INTERLEAVED>(rot, c);
            } else {
                // the bf16 append's eight values, THEN their codes: 8 bytes a lane at byte 8 lane; the rotary bf16 behind byte 512
                char* row = (char*)a.C + to;
                *reinterpret_cast<u32x2*>(row + 8 * lane) = kv_quantise8(qk_norm_scale8(x, r, w0, w1), ds);
                if (lane < 8) *reinterpret_cast<u32x4*>(row + kMlaAppLatent + 16 * c) = mla_app_rot<INTERLEAVED>(rot, c);
            }
        } else {
            // ---- a query unit: heads h0 .. h0 + n - 1 of token (b, t)
            const int h0 = (k - 1) * kMlaAppHeads;
            const int n = min(kMlaAppHeads, a.H - h0);
            const bool live = pos >= 0;          // wave-uniform
            const bool mine = hh < n;            // this lane's head exists
            const u32x4 zero = u32x4{0u, 0u, 0u, 0u};      // a row whose position has no table row: +0.0 throughout
            u32x4 x[kMlaAppHeads];
#pragma unroll
            for (int i = 0; i < kMlaAppHeads; ++i) x[i] = zero;
            MlaAppRot rot;
            if (live) {
                const __bf16* nope = (const __bf16*)a.q_nope + (long long)b * a.nb + (long long)h0 * a.nh + (long long)t * a.nt + 8 * lane;
#pragma unroll
                for (int i = 0; i < kMlaAppHeads; ++i)
                    if (i < n) x[i] = *reinterpret_cast<const u32x4*>(nope + (long long)i * a.nh);
                if (mine)
                    rot = mla_app_rot_load<INTERLEAVED>((const __bf16*)a.q_pe + (long long)b * a.pb + (long long)(h0 + hh) * a.ph + (long long)t * a.pt,
                                                        c, pos, a.cos, a.sin);
            }
            // every row of Q_out is written: row (b, head, t), a function of host values and the unit alone
            __bf16* out = (__bf16*)a.Qout + (((long long)b * a.H + h0) * a.n_new + t) * kMlaAppRow;
            const long long hstride = (long long)a.n_new * kMlaAppRow;
#pragma unroll
            for (int i = 0; i < kMlaAppHeads; ++i)
                if (i < n) *reinterpret_cast<u32x4*>(out + i * hstride + 8 * lane) = x[i];
            if (mine) {
                u32x4 y = zero;
                if (live) y = mla_app_rot<INTERLEAVED>(rot, c);
                *reinterpret_cast<u32x4*>(out + hh * hstride + kMlaAppLatent + 8 * c) = y;
            }
        }
    }
}

template <bool PAGED, bool INTERLEAVED, int EB>
hipError_t mla_append_launch(MlaAppendArgs a, hipStream_t stream)
{
    a.upt = 1u + (unsigned)((a.H + kMlaAppHeads - 1) / kMlaAppHeads);
    const long long units = (long long)a.B * a.n_new * a.upt;      // <= B x (H + 1) x n_new
    a.units = (unsigned)units;
    const unsigned grid = (unsigned)std::min<long long>((units + 3) / 4, kMlaAppMaxBlocks);
    hipLaunchKernelGGL((fa2_mla_append_kernel<PAGED, INTERLEAVED, EB>), dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

inline bool mla_append_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

inline bool mla_append_bad_stride(long long s) { return s < 0 || s % 8 != 0; }

// The pointers of both entry points: q_nope, q_pe and Q_out come as a triple, and only a call without heads may leave them out.
inline bool mla_append_null(const void* q_nope, const void* q_pe, const void* Q_out, int H, const void* kv_new, const void* cache,
                            const float* cos_table, const float* sin_table, const float* kv_weight, const int* seqlens_k)
{
    if (!kv_new || !cache || !cos_table || !sin_table || !kv_weight || !seqlens_k) return true;
    const int given = (q_nope != nullptr) + (q_pe != nullptr) + (Q_out != nullptr);
    return (given != 0 && given != 3) || (given == 0 && H != 0);
}

// Everything both entry points check after their NULL pointers and their own capacity rules, in the header's order, then the
// launch; capacity is kv_capacity or max_pages_per_seq x page_size.
template <bool PAGED, int EB = 2>
int mla_append_run(const MlaAppendArgs& a, int kv_lora_rank, int rope_dim, int n_positions, int interleaved, hipStream_t stream)
{
    if ((long long)a.B * ((long long)a.H + 1) > 0x7fffffffLL || (long long)a.B * ((long long)a.H + 1) * a.n_new > 0x7fffffffLL)
        return FA2_ERR_INVALID_SHAPE;                                                      // the units are counted in 32 bits
    if (!std::isfinite(a.eps) || !(a.eps > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    if (interleaved != 0 && interleaved != 1) return FA2_ERR_INVALID_SHAPE;
    if (n_positions < a.Ncap) return FA2_ERR_INVALID_SHAPE;
    if (mla_append_bad_stride(a.nb) || mla_append_bad_stride(a.nh) || mla_append_bad_stride(a.nt)) return FA2_ERR_INVALID_SHAPE;
    if (mla_append_bad_stride(a.pb) || mla_append_bad_stride(a.ph) || mla_append_bad_stride(a.pt)) return FA2_ERR_INVALID_SHAPE;
    if (mla_append_bad_stride(a.kb) || mla_append_bad_stride(a.kt)) return FA2_ERR_INVALID_SHAPE;
    if (mla_append_misaligned(a.q_nope) || mla_append_misaligned(a.q_pe) || mla_append_misaligned(a.Qout) || mla_append_misaligned(a.kv) ||
        mla_append_misaligned(a.C) || mla_append_misaligned(a.cos) || mla_append_misaligned(a.sin) || mla_append_misaligned(a.w))
        return FA2_ERR_INVALID_SHAPE;
    if (kv_lora_rank != kMlaAppLatent || rope_dim != kMlaAppRope) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    const hipError_t e = interleaved ? mla_append_launch<PAGED, true, EB>(a, stream) : mla_append_launch<PAGED, false, EB>(a, stream);
    return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e;
}

}  // namespace

}  // namespace fa2

namespace fa2 {

namespace {

struct MlaAppendStrides { long long nb, nh, nt, pb, ph, pt, kb, kt; };

// fa2_mla_kv_append and its e4m3 form: the checks of the contiguous call, then mla_append_run
template <int EB>
int mla_append_contiguous(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_cache, const float* cos_table,
                          const float* sin_table, const float* kv_weight, float eps, const float* descale, const int* seqlens_k, int B,
                          int H, int n_new, int kv_capacity, int kv_lora_rank, int rope_dim, int n_positions, int interleaved,
                          const MlaAppendStrides& s, void* stream)
{
    if (mla_append_null(q_nope, q_pe, Q_out, H, kv_new, ckv_cache, cos_table, sin_table, kv_weight, seqlens_k)) return FA2_ERR_NULL_POINTER;
    if (B <= 0 || n_new <= 0 || kv_capacity <= 0 || H < 0) return FA2_ERR_INVALID_SHAPE;
    // the MLA decode's limit: one sequence, one buffer resource of 1152-byte (e4m3: 640-byte) rows
    if ((long long)kv_capacity * (EB * kMlaAppLatent + 2 * kMlaAppRope) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    MlaAppendArgs a{};
    a.q_nope = q_nope; a.q_pe = q_pe; a.Qout = Q_out; a.kv = kv_new; a.C = ckv_cache; a.cos = cos_table; a.sin = sin_table;
    a.w = kv_weight; a.eps = eps; a.seqlens = seqlens_k; a.descale = descale;
    a.B = B; a.H = Q_out ? H : 0; a.n_new = n_new; a.Ncap = kv_capacity;
    a.nb = s.nb; a.nh = s.nh; a.nt = s.nt; a.pb = s.pb; a.ph = s.ph; a.pt = s.pt; a.kb = s.kb; a.kt = s.kt;
    return mla_append_run<false, EB>(a, kv_lora_rank, rope_dim, n_positions, interleaved, (hipStream_t)stream);
}

template <int EB>
int mla_append_paged(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_pages, const int* block_table,
                     const float* cos_table, const float* sin_table, const float* kv_weight, float eps, const float* descale,
                     const int* seqlens_k, int B, int H, int n_new, int n_pages, int page_size, int max_pages_per_seq, int kv_lora_rank,
                     int rope_dim, int n_positions, int interleaved, const MlaAppendStrides& s, void* stream)
{
    if (mla_append_null(q_nope, q_pe, Q_out, H, kv_new, ckv_pages, cos_table, sin_table, kv_weight, seqlens_k) || !block_table)
        return FA2_ERR_NULL_POINTER;
    if (B <= 0 || n_new <= 0 || n_pages <= 0 || page_size <= 0 || max_pages_per_seq <= 0 || H < 0) return FA2_ERR_INVALID_SHAPE;
    if (page_size % kDecodeTile) return FA2_ERR_INVALID_SHAPE;
    // the paged MLA decode's capacity limit: what this call writes, that call must be able to read
    if ((long long)max_pages_per_seq * page_size > 0x7fffffffLL - (kDecodeMaxSplits + 2) * kDecodeKB) return FA2_ERR_INVALID_SHAPE;
    MlaAppendArgs a{};
    a.q_nope = q_nope; a.q_pe = q_pe; a.Qout = Q_out; a.kv = kv_new; a.C = ckv_pages; a.cos = cos_table; a.sin = sin_table;
    a.w = kv_weight; a.eps = eps; a.seqlens = seqlens_k; a.block_table = block_table; a.descale = descale;
    a.B = B; a.H = Q_out ? H : 0; a.n_new = n_new; a.Ncap = max_pages_per_seq * page_size;
    a.n_pages = n_pages; a.page_size = page_size; a.max_pages = max_pages_per_seq;
    a.nb = s.nb; a.nh = s.nh; a.nt = s.nt; a.pb = s.pb; a.ph = s.ph; a.pt = s.pt; a.kb = s.kb; a.kt = s.kt;
    return mla_append_run<true, EB>(a, kv_lora_rank, rope_dim, n_positions, interleaved, (hipStream_t)stream);
}

}  // namespace

}  // namespace fa2

extern "C" {

int fa2_mla_kv_append(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_cache,
                      const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                      const int* seqlens_k,
                      int B, int H, int n_new, int kv_capacity, int kv_lora_rank, int rope_dim,
                      int n_positions, int interleaved,
                      long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                      long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                      long long kv_stride_b, long long kv_stride_t, void* stream)
{
    return fa2::mla_append_contiguous<2>(q_nope, q_pe, Q_out, kv_new, ckv_cache, cos_table, sin_table, kv_weight, eps, nullptr, seqlens_k, B, H,
                                         n_new, kv_capacity, kv_lora_rank, rope_dim, n_positions, interleaved,
                                         {q_nope_stride_b, q_nope_stride_h, q_nope_stride_t, q_pe_stride_b, q_pe_stride_h, q_pe_stride_t,
                                          kv_stride_b, kv_stride_t}, stream);
}

int fa2_mla_kv_append_paged(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_pages,
                            const int* block_table,
                            const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                            const int* seqlens_k,
                            int B, int H, int n_new, int n_pages, int page_size, int max_pages_per_seq,
                            int kv_lora_rank, int rope_dim,
                            int n_positions, int interleaved,
                            long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                            long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                            long long kv_stride_b, long long kv_stride_t, void* stream)
{
    return fa2::mla_append_paged<2>(q_nope, q_pe, Q_out, kv_new, ckv_pages, block_table, cos_table, sin_table, kv_weight, eps, nullptr,
                                    seqlens_k, B, H, n_new, n_pages, page_size, max_pages_per_seq, kv_lora_rank, rope_dim, n_positions,
                                    interleaved,
                                    {q_nope_stride_b, q_nope_stride_h, q_nope_stride_t, q_pe_stride_b, q_pe_stride_h, q_pe_stride_t,
                                     kv_stride_b, kv_stride_t}, stream);
}

int fa2_mla_kv_append_fp8kv(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_cache,
                            const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                            const float* latent_descale, const int* seqlens_k,
                            int B, int H, int n_new, int kv_capacity, int kv_lora_rank, int rope_dim,
                            int n_positions, int interleaved,
                            long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                            long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                            long long kv_stride_b, long long kv_stride_t, void* stream)
{
    return fa2::mla_append_contiguous<1>(q_nope, q_pe, Q_out, kv_new, ckv_cache, cos_table, sin_table, kv_weight, eps, latent_descale,
                                         seqlens_k, B, H, n_new, kv_capacity, kv_lora_rank, rope_dim, n_positions, interleaved,
                                         {q_nope_stride_b, q_nope_stride_h, q_nope_stride_t, q_pe_stride_b, q_pe_stride_h, q_pe_stride_t,
                                          kv_stride_b, kv_stride_t}, stream);
}

int fa2_mla_kv_append_paged_fp8kv(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_pages,
                                  const int* block_table,
                                  const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                                  const float* latent_descale, const int* seqlens_k,
                                  int B, int H, int n_new, int n_pages, int page_size, int max_pages_per_seq,
                                  int kv_lora_rank, int rope_dim,
                                  int n_positions, int interleaved,
                                  long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                                  long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                                  long long kv_stride_b, long long kv_stride_t, void* stream)
{
    return fa2::mla_append_paged<1>(q_nope, q_pe, Q_out, kv_new, ckv_pages, block_table, cos_table, sin_table, kv_weight, eps,
                                    latent_descale, seqlens_k, B, H, n_new, n_pages, page_size, max_pages_per_seq, kv_lora_rank, rope_dim,
                                    n_positions, interleaved,
                                    {q_nope_stride_b, q_nope_stride_h, q_nope_stride_t, q_pe_stride_b, q_pe_stride_h, q_pe_stride_t,
                                     kv_stride_b, kv_stride_t}, stream);
}

}  // extern "C"
