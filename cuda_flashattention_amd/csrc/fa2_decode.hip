// fa2_decode.hip -- split-KV decode attention over a KV cache with per-sequence lengths (fa2_forward_decode,
// include/fa2_mi355x.h): a few new query tokens per sequence (N_q) against [B][H_kv][N_cap][d] caches of which sequence b uses
// the first len_b = clamp(seqlens_k[b], 0, N_cap) rows.
//
// WORK SPLIT.  One workgroup = one (sequence, K/V head, key split).  The M = G N_q query rows of the head's group (G = H_q / H_kv;
// they are one contiguous [M][d] slab of Q, O and L) are the 32 COLUMNS of an MFMA tile, so the K/V head is streamed once for
// the whole group.  Split s covers keys [s chunk, min((s + 1) chunk, len_b)), chunk = roundup(ceil(len_b / n_splits), kDecodeKB),
// computed here from len_b: the host never sees a length.  Inside the split the four waves take the 32-key tiles round-robin
// (wave w: tiles w, w + 4, ...), each with an online softmax of its own; they meet once, through LDS, at the end.
// DATA PATH per 32-key tile of a wave:
//   S^T = K Q^T   A = K: lane (key r, half h) holds 16 contiguous bytes of its key row per k-step, loaded straight from global
//                 memory into VGPRs (every K byte is used once: no LDS round trip); B = Q^T, loaded once, rows >= M zero;
//   softmax       a score's query row is the LANE, its 16 keys the registers: maximum and sum are in-lane plus one
//                 permlane32_swap; masked probabilities are SELECTED to 0; the row sum adds the fp32 P;
//   O^T += V^T P^T  P^T is the accumulator itself (bf16-rounded) as the B operand; V^T comes from V rows loaded in whole lines
//                 into VGPRs, written into the wave's own swizzled LDS image (lds_off) and read back with ds_read_b64_tr_b16.
//                 A wave's LDS operations execute in order, so its private image needs no barrier.
// K and V are read through buffer resources that end at the split's last key: rows past it (whatever a cache holds beyond
// its length, NaNs included) come back as zeros and never meet an MFMA as data.  The next tile's K and V loads are issued before
// the current tile's arithmetic.
// RESULT.  n_splits == 1: O (bf16, the sink applied) and L.  Otherwise an fp32 partial per (split, row): the normalised O_s [d]
// and L_s (-inf for a split without a visible key), which fa2_decode_combine_kernel -- a second plain launch on the same
// stream -- folds in ascending s: L = logsumexp_s L_s, O = sum_s exp(L_s - L) O_s, then the sink, then ONE rounding to bf16.
// No workgroup talks to another inside a launch: no atomics, no flags, no waiting; every sum has a fixed order.
// PAGED (fa2_forward_decode_paged): the same body over a pool of pages and a block table, see decode_split_body.
// FP8 CACHES (fa2_forward_decode_fp8kv, _paged_fp8kv): the same body over e4m3 K and V with a descale per K/V head, see there.
// SLIDING WINDOW (fa2_forward_decode_window, _paged_window): the same body with a lower bound on the key range, see there.
// EXTEND (fa2_forward_extend, _paged; include/fa2_extend_mi355x.h): more than 32 rows per K/V head, see extend_split_body.
#include "fa2_common.h"
#include "fa2_launch.h"

#include <algorithm>
#include <type_traits>

namespace fa2 {

namespace {

constexpr float kDecLn2 = 0.6931471805599453f;
constexpr int kDecWaves = kDecodeKB / kDecodeTile;      // 4: one tile per wave and round
typedef __attribute__((address_space(3))) bf16x4 dec_lds_bf16x4;
typedef __attribute__((address_space(4))) int dec_const_int;
constexpr int kCombineBatch = 8;      // partials of a row in flight in the combine

// L <- log(exp L + exp s), returns exp(L_old - L_new), what O scales by (fa2_forward_sink's rule).  s = -inf: no sink, nothing
// changes, bit for bit.  L = -inf (a row without a key): L = s and O = 0.
__device__ __forceinline__ float decode_sink(float s, float& L)
{
    const bool none = s == -INFINITY, keyless = L == -INFINITY;
    const float hi = fmaxf(L, s);
    const float e = __builtin_amdgcn_exp2f(-fabsf(L - s) * kLog2e);             // (NaN where both are -inf: selected away)
    const float Ln = hi + __builtin_amdgcn_logf(1.0f + e) * kDecLn2;
    const float w = __builtin_amdgcn_exp2f((L - Ln) * kLog2e);
    const float Lold = L;
    L = none ? Lold : (keyless ? s : Ln);
    return none ? 1.0f : (keyless ? 0.0f : w);
}

__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4& v, float w)
{
    bf16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (__bf16)(v[e] * w);
    return r;
}

// Eight OCP e4m3 codes (two words, ascending bytes) as their bf16 values: one v_cvt_scalef32_pk_bf16_fp8 per pair, at scale 1.
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(uint32_t w0, uint32_t w1)
{
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// The body of the split kernels.  PAGED (fa2_forward_decode_paged): K and V are pools [n_pages][Hkv][page_size][d] and key j of
// sequence b is row j % page_size of page block_table[b][j / page_size]; page_size is a multiple of the 32-key tile, so a tile
// lies in one page and the ONLY difference is where a tile's two buffer resources start: at the tile's first row in (page, hkv),
// min(32, end - kb) rows long, the lane offsets without the tile's base.  The tile's page is a wave-uniform scalar: its table
// entry is loaded one iteration ahead of the K/V loads that need it (which themselves run one tile ahead of the arithmetic), and
// becomes an address only after the clamp to [0, n_pages).  Only tiles with a key below `end` index the table, so the entries at
// and beyond ceil(len_b / page_size) are never read; a tile past `end` gets a resource of no rows.
//
// EB: bytes per element of K and V.  2: bf16, everything above.  1 (fa2_forward_decode_fp8kv): OCP e4m3 caches with a descale per
// K/V head (the cache holds x / descale[hkv]).  A row is D bytes, so a lane's 16-byte K load holds the elements of TWO k-steps
// (load t', words 2u ..+2: k-step 2t' + u, elements 32t' + 16h + 8u ..+8; Q's fragments are loaded in that order) and a V load
// covers twice the rows.  Both are widened to bf16 in VGPRs (exact: 3 mantissa bits, and every e4m3 exponent is a normal bf16
// one): K's on the way into the first product, V's on the way into the wave's LDS image, which -- like the transposed reads,
// both products and the softmax -- stays the bf16 one.  k_descale joins the scalar the scores are multiplied by, v_descale
// multiplies the fp32 row piece a split emits, before anything is rounded.
//
// WIN (fa2_forward_decode_window, _paged_window): a sliding window under the causal mask.  Row i sees keys [kmin_i, kmax_i),
// kmin_i = max(0, pos_i - window_left), and no row of the sequence sees a key below lo = max(0, len - Nq - window_left).  The
// splits share [base, len), base = rounddown(lo, kDecodeKB), instead of [0, len): they still start on multiples of kDecodeKB and
// a wave's tiles are the tiles of the plain call.  What lies below lo may hold anything, table entries included, so
//   a tile wholly below lo (at most three, in [base, base + kDecodeKB)) is treated like a tile past `end`: a resource of no rows
//   (every tile is bound by a resource of its own here, contiguous caches too) and table index 0;
//   the one tile that straddles lo is loaded whole -- its rows are in the slab, or in a page that holds a visible key -- and
//   its V rows below lo are zeroed in VGPRs before they enter the LDS image (0 x NaN is NaN; K's scores are selected away);
//   the two selects of a tile take kmin beside kmax.
template <int D, bool PAGED, int EB, bool WIN = false>
__device__ __forceinline__ void decode_split_body(const DecodeArgs& a)
{
    static_assert(EB == 1 || EB == 2, "bf16 or e4m3 caches");
    using kv_t = std::conditional_t<EB == 2, __bf16, uint8_t>;      // one cache element: offsets below count elements
    constexpr int ROWB = EB * D;              // bytes per cache row
    constexpr int KS = D / 16;                // k-steps of S^T = K Q^T
    constexpr int KL = ROWB / 32;             // K loads per tile: 16 bytes of the lane's row each
    constexpr int CPR = ROWB / 16;            // 16-byte chunks per row
    constexpr int RPI = 64 / CPR;             // V rows one wave-wide load covers
    constexpr int NV = kDecodeTile / RPI;     // V loads per tile
    constexpr int DB = D / 32;                // 32-column tiles of O^T
    constexpr int VIMG = kDecodeTile * 2 * D; // a wave's V image (bf16 whatever the cache holds)
    constexpr int OP = D + 4;                 // floats per row of a wave's O image (the pad spreads 32 rows over the banks)
    constexpr int C4 = D / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // kDecWaves x max(VIMG, 32 OP 4) | m, l: kDecWaves x 32 x 2 floats
    float* const s_ml = reinterpret_cast<float*>(smem + kDecWaves * 32 * OP * 4);

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = a.Hq / a.Hkv, M = G * a.Nq;
    const int bid = blockIdx.x;
    const int split = bid % a.n_splits, hkv = (bid / a.n_splits) % a.Hkv, b = bid / (a.n_splits * a.Hkv);

    // the clamp is the contract: nothing below sees the stored value
    int len = a.Ncap;
    if (a.seqlens) len = min(max(__builtin_amdgcn_readfirstlane(a.seqlens[b]), 0), a.Ncap);
    // WIN: lo without forming len - Nq - window_left (window_left may be INT_MAX, len < Nq happens); 0 otherwise
    int lo = 0;
    if constexpr (WIN) lo = len - a.Nq > a.window_left ? len - a.Nq - a.window_left : 0;
    const int base0 = WIN ? lo / kDecodeKB * kDecodeKB : 0;
    const int per = (len - base0 + a.n_splits - 1) / a.n_splits;
    const int chunk = (per + kDecodeKB - 1) / kDecodeKB * kDecodeKB;
    const int begin = base0 + split * chunk;              // <= len + n_splits kDecodeKB: no overflow
    const int end = min(begin + chunk, len);

    const size_t R = (size_t)a.B * a.Hq * a.Nq;           // rows of O, L and of one split's partials
    const size_t row0 = ((size_t)b * a.Hq + (size_t)hkv * G) * a.Nq;      // the group's first row

    // what a finished row piece becomes: a partial, or the result
    const float vd = EB == 1 && a.v_descale ? a.v_descale[hkv] : 1.0f;
    const auto emit = [&](int row, int c4, f32x4 o, float Lrow) {
        const size_t gr = row0 + row;
        if constexpr (EB == 1) o *= vd;
        if (a.n_splits > 1) {
            *reinterpret_cast<f32x4*>(a.wsO + ((size_t)split * R + gr) * D + 4 * c4) = o;
            if (c4 == 0) a.wsL[(size_t)split * R + gr] = Lrow;
        } else {
            float w = 1.0f;
            if (a.sink) w = decode_sink(a.sink[hkv * G + row / a.Nq], Lrow);
            *reinterpret_cast<bf16x4*>((__bf16*)a.O + gr * D + 4 * c4) = to_bf16x4(o, w);
            if (c4 == 0) a.L[gr] = Lrow;
        }
    };

    if (begin >= end) {                                   // an empty split (a short sequence's later splits, len = 0): no key
        for (int idx = tid; idx < M * C4; idx += 256) emit(idx / C4, idx % C4, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, -INFINITY);
        return;
    }

    // Q^T fragments: lane (row r, half h) holds Q[r][16 t + 8 h ..+8] for k-step t (EB = 1: Q[r][32 (t / 2) + 16 h + 8 (t % 2) ..+8])
    bf16x8 q[KS];
    {
        const __bf16* Qg = (const __bf16*)a.Q + (row0 + (r < M ? r : 0)) * D + (EB == 2 ? 8 : 16) * h;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            q[t] = *reinterpret_cast<const bf16x8*>(Qg + (EB == 2 ? 16 * t : 32 * (t / 2) + 8 * (t % 2)));
            if (r >= M) q[t] = bf16x8{};
        }
    }
    // keys [0, kmax) are visible to this lane's row (bottom-right causal: j <= i + len - N_q), none to a padding row
    int kmax = end;
    if (a.causal) kmax = min(end, r % a.Nq + len - a.Nq + 1);
    if (r >= M) kmax = 0;
    int kmin = 0;      // WIN: keys [kmin, kmax); a row with pos < 0 has no key whatever kmin is
    if constexpr (WIN) {
        const int pos = r % a.Nq + len - a.Nq;
        kmin = pos > a.window_left ? pos - a.window_left : 0;
    }

    const size_t slab = PAGED ? (size_t)hkv * a.page_size * D : ((size_t)b * a.Hkv + hkv) * (size_t)a.Ncap * D;
    const auto k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + slab), 0, end * ROWB, 0x00020000);
    const auto v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + slab), 0, end * ROWB, 0x00020000);
    const uint32_t koff = (uint32_t)r * ROWB + 16 * h;                       // + 32 t per load
    const uint32_t voff = (uint32_t)(lane / CPR) * ROWB + 16 * (lane % CPR);   // + RPI rows per load
    // Tiles a wave keeps in flight ahead of its arithmetic.  An e4m3 tile is half the bytes (and its fragments half the registers)
    // of a bf16 one, and with one workgroup per CU one of them in flight left the loop waiting on memory: two.
    constexpr int PF = EB == 1 ? 2 : 1;
    u32x4 kf[PF][KL], vf[PF][NV];
    // PAGED.  (pg_i, pg_o): page index and row within the page of the tile whose table entry is fetched next; a wave's tiles are
    // kDecodeKB keys apart, that is (pg_di, pg_do) further, carried without a division.  (ent, ent_o): the fetched entry and row
    // of the tile that is LOADED next.  A tile with a key indexes the table below max_pages (kb < len <= max_pages page_size);
    // one without reads entry 0 of its sequence, which the clamp and its resource of no rows keep from being used.
    // The table does not change while the kernel runs: read through the constant address space, a uniform index is a scalar load
    // whatever else the loop stores (the compiler gives up proving that for a plain global load this deep in a loop, and a
    // vector load would leave the resource in VGPRs).
    int pg_i = 0, pg_o = 0, pg_di = 0, pg_do = 0, ent = 0, ent_o = 0;
    const dec_const_int* const table = (const dec_const_int*)a.block_table + (size_t)b * a.max_pages;
    const auto fetch_entry = [&](int base) {
        // (the outer readfirstlane costs nothing on a scalar; it keeps the compiler from merging this load with the one before
        // the loop into a single load at the top of the iteration that uses it, which would undo the prefetch)
        if constexpr (WIN)      // a tile wholly below lo reads entry 0 too: the entries of pages below lo are never read
            ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end && base + kDecodeTile > lo ? pg_i : 0)]);
        else
            ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end ? pg_i : 0)]);
        ent_o = pg_o;
        pg_i += pg_di;
        pg_o += pg_do;
        if (pg_o >= a.page_size) { pg_o -= a.page_size; ++pg_i; }
    };
    const auto load_tile = [&](int base, int sl) {      // rows past `end` read as zeros (and cost no traffic)
        if constexpr (WIN) {      // a resource per tile, of no rows where the tile has no key at or above lo
            const bool live = base < end && base + kDecodeTile > lo;
            const int page = PAGED && live ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            const int rows = __builtin_amdgcn_readfirstlane(live ? min(kDecodeTile, end - base) : 0);
            const size_t at = slab + (PAGED ? (size_t)page * a.Hkv * a.page_size + ent_o : (size_t)(live ? base : 0)) * D;
            const auto kp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + at), 0, rows * ROWB, 0x00020000);
            const auto vp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(kp, koff + 32 * t, 0, 0);
#pragma unroll
            for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(vp, voff + n * RPI * ROWB, 0, 0);
            return;
        }
        if constexpr (PAGED) {
            const int page = base < end ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            // (readfirstlane: the compiler clamps with v_med3_i32, and a resource with a VGPR word is loaded in a waterfall loop)
            const int rows = __builtin_amdgcn_readfirstlane(max(min(kDecodeTile, end - base), 0));
            const size_t at = slab + ((size_t)page * a.Hkv * a.page_size + ent_o) * D;      // 64-bit: a pool may exceed 4 GiB
            const auto kp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + at), 0, rows * ROWB, 0x00020000);
            const auto vp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(kp, koff + 32 * t, 0, 0);
#pragma unroll
            for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(vp, voff + n * RPI * ROWB, 0, 0);
            return;
        }
        const uint32_t b0 = (uint32_t)base * ROWB;
#pragma unroll
        for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, b0 + koff + 32 * t, 0, 0);
#pragma unroll
        for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, b0 + voff + n * RPI * ROWB, 0, 0);
    };

    char* const vimg = smem + wave * VIMG;
    // ds_read_b64_tr_b16: lane 4 qq + p of a 16-lane group supplies row qq, columns 4 p ..+4 of a 4 x 16 block; the group's lanes
    // get the block's columns.  Group g serves half g >> 1 and columns 16 (g & 1) ..+16 of a 32-column tile of V.
    const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, c0 = 16 * ((lane >> 4) & 1);

    float m = -INFINITY, l = 0.0f;              // running maximum (log2 units) and this lane half's part of the running sum
    f32x16 o[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[c][e] = 0.0f;
    float sc = a.scale * kLog2e;
    if constexpr (EB == 1) sc *= a.k_descale ? a.k_descale[hkv] : 1.0f;

    int kb = begin + kDecodeTile * wave;
    if constexpr (PAGED) {      // the two divisions of a workgroup
        pg_i = kb / a.page_size;
        pg_o = kb - pg_i * a.page_size;
        pg_di = kDecodeKB / a.page_size;
        pg_do = kDecodeKB - pg_di * a.page_size;
        fetch_entry(kb);
    }
    load_tile(kb, 0);
    if constexpr (PAGED) fetch_entry(kb + kDecodeKB);
    if constexpr (PF == 1) {
        for (; kb < end; kb += kDecodeKB) {
#define DEC_KB kb
#define DEC_SL 0
#include "fa2_decode_tile.inc"
        }
    } else {      // two tiles in flight: slot 0 holds the wave's even tiles, slot 1 the odd ones
        load_tile(kb + kDecodeKB, 1);
        if constexpr (PAGED) fetch_entry(kb + 2 * kDecodeKB);
        for (; kb < end; kb += 2 * kDecodeKB) {
            {
#define DEC_KB kb
#define DEC_SL 0
#include "fa2_decode_tile.inc"
            }
            if (kb + kDecodeKB < end) {
#define DEC_KB (kb + kDecodeKB)
#define DEC_SL 1
#include "fa2_decode_tile.inc"
            }
        }
    }

    // the four waves' states meet: common maximum, then O and l at that maximum, summed in wave order
    l = half_sum(l);
    if (h == 0) { s_ml[(wave * 32 + r) * 2] = m; s_ml[(wave * 32 + r) * 2 + 1] = l; }
    __syncthreads();      // every wave is done with its V image: the O images below overlap them
    {
        float ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < kDecWaves; ++w) ms = fmaxf(ms, s_ml[(w * 32 + r) * 2]);
        const float f = __builtin_amdgcn_exp2f(m - (ms == -INFINITY ? 0.0f : ms));
        float* const oimg = reinterpret_cast<float*>(smem) + (wave * 32 + r) * OP + 4 * h;
#pragma unroll
        for (int c = 0; c < DB; ++c)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {      // registers 4 g4 ..+4: columns 32 c + 8 g4 + 4 h ..+4 of O's row r
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = o[c][4 * g4 + e] * f;
                *reinterpret_cast<f32x4*>(oimg + 32 * c + 8 * g4) = v;
            }
    }
    __syncthreads();
    for (int idx = tid; idx < M * C4; idx += 256) {
        const int row = idx / C4, c4 = idx % C4;
        float ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < kDecWaves; ++w) ms = fmaxf(ms, s_ml[(w * 32 + row) * 2]);
        const float ms0 = ms == -INFINITY ? 0.0f : ms;
        float lt = 0.0f;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int w = 0; w < kDecWaves; ++w) {
            lt += s_ml[(w * 32 + row) * 2 + 1] * __builtin_amdgcn_exp2f(s_ml[(w * 32 + row) * 2] - ms0);
            acc += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem) + (w * 32 + row) * OP + 4 * c4);
        }
        const bool has = lt > 0.0f;             // a select: a row without a visible key in this split
        const float inv = 1.0f / lt;
        f32x4 out;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = has ? acc[e] * inv : 0.0f;
        emit(row, c4, out, has ? (ms + __builtin_amdgcn_logf(lt)) * kDecLn2 : -INFINITY);      // (v_log_f32 is log2)
    }
}

// EXTEND (fa2_forward_extend, include/fa2_extend_mi355x.h): decode_split_body with RT = 2 row tiles per wave, for any M.  The data path,
// the loads, the page and window handling are decode_split_body's, statement for statement (a body of its own and not a parameter
// of that one: with the parameter the ten kernels above came out of the compiler re-scheduled, tools/asm_identity.py).  A workgroup
// is (sequence, K/V head, block of 32 RT rows, split), block j owning rows 64 j ..+64 of the group's [G][Nq] slab (row rho: head
// rho / Nq, token rho % Nq; rows >= M are padding).  Every K fragment and every V image a wave loads feeds the products of both
// row tiles, so the K/V head is streamed once per 64 rows.  The split ranges are decode_split_body's (shared by the blocks of a
// sequence); a block clips its own: it stops at the largest kmax of its rows and, under a window, starts at the 32-key tile
// that holds the smallest kmin of its rows, each wave at the first of ITS tiles (w, w + 4, ... counted from the split's first)
// at or behind that one.  The clip only drops tiles whose every probability would be selected to 0, a row's arithmetic does
// not depend on the tile it sits in, and the waves' states meet row tile by row tile through the same LDS image: a row's
// result is bit for bit the one decode_split_body computes for it.
template <int D, bool PAGED, int EB, bool WIN>
__device__ __forceinline__ void extend_split_body(const DecodeArgs& a)
{
    constexpr int RT = kExtendRows / 32;      // row tiles per wave
    static_assert(EB == 1 || EB == 2, "bf16 or e4m3 caches");
    using kv_t = std::conditional_t<EB == 2, __bf16, uint8_t>;      // one cache element: offsets below count elements
    constexpr int ROWB = EB * D;              // bytes per cache row
    constexpr int KS = D / 16;                // k-steps of S^T = K Q^T
    constexpr int KL = ROWB / 32;             // K loads per tile: 16 bytes of the lane's row each
    constexpr int CPR = ROWB / 16;            // 16-byte chunks per row
    constexpr int RPI = 64 / CPR;             // V rows one wave-wide load covers
    constexpr int NV = kDecodeTile / RPI;     // V loads per tile
    constexpr int DB = D / 32;                // 32-column tiles of O^T
    constexpr int VIMG = kDecodeTile * 2 * D; // a wave's V image (bf16 whatever the cache holds)
    constexpr int OP = D + 4;                 // floats per row of a wave's O image (the pad spreads 32 rows over the banks)
    constexpr int C4 = D / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // kDecWaves x max(VIMG, 32 OP 4) | m, l: kDecWaves x 32 x 2 floats
    float* const s_ml = reinterpret_cast<float*>(smem + kDecWaves * 32 * OP * 4);

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = a.Hq / a.Hkv, M = G * a.Nq;
    const int bid = blockIdx.x;
    const int RB = (M + 32 * RT - 1) / (32 * RT);      // row blocks of a group
    const int split = bid % a.n_splits, hkv = (bid / (a.n_splits * RB)) % a.Hkv, b = bid / (a.n_splits * RB * a.Hkv);
    const int rb0 = bid / a.n_splits % RB * (32 * RT);      // the block's first row
    const int Mb = min(M - rb0, 32 * RT);              // its live rows

    // the clamp is the contract: nothing below sees the stored value
    int len = a.Ncap;
    if (a.seqlens) len = min(max(__builtin_amdgcn_readfirstlane(a.seqlens[b]), 0), a.Ncap);
    // WIN: lo without forming len - Nq - window_left (window_left may be INT_MAX, len < Nq happens); 0 otherwise
    int lo = 0;
    if constexpr (WIN) lo = len - a.Nq > a.window_left ? len - a.Nq - a.window_left : 0;
    const int base0 = WIN ? lo / kDecodeKB * kDecodeKB : 0;
    const int per = (len - base0 + a.n_splits - 1) / a.n_splits;
    const int chunk = (per + kDecodeKB - 1) / kDecodeKB * kDecodeKB;
    const int begin = base0 + split * chunk;              // <= len + n_splits kDecodeKB: no overflow
    int end = min(begin + chunk, len);
    int cstart = 0;      // WIN: the first tile with a key visible to a row of the block
    {      // the block's clip: its rows' tokens are [tlo, thi], all of them where it crosses a head
        const int rl = rb0 + Mb - 1;
        const bool wrap = rb0 / a.Nq != rl / a.Nq;
        const int tlo = wrap ? 0 : rb0 % a.Nq, thi = wrap ? a.Nq - 1 : rl % a.Nq;
        if (a.causal) end = min(end, thi + len - a.Nq + 1);
        if constexpr (WIN) {
            const int pos = tlo + len - a.Nq;
            cstart = (pos > a.window_left ? pos - a.window_left : 0) / kDecodeTile * kDecodeTile;
        }
    }

    const size_t R = (size_t)a.B * a.Hq * a.Nq;           // rows of O, L and of one split's partials
    const size_t row0 = ((size_t)b * a.Hq + (size_t)hkv * G) * a.Nq;      // the group's first row

    // what a finished row piece becomes: a partial, or the result
    const float vd = EB == 1 && a.v_descale ? a.v_descale[hkv] : 1.0f;
    const auto emit = [&](int row, int c4, f32x4 o, float Lrow) {
        const size_t gr = row0 + row;
        if constexpr (EB == 1) o *= vd;
        if (a.n_splits > 1) {
            *reinterpret_cast<f32x4*>(a.wsO + ((size_t)split * R + gr) * D + 4 * c4) = o;
            if (c4 == 0) a.wsL[(size_t)split * R + gr] = Lrow;
        } else {
            float w = 1.0f;
            if (a.sink) w = decode_sink(a.sink[hkv * G + row / a.Nq], Lrow);
            *reinterpret_cast<bf16x4*>((__bf16*)a.O + gr * D + 4 * c4) = to_bf16x4(o, w);
            if (c4 == 0) a.L[gr] = Lrow;
        }
    };

    if (begin >= end || (WIN && cstart >= end)) {      // an empty split (a short sequence's later splits, len = 0): no key
        for (int idx = tid; idx < Mb * C4; idx += 256) emit(rb0 + idx / C4, idx % C4, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, -INFINITY);
        return;
    }

    // Q^T fragments: lane (row r, half h) holds Q[r][16 t + 8 h ..+8] for k-step t (EB = 1: Q[r][32 (t / 2) + 16 h + 8 (t % 2) ..+8])
    // (row tile i of the wave: the lane's row is rho = rb0 + 32 i + r)
    bf16x8 q[RT][KS];
    int kmax[RT], kmin[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int rho = rb0 + 32 * i + r;
        const __bf16* Qg = (const __bf16*)a.Q + (row0 + (rho < M ? rho : 0)) * D + (EB == 2 ? 8 : 16) * h;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            q[i][t] = *reinterpret_cast<const bf16x8*>(Qg + (EB == 2 ? 16 * t : 32 * (t / 2) + 8 * (t % 2)));
            if (rho >= M) q[i][t] = bf16x8{};
        }
        // keys [0, kmax) are visible to this lane's row (bottom-right causal: j <= i + len - N_q), none to a padding row
        kmax[i] = end;
        if (a.causal) kmax[i] = min(end, rho % a.Nq + len - a.Nq + 1);
        if (rho >= M) kmax[i] = 0;
        kmin[i] = 0;      // WIN: keys [kmin, kmax); a row with pos < 0 has no key whatever kmin is
        if constexpr (WIN) {
            const int pos = rho % a.Nq + len - a.Nq;
            kmin[i] = pos > a.window_left ? pos - a.window_left : 0;
        }
    }

    const size_t slab = PAGED ? (size_t)hkv * a.page_size * D : ((size_t)b * a.Hkv + hkv) * (size_t)a.Ncap * D;
    const auto k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + slab), 0, end * ROWB, 0x00020000);
    const auto v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + slab), 0, end * ROWB, 0x00020000);
    const uint32_t koff = (uint32_t)r * ROWB + 16 * h;                       // + 32 t per load
    const uint32_t voff = (uint32_t)(lane / CPR) * ROWB + 16 * (lane % CPR);   // + RPI rows per load
    // Tiles a wave keeps in flight ahead of its arithmetic.  An e4m3 tile is half the bytes (and its fragments half the registers)
    // of a bf16 one, and with one workgroup per CU one of them in flight left the loop waiting on memory: two.
    constexpr int PF = EB == 1 ? 2 : 1;
    u32x4 kf[PF][KL], vf[PF][NV];
    // PAGED.  (pg_i, pg_o): page index and row within the page of the tile whose table entry is fetched next; a wave's tiles are
    // kDecodeKB keys apart, that is (pg_di, pg_do) further, carried without a division.  (ent, ent_o): the fetched entry and row
    // of the tile that is LOADED next.  A tile with a key indexes the table below max_pages (kb < len <= max_pages page_size);
    // one without reads entry 0 of its sequence, which the clamp and its resource of no rows keep from being used.
    // The table does not change while the kernel runs: read through the constant address space, a uniform index is a scalar load
    // whatever else the loop stores (the compiler gives up proving that for a plain global load this deep in a loop, and a
    // vector load would leave the resource in VGPRs).
    int pg_i = 0, pg_o = 0, pg_di = 0, pg_do = 0, ent = 0, ent_o = 0;
    const dec_const_int* const table = (const dec_const_int*)a.block_table + (size_t)b * a.max_pages;
    const auto fetch_entry = [&](int base) {
        // (the outer readfirstlane costs nothing on a scalar; it keeps the compiler from merging this load with the one before
        // the loop into a single load at the top of the iteration that uses it, which would undo the prefetch)
        if constexpr (WIN)      // a tile wholly below lo reads entry 0 too: the entries of pages below lo are never read
            ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end && base + kDecodeTile > lo ? pg_i : 0)]);
        else
            ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end ? pg_i : 0)]);
        ent_o = pg_o;
        pg_i += pg_di;
        pg_o += pg_do;
        if (pg_o >= a.page_size) { pg_o -= a.page_size; ++pg_i; }
    };
    const auto load_tile = [&](int base, int sl) {      // rows past `end` read as zeros (and cost no traffic)
        if constexpr (WIN) {      // a resource per tile, of no rows where the tile has no key at or above lo
            const bool live = base < end && base + kDecodeTile > lo;
            const int page = PAGED && live ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            const int rows = __builtin_amdgcn_readfirstlane(live ? min(kDecodeTile, end - base) : 0);
            const size_t at = slab + (PAGED ? (size_t)page * a.Hkv * a.page_size + ent_o : (size_t)(live ? base : 0)) * D;
            const auto kp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + at), 0, rows * ROWB, 0x00020000);
            const auto vp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(kp, koff + 32 * t, 0, 0);
#pragma unroll
            for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(vp, voff + n * RPI * ROWB, 0, 0);
            return;
        }
        if constexpr (PAGED) {
            const int page = base < end ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            // (readfirstlane: the compiler clamps with v_med3_i32, and a resource with a VGPR word is loaded in a waterfall loop)
            const int rows = __builtin_amdgcn_readfirstlane(max(min(kDecodeTile, end - base), 0));
            const size_t at = slab + ((size_t)page * a.Hkv * a.page_size + ent_o) * D;      // 64-bit: a pool may exceed 4 GiB
            const auto kp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + at), 0, rows * ROWB, 0x00020000);
            const auto vp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(kp, koff + 32 * t, 0, 0);
#pragma unroll
            for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(vp, voff + n * RPI * ROWB, 0, 0);
            return;
        }
        const uint32_t b0 = (uint32_t)base * ROWB;
#pragma unroll
        for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, b0 + koff + 32 * t, 0, 0);
#pragma unroll
        for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, b0 + voff + n * RPI * ROWB, 0, 0);
    };

    char* const vimg = smem + wave * VIMG;
    // ds_read_b64_tr_b16: lane 4 qq + p of a 16-lane group supplies row qq, columns 4 p ..+4 of a 4 x 16 block; the group's lanes
    // get the block's columns.  Group g serves half g >> 1 and columns 16 (g & 1) ..+16 of a 32-column tile of V.
    const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, c0 = 16 * ((lane >> 4) & 1);

    float m[RT], l[RT];                         // running maximum (log2 units) and this lane half's part of the running sum
    f32x16 o[RT][DB];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        m[i] = -INFINITY;
        l[i] = 0.0f;
#pragma unroll
        for (int c = 0; c < DB; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[i][c][e] = 0.0f;
    }
    float sc = a.scale * kLog2e;
    if constexpr (EB == 1) sc *= a.k_descale ? a.k_descale[hkv] : 1.0f;

    int kb = begin + kDecodeTile * wave;
    if constexpr (WIN)      // the wave's first tile at or behind the block's first
        if (cstart > kb) kb += (cstart - kb + kDecodeKB - 1) / kDecodeKB * kDecodeKB;
    if constexpr (PAGED) {      // the two divisions of a workgroup
        pg_i = kb / a.page_size;
        pg_o = kb - pg_i * a.page_size;
        pg_di = kDecodeKB / a.page_size;
        pg_do = kDecodeKB - pg_di * a.page_size;
        fetch_entry(kb);
    }
    load_tile(kb, 0);
    if constexpr (PAGED) fetch_entry(kb + kDecodeKB);
    if constexpr (PF == 1) {
        for (; kb < end; kb += kDecodeKB) {
#define DEC_KB kb
#define DEC_SL 0
#include "fa2_extend_tile.inc"
        }
    } else {      // two tiles in flight: slot 0 holds the wave's even tiles, slot 1 the odd ones
        load_tile(kb + kDecodeKB, 1);
        if constexpr (PAGED) fetch_entry(kb + 2 * kDecodeKB);
        for (; kb < end; kb += 2 * kDecodeKB) {
            {
#define DEC_KB kb
#define DEC_SL 0
#include "fa2_extend_tile.inc"
            }
            if (kb + kDecodeKB < end) {
#define DEC_KB (kb + kDecodeKB)
#define DEC_SL 1
#include "fa2_extend_tile.inc"
            }
        }
    }

    // the four waves' states meet, row tile by row tile: common maximum, then O and l at that maximum, summed in wave order
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        if (i) __syncthreads();      // the tile before is out of the images
        l[i] = half_sum(l[i]);
        if (h == 0) { s_ml[(wave * 32 + r) * 2] = m[i]; s_ml[(wave * 32 + r) * 2 + 1] = l[i]; }
        __syncthreads();      // every wave is done with its V image: the O images below overlap them
        {
            float ms = -INFINITY;
#pragma unroll
            for (int w = 0; w < kDecWaves; ++w) ms = fmaxf(ms, s_ml[(w * 32 + r) * 2]);
            const float f = __builtin_amdgcn_exp2f(m[i] - (ms == -INFINITY ? 0.0f : ms));
            float* const oimg = reinterpret_cast<float*>(smem) + (wave * 32 + r) * OP + 4 * h;
#pragma unroll
            for (int c = 0; c < DB; ++c)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {      // registers 4 g4 ..+4: columns 32 c + 8 g4 + 4 h ..+4 of O's row r
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = o[i][c][4 * g4 + e] * f;
                    *reinterpret_cast<f32x4*>(oimg + 32 * c + 8 * g4) = v;
                }
        }
        __syncthreads();
        const int Mi = min(max(Mb - 32 * i, 0), 32);      // the tile's live rows
        for (int idx = tid; idx < Mi * C4; idx += 256) {
            const int row = idx / C4, c4 = idx % C4;
            float ms = -INFINITY;
#pragma unroll
            for (int w = 0; w < kDecWaves; ++w) ms = fmaxf(ms, s_ml[(w * 32 + row) * 2]);
            const float ms0 = ms == -INFINITY ? 0.0f : ms;
            float lt = 0.0f;
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int w = 0; w < kDecWaves; ++w) {
                lt += s_ml[(w * 32 + row) * 2 + 1] * __builtin_amdgcn_exp2f(s_ml[(w * 32 + row) * 2] - ms0);
                acc += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem) + (w * 32 + row) * OP + 4 * c4);
            }
            const bool has = lt > 0.0f;             // a select: a row without a visible key in this split
            const float inv = 1.0f / lt;
            f32x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = has ? acc[e] * inv : 0.0f;
            emit(rb0 + 32 * i + row, c4, out, has ? (ms + __builtin_amdgcn_logf(lt)) * kDecLn2 : -INFINITY);      // (v_log_f32 is log2)
        }
    }
}

// RAGGED EXTEND (fa2_forward_extend_ragged, include/fa2_extend_ragged_mi355x.h): extend_split_body with a q_len per sequence and
// token-major rows.  A third body and not a parameter of that one, for the reason that one is no parameter of the first.  Three
// things differ.  (1) The workgroup is (work item, K/V head, split): the item -- (sequence b, row block) -- and the sequence's
// (start, qn) come out of the PLAN (fa2_launch.h) with scalar loads, never out of cu_seqlens_q; a tail item, a plan made for
// another B, G or T, and an entry out of range end the workgroup before it touches anything.  (2) a.Nq is qn throughout.
// (3) Row rho of the [G][qn] slab is row (start + rho % qn) Hq + hkv G + rho / qn of O, L and the partials, and its Q row
// stands q_stride elements per token from Q.  The tile loop is fa2_extend_tile.inc, unchanged: with the same n_splits a row's
// O and L are bit for bit what extend_split_body gives for it in a call on its sequence alone.
template <int D, bool PAGED, int EB, bool WIN>
__device__ __forceinline__ void extend_ragged_split_body(const ExtendRaggedArgs& x)
{
    const DecodeArgs& a = x.a;
    constexpr int RT = kExtendRows / 32;      // row tiles per wave
    static_assert(EB == 1 || EB == 2, "bf16 or e4m3 caches");
    using kv_t = std::conditional_t<EB == 2, __bf16, uint8_t>;      // one cache element: offsets below count elements
    constexpr int ROWB = EB * D;              // bytes per cache row
    constexpr int KS = D / 16;                // k-steps of S^T = K Q^T
    constexpr int KL = ROWB / 32;             // K loads per tile: 16 bytes of the lane's row each
    constexpr int CPR = ROWB / 16;            // 16-byte chunks per row
    constexpr int RPI = 64 / CPR;             // V rows one wave-wide load covers
    constexpr int NV = kDecodeTile / RPI;     // V loads per tile
    constexpr int DB = D / 32;                // 32-column tiles of O^T
    constexpr int VIMG = kDecodeTile * 2 * D; // a wave's V image (bf16 whatever the cache holds)
    constexpr int OP = D + 4;                 // floats per row of a wave's O image (the pad spreads 32 rows over the banks)
    constexpr int C4 = D / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // kDecWaves x max(VIMG, 32 OP 4) | m, l: kDecWaves x 32 x 2 floats
    float* const s_ml = reinterpret_cast<float*>(smem + kDecWaves * 32 * OP * 4);

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = a.Hq / a.Hkv;
    const int bid = blockIdx.x;
    const int split = bid % a.n_splits, hkv = (bid / a.n_splits) % a.Hkv, item = bid / (a.n_splits * a.Hkv);      // item < max_blocks

    // the plan is the contract: nothing below sees cu_seqlens_q, and every entry is checked before it becomes an address
    const dec_const_int* const plan = (const dec_const_int*)x.plan;
    if (plan[0] != a.B || plan[1] != G || plan[2] != x.T) return;
    const dec_const_int* const pseq = plan + kRaggedPlanHeader;
    const dec_const_int* const pitems = pseq + 2 * (size_t)a.B;
    const int b = __builtin_amdgcn_readfirstlane(pitems[2 * (size_t)item]);
    const int jb = __builtin_amdgcn_readfirstlane(pitems[2 * (size_t)item + 1]);
    if (b < 0 || b >= a.B || jb < 0) return;      // the tail
    const int start = __builtin_amdgcn_readfirstlane(pseq[2 * (size_t)b]), qn = __builtin_amdgcn_readfirstlane(pseq[2 * (size_t)b + 1]);
    if (start < 0 || qn <= 0 || qn > x.T - start) return;
    const int M = G * qn;                     // <= T Hq, which fits
    if (jb > (M - 1) / (32 * RT)) return;
    const int rb0 = jb * (32 * RT);           // the block's first row
    const int Mb = min(M - rb0, 32 * RT);     // its live rows

    // the clamp is the contract: nothing below sees the stored value
    int len = a.Ncap;
    if (a.seqlens) len = min(max(__builtin_amdgcn_readfirstlane(a.seqlens[b]), 0), a.Ncap);
    // WIN: lo without forming len - qn - window_left (window_left may be INT_MAX, len < qn happens); 0 otherwise
    int lo = 0;
    if constexpr (WIN) lo = len - qn > a.window_left ? len - qn - a.window_left : 0;
    const int base0 = WIN ? lo / kDecodeKB * kDecodeKB : 0;
    const int per = (len - base0 + a.n_splits - 1) / a.n_splits;
    const int chunk = (per + kDecodeKB - 1) / kDecodeKB * kDecodeKB;
    const int begin = base0 + split * chunk;              // <= len + n_splits kDecodeKB: no overflow
    int end = min(begin + chunk, len);
    int cstart = 0;      // WIN: the first tile with a key visible to a row of the block
    {      // the block's clip: its rows' tokens are [tlo, thi], all of them where it crosses a head
        const int rl = rb0 + Mb - 1;
        const bool wrap = rb0 / qn != rl / qn;
        const int tlo = wrap ? 0 : rb0 % qn, thi = wrap ? qn - 1 : rl % qn;
        if (a.causal) end = min(end, thi + len - qn + 1);
        if constexpr (WIN) {
            const int pos = tlo + len - qn;
            cstart = (pos > a.window_left ? pos - a.window_left : 0) / kDecodeTile * kDecodeTile;
        }
    }

    const size_t R = (size_t)x.T * a.Hq;                  // rows of O, L and of one split's partials

    // what a finished row piece becomes: a partial, or the result
    const float vd = EB == 1 && a.v_descale ? a.v_descale[hkv] : 1.0f;
    const auto emit = [&](int row, int c4, f32x4 o, float Lrow) {
        const int head = hkv * G + row / qn;
        const size_t gr = (size_t)(start + row % qn) * a.Hq + head;      // token-major
        if constexpr (EB == 1) o *= vd;
        if (a.n_splits > 1) {
            *reinterpret_cast<f32x4*>(a.wsO + ((size_t)split * R + gr) * D + 4 * c4) = o;
            if (c4 == 0) a.wsL[(size_t)split * R + gr] = Lrow;
        } else {
            float w = 1.0f;
            if (a.sink) w = decode_sink(a.sink[head], Lrow);
            *reinterpret_cast<bf16x4*>((__bf16*)a.O + gr * D + 4 * c4) = to_bf16x4(o, w);
            if (c4 == 0) a.L[gr] = Lrow;
        }
    };

    if (begin >= end || (WIN && cstart >= end)) {      // an empty split (a short sequence's later splits, len = 0): no key
        for (int idx = tid; idx < Mb * C4; idx += 256) emit(rb0 + idx / C4, idx % C4, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, -INFINITY);
        return;
    }

    // Q^T fragments: lane (row r, half h) holds Q[r][16 t + 8 h ..+8] for k-step t (EB = 1: Q[r][32 (t / 2) + 16 h + 8 (t % 2) ..+8])
    // (row tile i of the wave: the lane's row is rho = rb0 + 32 i + r)
    bf16x8 q[RT][KS];
    int kmax[RT], kmin[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int rho = rb0 + 32 * i + r;
        const int rq = rho < M ? rho : 0;
        const __bf16* Qg = (const __bf16*)a.Q + (size_t)(start + rq % qn) * (size_t)x.q_stride + (size_t)(hkv * G + rq / qn) * D +
                           (EB == 2 ? 8 : 16) * h;
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            q[i][t] = *reinterpret_cast<const bf16x8*>(Qg + (EB == 2 ? 16 * t : 32 * (t / 2) + 8 * (t % 2)));
            if (rho >= M) q[i][t] = bf16x8{};
        }
        // keys [0, kmax) are visible to this lane's row (bottom-right causal: j <= i + len - q_b), none to a padding row
        kmax[i] = end;
        if (a.causal) kmax[i] = min(end, rho % qn + len - qn + 1);
        if (rho >= M) kmax[i] = 0;
        kmin[i] = 0;      // WIN: keys [kmin, kmax); a row with pos < 0 has no key whatever kmin is
        if constexpr (WIN) {
            const int pos = rho % qn + len - qn;
            kmin[i] = pos > a.window_left ? pos - a.window_left : 0;
        }
    }

    const size_t slab = PAGED ? (size_t)hkv * a.page_size * D : ((size_t)b * a.Hkv + hkv) * (size_t)a.Ncap * D;
    const auto k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + slab), 0, end * ROWB, 0x00020000);
    const auto v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + slab), 0, end * ROWB, 0x00020000);
    const uint32_t koff = (uint32_t)r * ROWB + 16 * h;                       // + 32 t per load
    const uint32_t voff = (uint32_t)(lane / CPR) * ROWB + 16 * (lane % CPR);   // + RPI rows per load
    constexpr int PF = EB == 1 ? 2 : 1;       // tiles a wave keeps in flight ahead of its arithmetic (extend_split_body)
    u32x4 kf[PF][KL], vf[PF][NV];
    // PAGED: extend_split_body's table walk, statement for statement
    int pg_i = 0, pg_o = 0, pg_di = 0, pg_do = 0, ent = 0, ent_o = 0;
    const dec_const_int* const table = (const dec_const_int*)a.block_table + (size_t)b * a.max_pages;
    const auto fetch_entry = [&](int base) {
        if constexpr (WIN)      // a tile wholly below lo reads entry 0 too: the entries of pages below lo are never read
            ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end && base + kDecodeTile > lo ? pg_i : 0)]);
        else
            ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end ? pg_i : 0)]);
        ent_o = pg_o;
        pg_i += pg_di;
        pg_o += pg_do;
        if (pg_o >= a.page_size) { pg_o -= a.page_size; ++pg_i; }
    };
    const auto load_tile = [&](int base, int sl) {      // rows past `end` read as zeros (and cost no traffic)
        if constexpr (WIN) {      // a resource per tile, of no rows where the tile has no key at or above lo
            const bool live = base < end && base + kDecodeTile > lo;
            const int page = PAGED && live ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            const int rows = __builtin_amdgcn_readfirstlane(live ? min(kDecodeTile, end - base) : 0);
            const size_t at = slab + (PAGED ? (size_t)page * a.Hkv * a.page_size + ent_o : (size_t)(live ? base : 0)) * D;
            const auto kp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + at), 0, rows * ROWB, 0x00020000);
            const auto vp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(kp, koff + 32 * t, 0, 0);
#pragma unroll
            for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(vp, voff + n * RPI * ROWB, 0, 0);
            return;
        }
        if constexpr (PAGED) {
            const int page = base < end ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            const int rows = __builtin_amdgcn_readfirstlane(max(min(kDecodeTile, end - base), 0));
            const size_t at = slab + ((size_t)page * a.Hkv * a.page_size + ent_o) * D;      // 64-bit: a pool may exceed 4 GiB
            const auto kp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.K + at), 0, rows * ROWB, 0x00020000);
            const auto vp = __builtin_amdgcn_make_buffer_rsrc((void*)((const kv_t*)a.V + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(kp, koff + 32 * t, 0, 0);
#pragma unroll
            for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(vp, voff + n * RPI * ROWB, 0, 0);
            return;
        }
        const uint32_t b0 = (uint32_t)base * ROWB;
#pragma unroll
        for (int t = 0; t < KL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, b0 + koff + 32 * t, 0, 0);
#pragma unroll
        for (int n = 0; n < NV; ++n) vf[sl][n] = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, b0 + voff + n * RPI * ROWB, 0, 0);
    };

    char* const vimg = smem + wave * VIMG;
    const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, c0 = 16 * ((lane >> 4) & 1);      // ds_read_b64_tr_b16's lane roles

    float m[RT], l[RT];                         // running maximum (log2 units) and this lane half's part of the running sum
    f32x16 o[RT][DB];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        m[i] = -INFINITY;
        l[i] = 0.0f;
#pragma unroll
        for (int c = 0; c < DB; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[i][c][e] = 0.0f;
    }
    float sc = a.scale * kLog2e;
    if constexpr (EB == 1) sc *= a.k_descale ? a.k_descale[hkv] : 1.0f;

    int kb = begin + kDecodeTile * wave;
    if constexpr (WIN)      // the wave's first tile at or behind the block's first
        if (cstart > kb) kb += (cstart - kb + kDecodeKB - 1) / kDecodeKB * kDecodeKB;
    if constexpr (PAGED) {      // the two divisions of a workgroup
        pg_i = kb / a.page_size;
        pg_o = kb - pg_i * a.page_size;
        pg_di = kDecodeKB / a.page_size;
        pg_do = kDecodeKB - pg_di * a.page_size;
        fetch_entry(kb);
    }
    load_tile(kb, 0);
    if constexpr (PAGED) fetch_entry(kb + kDecodeKB);
    if constexpr (PF == 1) {
        for (; kb < end; kb += kDecodeKB) {
#define DEC_KB kb
#define DEC_SL 0
#include "fa2_extend_tile.inc"
        }
    } else {      // two tiles in flight: slot 0 holds the wave's even tiles, slot 1 the odd ones
        load_tile(kb + kDecodeKB, 1);
        if constexpr (PAGED) fetch_entry(kb + 2 * kDecodeKB);
        for (; kb < end; kb += 2 * kDecodeKB) {
            {
#define DEC_KB kb
#define DEC_SL 0
#include "fa2_extend_tile.inc"
            }
            if (kb + kDecodeKB < end) {
#define DEC_KB (kb + kDecodeKB)
#define DEC_SL 1
#include "fa2_extend_tile.inc"
            }
        }
    }

    // the four waves' states meet, row tile by row tile: common maximum, then O and l at that maximum, summed in wave order
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        if (i) __syncthreads();      // the tile before is out of the images
        l[i] = half_sum(l[i]);
        if (h == 0) { s_ml[(wave * 32 + r) * 2] = m[i]; s_ml[(wave * 32 + r) * 2 + 1] = l[i]; }
        __syncthreads();      // every wave is done with its V image: the O images below overlap them
        {
            float ms = -INFINITY;
#pragma unroll
            for (int w = 0; w < kDecWaves; ++w) ms = fmaxf(ms, s_ml[(w * 32 + r) * 2]);
            const float f = __builtin_amdgcn_exp2f(m[i] - (ms == -INFINITY ? 0.0f : ms));
            float* const oimg = reinterpret_cast<float*>(smem) + (wave * 32 + r) * OP + 4 * h;
#pragma unroll
            for (int c = 0; c < DB; ++c)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {      // registers 4 g4 ..+4: columns 32 c + 8 g4 + 4 h ..+4 of O's row r
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = o[i][c][4 * g4 + e] * f;
                    *reinterpret_cast<f32x4*>(oimg + 32 * c + 8 * g4) = v;
                }
        }
        __syncthreads();
        const int Mi = min(max(Mb - 32 * i, 0), 32);      // the tile's live rows
        for (int idx = tid; idx < Mi * C4; idx += 256) {
            const int row = idx / C4, c4 = idx % C4;
            float ms = -INFINITY;
#pragma unroll
            for (int w = 0; w < kDecWaves; ++w) ms = fmaxf(ms, s_ml[(w * 32 + row) * 2]);
            const float ms0 = ms == -INFINITY ? 0.0f : ms;
            float lt = 0.0f;
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int w = 0; w < kDecWaves; ++w) {
                lt += s_ml[(w * 32 + row) * 2 + 1] * __builtin_amdgcn_exp2f(s_ml[(w * 32 + row) * 2] - ms0);
                acc += *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(smem) + (w * 32 + row) * OP + 4 * c4);
            }
            const bool has = lt > 0.0f;             // a select: a row without a visible key in this split
            const float inv = 1.0f / lt;
            f32x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] = has ? acc[e] * inv : 0.0f;
            emit(rb0 + 32 * i + row, c4, out, has ? (ms + __builtin_amdgcn_logf(lt)) * kDecLn2 : -INFINITY);      // (v_log_f32 is log2)
        }
    }
}

}  // namespace

template <int D>
__global__ void __launch_bounds__(256) fa2_decode_split_kernel(DecodeArgs a)
{
    decode_split_body<D, false, 2>(a);
}

template <int D>
__global__ void __launch_bounds__(256) fa2_decode_paged_split_kernel(DecodeArgs a)
{
    decode_split_body<D, true, 2>(a);
}

// fa2_forward_decode_fp8kv / _paged_fp8kv: the same body over e4m3 caches (EB = 1)
template <int D>
__global__ void __launch_bounds__(256) fa2_decode_f8_split_kernel(DecodeArgs a)
{
    decode_split_body<D, false, 1>(a);
}

template <int D>
__global__ void __launch_bounds__(256) fa2_decode_f8_paged_split_kernel(DecodeArgs a)
{
    decode_split_body<D, true, 1>(a);
}

// fa2_forward_decode_window / _paged_window: the same body with the window (WIN), over both element sizes
template <int D>
__global__ void __launch_bounds__(256) fa2_decode_win_split_kernel(DecodeArgs a)
{
    decode_split_body<D, false, 2, true>(a);
}

template <int D>
__global__ void __launch_bounds__(256) fa2_decode_win_paged_split_kernel(DecodeArgs a)
{
    decode_split_body<D, true, 2, true>(a);
}

template <int D>
__global__ void __launch_bounds__(256) fa2_decode_win_f8_split_kernel(DecodeArgs a)
{
    decode_split_body<D, false, 1, true>(a);
}

template <int D>
__global__ void __launch_bounds__(256) fa2_decode_win_f8_paged_split_kernel(DecodeArgs a)
{
    decode_split_body<D, true, 1, true>(a);
}

// fa2_forward_extend / _paged (include/fa2_extend_mi355x.h): extend_split_body, any M
template <int D, bool PAGED, int EB, bool WIN>
__global__ void __launch_bounds__(256) fa2_extend_split_kernel(DecodeArgs a)
{
    extend_split_body<D, PAGED, EB, WIN>(a);
}

// rows x d / 4 lanes, a lane owns four columns of one row: partials in, ascending s, fp32; the sink; one rounding
template <int D>
__global__ void __launch_bounds__(256) fa2_decode_combine_kernel(DecodeArgs a)
{
    constexpr int C4 = D / 4;
    const size_t R = (size_t)a.B * a.Hq * a.Nq;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = t / C4;
    const int c4 = (int)(t % C4);
    if (row >= R) return;
#define DEC_NQ a.Nq
#include "fa2_decode_combine.inc"
}

int decode_num_splits(int B, int H_kv, int kv_capacity)
{
    const long long groups = (long long)B * H_kv;
    const long long fill = (kDecodeCUs + groups - 1) / groups;               // smallest s with B H_kv s >= the CU count
    const long long room = std::max(1, kv_capacity / kDecodeMinSplitKeys);   // a split of a full cache keeps that many keys
    return (int)std::min<long long>(std::min(fill, room), kDecodeMaxSplits);
}

template <int D>
static hipError_t decode_launch(const DecodeArgs& a, hipStream_t stream)
{
    constexpr int lds = kDecWaves * 32 * (D + 4) * 4 + kDecWaves * 32 * 2 * 4;
    static_assert(kDecWaves * kDecodeTile * 2 * D <= kDecWaves * 32 * (D + 4) * 4, "the V images fit under the O images");
    const unsigned grid = (unsigned)a.B * a.Hkv * a.n_splits;
    hipError_t e;
    if (a.window_left >= 0 && a.kv_fp8)
        e = a.block_table ? launch_lds<fa2_decode_win_f8_paged_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a)
                          : launch_lds<fa2_decode_win_f8_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a);
    else if (a.window_left >= 0)
        e = a.block_table ? launch_lds<fa2_decode_win_paged_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a)
                          : launch_lds<fa2_decode_win_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a);
    else if (a.kv_fp8)
        e = a.block_table ? launch_lds<fa2_decode_f8_paged_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a)
                          : launch_lds<fa2_decode_f8_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a);
    else
        e = a.block_table ? launch_lds<fa2_decode_paged_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a)
                          : launch_lds<fa2_decode_split_kernel<D>>(dim3(grid), dim3(256), lds, stream, a);
    if (e != hipSuccess || a.n_splits == 1) return e;
    const size_t threads = (size_t)a.B * a.Hq * a.Nq * (D / 4);
    hipLaunchKernelGGL(fa2_decode_combine_kernel<D>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <int D, bool PAGED, int EB>
static hipError_t extend_launch(const DecodeArgs& a, hipStream_t stream)
{
    constexpr int lds = kDecWaves * 32 * (D + 4) * 4 + kDecWaves * 32 * 2 * 4;      // decode_launch's: the row tiles take turns
    const int M = a.Hq / a.Hkv * a.Nq;
    const unsigned grid = (unsigned)a.B * a.Hkv * ((M + kExtendRows - 1) / kExtendRows) * a.n_splits;
    const hipError_t e = a.window_left >= 0 ? launch_lds<fa2_extend_split_kernel<D, PAGED, EB, true>>(dim3(grid), dim3(256), lds, stream, a)
                                            : launch_lds<fa2_extend_split_kernel<D, PAGED, EB, false>>(dim3(grid), dim3(256), lds, stream, a);
    if (e != hipSuccess || a.n_splits == 1) return e;
    const size_t threads = (size_t)a.B * a.Hq * a.Nq * (D / 4);
    hipLaunchKernelGGL(fa2_decode_combine_kernel<D>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <int D>
static hipError_t extend_launch(const DecodeArgs& a, hipStream_t stream)
{
    if (a.kv_fp8) return a.block_table ? extend_launch<D, true, 1>(a, stream) : extend_launch<D, false, 1>(a, stream);
    return a.block_table ? extend_launch<D, true, 2>(a, stream) : extend_launch<D, false, 2>(a, stream);
}

hipError_t launch_extend(const DecodeArgs& a, int d, hipStream_t stream)
{
    if (a.n_splits < 1 || a.n_splits > kDecodeMaxSplits || a.Hkv < 1 || a.Hq % a.Hkv || a.Nq < 1) return hipErrorInvalidValue;
    if (a.window_left >= 0 && !a.causal) return hipErrorInvalidValue;      // the window is a causal one
    const long long M = (long long)(a.Hq / a.Hkv) * a.Nq, rows = (long long)a.B * a.Hq * a.Nq;
    if (M > 0x7fffffffLL - kExtendRows || rows > 0x7fffffffLL) return hipErrorInvalidValue;
    if ((long long)a.B * a.Hkv * ((M + kExtendRows - 1) / kExtendRows) > 0x7fffffffLL / a.n_splits) return hipErrorInvalidValue;
    if (rows * (d / 4) > 0x7fffffffLL * 256) return hipErrorInvalidValue;      // the combine's grid
    if (a.block_table && (a.n_pages < 1 || a.max_pages < 1 || a.page_size < kDecodeTile || a.page_size % kDecodeTile ||
                          (long long)a.max_pages * a.page_size != a.Ncap))
        return hipErrorInvalidValue;
    if (d == 128) return extend_launch<128>(a, stream);
    if (d == 64) return extend_launch<64>(a, stream);
    return hipErrorInvalidValue;
}

// ---- ragged extend (fa2_forward_extend_ragged / _paged, include/fa2_extend_ragged_mi355x.h): extend_ragged_split_body
template <int D, bool PAGED, int EB, bool WIN>
__global__ void __launch_bounds__(256) fa2_extend_ragged_split_kernel(ExtendRaggedArgs x)
{
    extend_ragged_split_body<D, PAGED, EB, WIN>(x);
}

// fa2_decode_combine_kernel's arithmetic on the flat rows [T][Hq] (nq = 1: the sink's index is the head), over the rows of the
// tokens the plan owns: a token of no sequence has no partials and keeps what O and L held
template <int D>
__global__ void __launch_bounds__(256) fa2_extend_ragged_combine_kernel(ExtendRaggedArgs x)
{
    constexpr int C4 = D / 4;
    const DecodeArgs& a = x.a;
    const dec_const_int* const plan = (const dec_const_int*)x.plan;
    if (plan[0] != a.B || plan[1] != a.Hq / a.Hkv || plan[2] != x.T) return;
    const int t0 = min(max(plan[4], 0), x.T), t1 = min(max(plan[5], 0), x.T);
    const size_t R = (size_t)x.T * a.Hq;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = t / C4;
    const int c4 = (int)(t % C4);
    if (row < (size_t)t0 * a.Hq || row >= (size_t)t1 * a.Hq) return;
#define DEC_NQ 1
#include "fa2_decode_combine.inc"
}

// The plan (fa2_launch.h), one workgroup: c_i = clamp(max(cu[0 .. i]), 0, T) for i = 0 .. B -- a running maximum, so whatever
// cu holds the sequences tile [c_0, c_B) in order -- then (start_b, q_b) = (c_b, c_{b+1} - c_b) and, behind a prefix sum of
// ceil(G q_b / kExtendRows), the sequence's work items.  A thread owns a run of ceil(B / 256) consecutive sequences; the two
// scans across threads go through LDS.  Not a hot path: one launch per step, whatever the number of layers.
__global__ void __launch_bounds__(256) fa2_extend_ragged_plan_kernel(const int* cu, int B, int G, int T, int max_blocks, int* plan)
{
    __shared__ int s_red[256];
    const int tid = threadIdx.x;
    const int C = (B + 255) / 256;
    const int b0 = (int)min((long long)tid * C, (long long)B), b1 = (int)min((long long)b0 + C, (long long)B);
    int* const seq = plan + kRaggedPlanHeader;
    int* const items = seq + 2 * (size_t)B;

    int lm = cu[0];
    for (int b = b0; b < b1; ++b) lm = max(lm, cu[b + 1]);
    s_red[tid] = lm;
    __syncthreads();
    int run = cu[0];
    for (int u = 0; u < tid; ++u) run = max(run, s_red[u]);
    int last = cu[0];      // the maximum of all of cu: c_B before the clamp
    for (int u = 0; u < 256; ++u) last = max(last, s_red[u]);
    int nb = 0;
    for (int b = b0; b < b1; ++b) {
        const int c0 = min(max(run, 0), T);
        run = max(run, cu[b + 1]);
        const int q = min(max(run, 0), T) - c0;
        seq[2 * (size_t)b] = c0;
        seq[2 * (size_t)b + 1] = q;
        nb += (G * q + kExtendRows - 1) / kExtendRows;      // G q <= G T, which the host checked
    }
    __syncthreads();      // every thread has read the maxima
    s_red[tid] = nb;
    __syncthreads();
    int at = 0, total = 0;
    for (int u = 0; u < 256; ++u) {
        if (u < tid) at += s_red[u];
        total += s_red[u];
    }
    for (int b = b0; b < b1; ++b) {
        const int n = (G * seq[2 * (size_t)b + 1] + kExtendRows - 1) / kExtendRows;      // (the thread's own store)
        for (int j = 0; j < n; ++j, ++at)
            if (at < max_blocks) { items[2 * (size_t)at] = b; items[2 * (size_t)at + 1] = j; }      // (always: total <= max_blocks)
    }
    for (int i = min(total, max_blocks) + tid; i < max_blocks; i += 256) { items[2 * (size_t)i] = -1; items[2 * (size_t)i + 1] = 0; }
    if (tid == 0) {
        plan[0] = B; plan[1] = G; plan[2] = T; plan[3] = min(total, max_blocks);
        plan[4] = min(max(cu[0], 0), T); plan[5] = min(max(last, 0), T);
        plan[6] = 0; plan[7] = 0;
    }
}

long long extend_ragged_max_blocks(int B, int H_q, int H_kv, int total_q)
{
    return (long long)(H_q / H_kv) * total_q / kExtendRows + std::min(B, total_q);
}

hipError_t launch_extend_ragged_plan(const int* cu_seqlens_q, int B, int G, int T, int* plan, hipStream_t stream)
{
    if (B < 1 || G < 1 || T < 1 || (long long)G * T > 0x7fffffffLL - kExtendRows) return hipErrorInvalidValue;
    const long long mb = (long long)G * T / kExtendRows + std::min(B, T);
    if (mb > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fa2_extend_ragged_plan_kernel, dim3(1), dim3(256), 0, stream, cu_seqlens_q, B, G, T, (int)mb, plan);
    return hipGetLastError();
}

template <int D, bool PAGED, int EB>
static hipError_t extend_ragged_launch(const ExtendRaggedArgs& x, hipStream_t stream)
{
    constexpr int lds = kDecWaves * 32 * (D + 4) * 4 + kDecWaves * 32 * 2 * 4;      // extend_launch's
    const unsigned grid = (unsigned)x.max_blocks * x.a.Hkv * x.a.n_splits;
    const hipError_t e = x.a.window_left >= 0
                             ? launch_lds<fa2_extend_ragged_split_kernel<D, PAGED, EB, true>>(dim3(grid), dim3(256), lds, stream, x)
                             : launch_lds<fa2_extend_ragged_split_kernel<D, PAGED, EB, false>>(dim3(grid), dim3(256), lds, stream, x);
    if (e != hipSuccess || x.a.n_splits == 1) return e;
    const size_t threads = (size_t)x.T * x.a.Hq * (D / 4);
    hipLaunchKernelGGL(fa2_extend_ragged_combine_kernel<D>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, x);
    return hipGetLastError();
}

template <int D>
static hipError_t extend_ragged_launch(const ExtendRaggedArgs& x, hipStream_t stream)
{
    if (x.a.kv_fp8) return x.a.block_table ? extend_ragged_launch<D, true, 1>(x, stream) : extend_ragged_launch<D, false, 1>(x, stream);
    return x.a.block_table ? extend_ragged_launch<D, true, 2>(x, stream) : extend_ragged_launch<D, false, 2>(x, stream);
}

hipError_t launch_extend_ragged(const ExtendRaggedArgs& x, int d, hipStream_t stream)
{
    const DecodeArgs& a = x.a;
    if (a.n_splits < 1 || a.n_splits > kDecodeMaxSplits || a.B < 1 || a.Hkv < 1 || a.Hq % a.Hkv || x.T < 1 || !x.plan) return hipErrorInvalidValue;
    if (a.window_left >= 0 && !a.causal) return hipErrorInvalidValue;      // the window is a causal one
    if ((long long)x.T * a.Hq > 0x7fffffffLL - kExtendRows || x.q_stride < (long long)a.Hq * d || x.q_stride % 8) return hipErrorInvalidValue;
    if (x.max_blocks != extend_ragged_max_blocks(a.B, a.Hq, a.Hkv, x.T)) return hipErrorInvalidValue;
    if ((long long)x.max_blocks * a.Hkv > 0x7fffffffLL / a.n_splits) return hipErrorInvalidValue;
    if ((long long)x.T * a.Hq * (d / 4) > 0x7fffffffLL * 256) return hipErrorInvalidValue;      // the combine's grid
    if (a.block_table && (a.n_pages < 1 || a.max_pages < 1 || a.page_size < kDecodeTile || a.page_size % kDecodeTile ||
                          (long long)a.max_pages * a.page_size != a.Ncap))
        return hipErrorInvalidValue;
    if (d == 128) return extend_ragged_launch<128>(x, stream);
    if (d == 64) return extend_ragged_launch<64>(x, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_decode(const DecodeArgs& a, int d, hipStream_t stream)
{
    if (a.n_splits < 1 || a.n_splits > kDecodeMaxSplits || a.Hq % a.Hkv || a.Hq / a.Hkv * a.Nq > kDecodeMaxRows)
        return hipErrorInvalidValue;
    if (a.window_left >= 0 && !a.causal) return hipErrorInvalidValue;      // the window is a causal one
    if ((long long)a.B * a.Hkv * a.n_splits > 0x7fffffffLL) return hipErrorInvalidValue;
    if (a.block_table && (a.n_pages < 1 || a.max_pages < 1 || a.page_size < kDecodeTile || a.page_size % kDecodeTile ||
                          (long long)a.max_pages * a.page_size != a.Ncap))
        return hipErrorInvalidValue;
    if (d == 128) return decode_launch<128>(a, stream);
    if (d == 64) return decode_launch<64>(a, stream);
    return hipErrorInvalidValue;
}

}  // namespace fa2
