// fa2_mla_decode.hip -- MLA decode attention over a 576-wide latent KV cache (fa2_forward_mla_decode / _paged,
// include/fa2_mla_mi355x.h): multi-query attention in which a token has ONE cache row, 512 latent columns followed by 64 rotary
// columns; the score uses all 576, the value is the first 512 of the same row.  Kernels, launchers and the C entry points.
//
// WORK SPLIT.  One workgroup (four waves) = one (sequence, block of 32 rows of the sequence's [M = H N_q] slab, key split).  Split
// s covers keys [s chunk, min((s + 1) chunk, len_b)), chunk = roundup(ceil(len_b / n_splits), 32), computed here from len_b.
// The four waves split the cache row by COLUMNS, not the keys by tile: wave w owns latent columns [128 w, 128 w + 128) and rotary
// columns [512 + 16 w, +16), 9 of the 36 k-steps of the score, and the same 128 columns of O.  Every cache byte is loaded once per
// workgroup, into registers, and serves both products.
// DATA PATH per 32-key tile, wave w:
//   loads        lane (key r, half h) holds 16 bytes of its row per k-step: 9 loads, straight from global memory into VGPRs
//                through a buffer resource that ends at the split's last key (rows past it read as zeros, whatever they hold);
//   S^T partial  9 MFMAs, A = those registers, B = the wave's Q^T fragments (36 VGPRs, loaded once, rows >= M zero);
//   exchange     the four partials (4 KiB each) go through a double-buffered LDS exchange, one barrier per tile; every wave adds
//                them in wave order 0..3, so all four hold the same bits of S and run the same online softmax (the decode's:
//                log2 units, lane = row, one permlane32_swap, masked P selected to 0): m, l and P need no further exchange;
//   O^T += V^T P^T  the 8 latent registers are written into the wave's private swizzled 8 KiB image (lds_off<128>: the d = 128
//                decode's V image) and read back with ds_read_b64_tr_b16; P^T is the bf16-rounded accumulator as the B operand:
//                8 MFMAs into the wave's 64 VGPRs of O^T.
// The loads of the next PF tiles are issued behind the first product.  The tile loop's bound is workgroup-uniform (every wave
// meets every barrier); an empty split returns before the first barrier.
// RESULT.  No merge of O across waves: each wave normalises and emits its 128 columns.  n_splits == 1: O (bf16) and L.
// Otherwise an fp32 partial per (split, row), O_s [512] and L_s (-inf without a visible key), folded by fa2_mla_combine_kernel in
// ascending s with ONE rounding to bf16 (fa2_decode_combine.inc's arithmetic at D = 512, without the sink).
// PAGED: the same body with one resource per tile; the tile's table entry is a scalar load one tile ahead of the loads that need
// it, clamped to [0, n_pages) before it becomes an address.
//
// E4M3 LATENT CACHES (fa2_forward_mla_decode_fp8kv / _paged_fp8kv, include/fa2_mla_fp8_mi355x.h): the same body at EB = 1.  A row
// is 640 bytes, 512 e4m3 codes then the 64 rotary columns in bf16, with ONE fp32 descale per cache read on the device (NULL: 1).
// Work split, table walk, exchange, softmax, emit and combine are the ones above; what changes is a wave's slice of a tile:
//   loads        wave w owns latent bytes [128 w, +128) and rotary bytes [512 + 32 w, +32): lane (key r, half h) issues FOUR
//                16-byte loads of codes (load j: bytes 128 w + 32 j + 16 h ..+16) and the rotary load: 5 loads, 20 VGPRs a tile.
//                The prefetch slots keep the raw codes, so kMlaPF8 tiles are in flight where the bf16 body keeps two;
//   widening     a 16-byte load holds the elements of TWO k-steps (low eight codes: k-step 2 j, high eight: 2 j + 1), widened
//                to bf16 in VGPRs (exact).  Q^T's fragment of k-step 2 j + u is Q[rho][128 w + 32 j + 16 h + 8 u ..+8];
//   score        two accumulators, latent (8 MFMAs) and rotary (1 MFMA); what enters the exchange is descale x s_latent +
//                s_rotary in fp32.  Q is not rescaled: that would round it a second time;
//   value        the widened chunk of (load j, half h, sub-step u) is chunk 4 j + 2 h + u of row r of the wave's V image.  Every
//                ds_write_b128 still has 16 consecutive rows and ONE chunk per 16-lane group, as the bf16 body's chunk 2 t + h
//                has: lds_off<128>'s XOR takes 16 different values on them, 16 different slots of the 256-byte bank row --
//                conflict-free, which chunk it is does not enter.  The image and its transposed reads are the bf16 ones;
//   epilogue     descale multiplies the fp32 row piece once, behind 1 / l, before anything is rounded.
#include "fa2_mla_mi355x.h"
#include "fa2_mla_fp8_mi355x.h"
#include "fa2_mla_sparse_mi355x.h"
#include "fa2_common.h"
#include "fa2_launch.h"

#include <algorithm>

namespace fa2 {

namespace {

constexpr float kMlaLn2 = 0.6931471805599453f;
constexpr int kMlaLatent = 512, kMlaRope = 64;      // the one accepted (kv_lora_rank, rope_dim)
constexpr int kMlaRow = kMlaLatent + kMlaRope;      // elements of a cache row and of a Q row
constexpr int kMlaRowB = 2 * kMlaRow;               // bytes of a cache row
constexpr int kMlaRowB8 = kMlaLatent + 2 * kMlaRope;      // ... of one with e4m3 latent columns: 640
constexpr int kMlaPF8 = 4;                          // tiles in flight over such a cache (20 VGPRs each): from the register report, not tuned
constexpr int kMlaTile = kDecodeTile;               // keys of a tile, rows of a block, and what a split's first key is a multiple of
constexpr int kMlaWaves = 4;
constexpr int kMlaKS = kMlaRow / 16 / kMlaWaves;    // 9 k-steps of a wave: 8 latent, 1 rotary
constexpr int kMlaVimg = kMlaTile * 256;            // a wave's V image: 32 keys x 128 columns
constexpr int kMlaXbuf = kMlaWaves * kMlaTile * 32 * 4;      // one exchange buffer: four partial S^T
constexpr int kMlaLds = kMlaWaves * kMlaVimg + 2 * kMlaXbuf;      // 64 KiB
constexpr int kMlaC4 = kMlaLatent / 4;
constexpr int kMlaCombineBatch = 8;                 // partials of a row in flight in the combine
typedef __attribute__((address_space(3))) bf16x4 mla_lds_bf16x4;
typedef __attribute__((address_space(4))) int mla_const_int;

struct MlaArgs {
    const void* Q; const void* C; const int* seqlens; const int* block_table;
    void* O; float* L; float* wsO; float* wsL;      // partials: wsO [n_splits][B M][512], wsL [n_splits][B M]
    int B, H, Nq, Ncap, n_splits;
    float scale;
    int causal;
    int n_pages, page_size, max_pages;               // paged: C is [n_pages][page_size][576], Ncap = max_pages page_size
    const float* descale;                            // e4m3 latent columns: the cache holds x / *descale (DEVICE; NULL: 1)
    const int* indices; int topk;                    // sparse: [B][Nq][topk] logical key positions, one row for all heads of a token
};

// (a copy of fa2_decode.hip's: that file's helpers sit in its anonymous namespace and its device code is left alone)
__device__ __forceinline__ bf16x4 mla_bf16x4(const f32x4& v)
{
    bf16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (__bf16)v[e];
    return r;
}

// (fa2_decode.hip's, copied for the same reason) eight OCP e4m3 codes, two words of ascending bytes, as their bf16 values
__device__ __forceinline__ bf16x8 mla_e4m3x8_to_bf16(uint32_t w0, uint32_t w1)
{
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// the tile's visibility predicate over consecutive keys: positions [0, kmax) of the lane's row
#define MLA_VISIBLE(e) (MLA_KB + acc_row(e, h) < kmax)

// PF: tiles in flight ahead of the arithmetic (36 VGPRs each; 20 at EB = 1).  EB: bytes per latent element, 2 (bf16) or 1 (e4m3).
template <bool PAGED, int PF, int EB = 2>
__device__ __forceinline__ void mla_split_body(const MlaArgs& a)
{
    static_assert(EB == 1 || EB == 2, "bf16 or e4m3 latent columns");
    static_assert(EB == 1 || PF == 1 || PF == 2, "one or two slots");
    constexpr int ROWB = EB == 2 ? kMlaRowB : kMlaRowB8;      // bytes of a cache row
    constexpr int NL = EB == 2 ? kMlaKS : 5;                  // 16-byte loads of a lane per tile, the last one the rotary columns
    extern __shared__ __attribute__((aligned(16))) char smem[];      // kMlaWaves V images | two exchange buffers

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = a.H * a.Nq;
    const int RB = (M + kMlaTile - 1) / kMlaTile;      // row blocks of a sequence
    const int bid = blockIdx.x;
    const int split = bid % a.n_splits, rb0 = bid / a.n_splits % RB * kMlaTile, b = bid / (a.n_splits * RB);
    const int Mb = min(M - rb0, kMlaTile);             // the block's live rows

    // the clamp is the contract: nothing below sees the stored value
    int len = a.Ncap;
    if (a.seqlens) len = min(max(__builtin_amdgcn_readfirstlane(a.seqlens[b]), 0), a.Ncap);
    const int per = (len + a.n_splits - 1) / a.n_splits;
    const int chunk = (per + kMlaTile - 1) / kMlaTile * kMlaTile;
    const int begin = split * chunk;                   // <= len + n_splits kMlaTile: no overflow
    const int end = min(begin + chunk, len);

    const size_t R = (size_t)a.B * M;                  // rows of O, L and of one split's partials
    const size_t row0 = (size_t)b * M;                 // the sequence's first row

    // what a finished row piece becomes: a partial, or the result
    const auto emit = [&](int row, int c4, f32x4 o, float Lrow) {
        const size_t gr = row0 + row;
        if (a.n_splits > 1) {
            *reinterpret_cast<f32x4*>(a.wsO + ((size_t)split * R + gr) * kMlaLatent + 4 * c4) = o;
            if (c4 == 0) a.wsL[(size_t)split * R + gr] = Lrow;
        } else {
            *reinterpret_cast<bf16x4*>((__bf16*)a.O + gr * kMlaLatent + 4 * c4) = mla_bf16x4(o);
            if (c4 == 0) a.L[gr] = Lrow;
        }
    };

    if (begin >= end) {      // an empty split (a short sequence's later splits, len = 0): no key, and no barrier met
        for (int idx = tid; idx < Mb * kMlaC4; idx += 256) emit(rb0 + idx / kMlaC4, idx % kMlaC4, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, -INFINITY);
        return;
    }

    // Q^T fragments of the wave's columns: lane (row r, half h) holds Q[rho][col_t + 8 h ..+8], col_t = 128 w + 16 t, 512 + 16 w
    // (EB = 1: the latent k-step t = 2 j + u takes the columns its half of load j holds, 128 w + 32 j + 16 h + 8 u ..+8)
    const int rho = rb0 + r;
    bf16x8 q[kMlaKS];
    {
        const __bf16* Qg = (const __bf16*)a.Q + (row0 + (rho < M ? rho : 0)) * kMlaRow + 8 * h;
#pragma unroll
        for (int t = 0; t < kMlaKS; ++t) {
            if constexpr (EB == 2) q[t] = *reinterpret_cast<const bf16x8*>(Qg + (t < 8 ? 128 * wave + 16 * t : kMlaLatent + 16 * wave));
            else q[t] = *reinterpret_cast<const bf16x8*>(Qg + (t < 8 ? 128 * wave + 32 * (t / 2) + 8 * h + 8 * (t % 2) : kMlaLatent + 16 * wave));
            if (rho >= M) q[t] = bf16x8{};
        }
    }
    // keys [0, kmax) are visible to this lane's row (bottom-right causal: j <= i + len - N_q), none to a padding row
    int kmax = end;
    if (a.causal) kmax = min(end, rho % a.Nq + len - a.Nq + 1);
    if (rho >= M) kmax = 0;

    const auto c_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.C + (PAGED ? 0 : (size_t)b * a.Ncap * ROWB)), 0,
                                                          PAGED ? 0 : end * ROWB, 0x00020000);
    // the lane's 16 bytes of latent load t (a k-step; two at EB = 1): + 32 t below the rotary load
    const uint32_t koff = (uint32_t)r * ROWB + 128 * EB * wave + 16 * h, roff = (uint32_t)r * ROWB + EB * kMlaLatent + 32 * wave + 16 * h;
    u32x4 kf[PF][NL];
    // PAGED: fa2_decode.hip's table walk with every wave on every tile.  (pg_i, pg_o): page index and row within the page of the
    // tile whose entry is fetched next; (ent, ent_o): the fetched entry and row of the tile that is LOADED next.  A tile with a
    // key indexes the table below max_pages (kb < len <= max_pages page_size); one without reads entry 0 of its sequence, which
    // the clamp and its resource of no rows keep from being used.  Read through the constant address space: a scalar load.
    int pg_i = 0, pg_o = 0, ent = 0, ent_o = 0;
    const mla_const_int* const table = (const mla_const_int*)a.block_table + (size_t)b * a.max_pages;
    const auto fetch_entry = [&](int base) {
        ent = __builtin_amdgcn_readfirstlane(table[__builtin_amdgcn_readfirstlane(base < end ? pg_i : 0)]);
        ent_o = pg_o;
        pg_o += kMlaTile;
        if (pg_o >= a.page_size) { pg_o -= a.page_size; ++pg_i; }
    };
    const auto load_tile = [&](int base, int sl) {      // rows past `end` read as zeros (and cost no traffic)
        if constexpr (PAGED) {
            const int page = base < end ? min(max(ent, 0), a.n_pages - 1) : 0;      // the clamp is the contract
            const int rows = __builtin_amdgcn_readfirstlane(max(min(kMlaTile, end - base), 0));
            const size_t at = ((size_t)page * a.page_size + ent_o) * ROWB;      // 64-bit: a pool may exceed 4 GiB
            const auto cp = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.C + at), 0, rows * ROWB, 0x00020000);
#pragma unroll
            for (int t = 0; t < NL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(cp, t < NL - 1 ? koff + 32 * t : roff, 0, 0);
            return;
        }
        const uint32_t b0 = (uint32_t)base * ROWB;
#pragma unroll
        for (int t = 0; t < NL; ++t) kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(c_rsrc, b0 + (t < NL - 1 ? koff + 32 * t : roff), 0, 0);
    };

    char* const vimg = smem + wave * kMlaVimg;
    // ds_read_b64_tr_b16: lane 4 qq + p of a 16-lane group supplies row qq, columns 4 p ..+4 of a 4 x 16 block; the group's lanes
    // get the block's columns.  Group g serves half g >> 1 and columns 16 (g & 1) ..+16 of a 32-column tile of V.
    const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, c0 = 16 * ((lane >> 4) & 1);

    float m = -INFINITY, l = 0.0f;              // running maximum (log2 units) and this lane half's part of the running sum
    f32x16 o[4];                                // O^T [128 w + 32 c ..+32][32 rows]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[c][e] = 0.0f;
    const float sc = a.scale * kLog2e;
    // the cache's descale: a scalar load, here and not on the host, so that a captured graph sees the value of its replay
    float ds = 1.0f;
    if constexpr (EB == 1)
        if (a.descale) ds = __uint_as_float(__builtin_amdgcn_readfirstlane(*(const mla_const_int*)a.descale));

    int kb = begin;
    if constexpr (PAGED) {      // the one division of a workgroup
        pg_i = kb / a.page_size;
        pg_o = kb - pg_i * a.page_size;
        fetch_entry(kb);
    }
    load_tile(kb, 0);
    if constexpr (PAGED) fetch_entry(kb + kMlaTile);
    if constexpr (EB == 2) {
    if constexpr (PF == 2) {
        load_tile(kb + kMlaTile, 1);
        if constexpr (PAGED) fetch_entry(kb + 2 * kMlaTile);
    }
    // two tiles per round: the exchange buffers alternate, and with PF = 2 so do the slots.  begin and end are the workgroup's.
    for (; kb < end; kb += 2 * kMlaTile) {
        {
#define MLA_KB kb
#define MLA_SL 0
#define MLA_XB 0
#include "fa2_mla_decode_tile.inc"
        }
        if (kb + kMlaTile < end) {
#define MLA_KB (kb + kMlaTile)
#define MLA_SL (PF - 1)
#define MLA_XB 1
#include "fa2_mla_decode_tile.inc"
        }
    }
    } else {
        // PF tiles in flight and a round of ROUND tiles, a multiple of PF and of the two exchange buffers, unrolled: slot i % PF
        // and buffer i & 1 are constants of the text.  A tile past `end` loads nothing (its resource has no rows there).
        constexpr int ROUND = PF % 2 ? 2 * PF : PF;
#pragma unroll
        for (int i = 1; i < PF; ++i) {
            load_tile(kb + i * kMlaTile, i);
            if constexpr (PAGED) fetch_entry(kb + (i + 1) * kMlaTile);
        }
        for (; kb < end; kb += ROUND * kMlaTile) {
#pragma unroll
            for (int i = 0; i < ROUND; ++i) {
                if (kb + i * kMlaTile < end) {
#define MLA_KB (kb + i * kMlaTile)
#define MLA_SL (i % PF)
#define MLA_XB (i & 1)
#include "fa2_mla_decode_tile.inc"
                }
            }
        }
    }

    // every wave holds the same m and l: it normalises and emits its own 128 columns (registers 4 g4 ..+4 of tile c are columns
    // 32 c + 8 g4 + 4 h ..+4 of row rho)
    l = half_sum(l);
    const bool has = l > 0.0f;                  // a select: a row without a visible key in this split
    const float inv = 1.0f / l;
    const float Lrow = has ? (m + __builtin_amdgcn_logf(l)) * kMlaLn2 : -INFINITY;      // (v_log_f32 is log2)
    if (rho < M) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = has ? (EB == 2 ? o[c][4 * g4 + e] * inv : o[c][4 * g4 + e] * inv * ds) : 0.0f;
                emit(rho, 32 * wave + 8 * c + 2 * g4 + h, v, Lrow);
            }
    }
}
#undef MLA_VISIBLE

// SPARSE (fa2_forward_mla_decode_sparse / _paged): the rows of a tile are the cache rows that 32 consecutive SLOTS of the token's
// index row name.  Loads and the index pipeline are this body's; from the first product on a tile is fa2_mla_decode_tile.inc.
// One workgroup = (sequence b, query token i, block of 32 heads, split of the slot list): the index row belongs to the token, so
// a row block never mixes tokens.  bit r of a tile's live mask: slot t0 + r names a live key (workgroup-uniform: every wave
// ballots the same 32 indices).
#define MLA_VISIBLE(e) ((vis >> acc_row(e, 0)) & 1u)

template <bool PAGED, int EB = 2>      // EB: the tile text's; bf16 rows only here
__device__ __forceinline__ void mla_sparse_body(const MlaArgs& a)
{
    static_assert(EB == 2, "bf16 latent columns");
    // tiles of ROWS in flight ahead of the arithmetic, 36 VGPRs each as in mla_split_body<., 2>: what the register report leaves
    // at two workgroups per CU.  The depth, and the distances of the index and table fetches below, are UNTUNED: nothing of this
    // pipeline has been measured against another depth.
    constexpr int PF = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // kMlaWaves V images | two exchange buffers

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HB = (a.H + kMlaTile - 1) / kMlaTile;    // head blocks of a token
    const int bid = blockIdx.x;
    const int split = bid % a.n_splits, hb0 = bid / a.n_splits % HB * kMlaTile, tok = bid / (a.n_splits * HB);
    const int b = tok / a.Nq, i = tok - b * a.Nq;
    const int Hb = min(a.H - hb0, kMlaTile);           // the block's live heads

    int len = a.Ncap;                                  // the clamp is the contract
    if (a.seqlens) len = min(max(__builtin_amdgcn_readfirstlane(a.seqlens[b]), 0), a.Ncap);
    // index j is live iff 0 <= j < jmax (bottom-right causal: j <= i + len - N_q)
    const int jmax = a.causal ? min(len, i + len - a.Nq + 1) : len;
    // the split's slots: host values only
    const int per = (a.topk + a.n_splits - 1) / a.n_splits;
    const int chunk = (per + kMlaTile - 1) / kMlaTile * kMlaTile;
    const int begin = split * chunk;                   // <= topk + n_splits kMlaTile: no overflow
    const int end = min(begin + chunk, a.topk);

    const size_t R = (size_t)a.B * a.H * a.Nq;         // rows of O, L and of one split's partials
    // (mla_split_body's emit at this body's rows: a shared function moved the dense kernels' registers)
    const auto emit = [&](int head, int c4, f32x4 o, float Lrow) {
        const size_t gr = ((size_t)b * a.H + head) * a.Nq + i;
        if (a.n_splits > 1) {
            *reinterpret_cast<f32x4*>(a.wsO + ((size_t)split * R + gr) * kMlaLatent + 4 * c4) = o;
            if (c4 == 0) a.wsL[(size_t)split * R + gr] = Lrow;
        } else {
            *reinterpret_cast<bf16x4*>((__bf16*)a.O + gr * kMlaLatent + 4 * c4) = mla_bf16x4(o);
            if (c4 == 0) a.L[gr] = Lrow;
        }
    };

    if (begin >= end || jmax <= 0) {      // no slot, or no index can be live: workgroup-uniform, and no barrier met
        for (int idx = tid; idx < Hb * kMlaC4; idx += 256) emit(hb0 + idx / kMlaC4, idx % kMlaC4, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, -INFINITY);
        return;
    }

    // Q^T fragments as in mla_split_body: lane (row r, half h) holds Q[b][head][i][col_t + 8 h ..+8]; heads >= H are zero
    const int head = hb0 + r;
    bf16x8 q[kMlaKS];
    {
        const __bf16* Qg = (const __bf16*)a.Q + (((size_t)b * a.H + (head < a.H ? head : 0)) * a.Nq + i) * kMlaRow + 8 * h;
#pragma unroll
        for (int t = 0; t < kMlaKS; ++t) {
            q[t] = *reinterpret_cast<const bf16x8*>(Qg + (t < 8 ? 128 * wave + 16 * t : kMlaLatent + 16 * wave));
            if (head >= a.H) q[t] = bf16x8{};
        }
    }

    // contiguous: one resource per sequence, ending at len rows; a dead slot's offset lies past every resource (zeros, no traffic)
    const auto c_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)a.C + (PAGED ? 0 : (size_t)b * a.Ncap * kMlaRowB)), 0,
                                                          PAGED ? 0 : len * kMlaRowB, 0x00020000);
    const uint32_t kcol = 256 * wave + 16 * h, rcol = 2 * kMlaLatent + 32 * wave + 16 * h;      // the lane's bytes within a row
    u32x4 kf[PF][kMlaKS];
    uint32_t msk[PF];      // the live masks of the tiles in the slots

    // INDEX PIPELINE.  Lane r (of both halves, of every wave) owns slot t0 + r of a tile.  With tile k in the first product:
    //   j_a = index of tile k + 2 (its rows are loaded now), j_b = index of tile k + 3, and the index of tile k + 4 is fetched;
    //   paged: (ent, rem) = table entry and row within the page of tile k + 2, fetched one tile ago; fetch_entry then fetches
    //   those of tile k + 3 from j_b.
    // So an index is two tiles old when a table entry or a row address is made of it and a table entry one tile old: no tile
    // waits on an index or table load it issued itself.  The index fetch stands ahead of the row loads so that waiting for it
    // (vmcnt counts in order) does not wait for them.
    const int* const idx = a.indices + ((size_t)b * a.Nq + i) * a.topk;
    // a slot past the split's last is dead; its lane re-reads the last slot (an unconditional load: a load that a branch may
    // skip makes every later wait count a guess, and the compiler then waits for everything)
    const auto fetch_index = [&](int t0) {
        const int t = t0 + r, v = idx[min(t, end - 1)];
        return t < end ? v : -1;
    };
    const auto is_live = [&](int j) { return (uint32_t)j < (uint32_t)jmax; };      // jmax > 0 here
    int j_a = fetch_index(begin), j_b = fetch_index(begin + kMlaTile);
    int ent = 0, rem = 0;
    const int* const table = a.block_table + (size_t)b * a.max_pages;
    const auto fetch_entry = [&](int) {                // PAGED only: of the tile j_a names, for live lanes only
        const uint32_t pg = (uint32_t)j_a / (uint32_t)a.page_size;      // < max_pages for a live j
        rem = j_a - (int)pg * a.page_size;
        ent = is_live(j_a) ? table[pg] : 0;
    };
    const auto load_tile = [&](int base, int sl) {
        const int j_n = fetch_index(base + 2 * kMlaTile);
        const bool live = is_live(j_a);
        msk[sl] = (uint32_t)__builtin_amdgcn_ballot_w64(live);      // both halves hold the same 32 bits
        if constexpr (PAGED) {
            // up to 32 pages a tile: a 64-bit address per lane (a pool may exceed 4 GiB), the loads under the live predicate
            const int page = min(max(ent, 0), a.n_pages - 1);       // the clamp is the contract
            const char* const row = (const char*)a.C + ((size_t)page * a.page_size + rem) * kMlaRowB;
#pragma unroll
            for (int t = 0; t < kMlaKS; ++t) kf[sl][t] = u32x4{0, 0, 0, 0};
            if (live) {
#pragma unroll
                for (int t = 0; t < kMlaKS; ++t)
                    kf[sl][t] = *reinterpret_cast<const u32x4*>(row + (t < kMlaKS - 1 ? kcol + 32 * t : rcol));
            }
        } else {
            const uint32_t at = live ? (uint32_t)j_a * kMlaRowB : 0x80000000u;      // a resource has at most INT_MAX bytes
#pragma unroll
            for (int t = 0; t < kMlaKS; ++t)
                kf[sl][t] = __builtin_amdgcn_raw_buffer_load_b128(c_rsrc, at + (t < kMlaKS - 1 ? kcol + 32 * t : rcol), 0, 0);
        }
        j_a = j_b;
        j_b = j_n;
    };

    char* const vimg = smem + wave * kMlaVimg;
    const int gi = lane & 15, qq = gi >> 2, pp = gi & 3, c0 = 16 * ((lane >> 4) & 1);      // mla_split_body's transposed reads

    float m = -INFINITY, l = 0.0f;
    f32x16 o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[c][e] = 0.0f;
    const float sc = a.scale * kLog2e;
    constexpr float ds = 1.0f;      // (the tile text's e4m3 branch names it; EB = 2 discards that branch)

    int kb = begin;                                    // a SLOT from here on
    if constexpr (PAGED) fetch_entry(kb);
    load_tile(kb, 0);
    if constexpr (PAGED) fetch_entry(kb + kMlaTile);
    load_tile(kb + kMlaTile, 1);
    if constexpr (PAGED) fetch_entry(kb + 2 * kMlaTile);
    // two tiles per round as in mla_split_body.  begin and end are host values: every wave meets every barrier
    for (; kb < end; kb += 2 * kMlaTile) {
        {
            const uint32_t vis = msk[0] >> (4 * h);
#define MLA_KB kb
#define MLA_SL 0
#define MLA_XB 0
#include "fa2_mla_decode_tile.inc"
        }
        if (kb + kMlaTile < end) {
            const uint32_t vis = msk[1] >> (4 * h);
#define MLA_KB (kb + kMlaTile)
#define MLA_SL 1
#define MLA_XB 1
#include "fa2_mla_decode_tile.inc"
        }
    }

    // mla_split_body's epilogue at this body's rows
    l = half_sum(l);
    const bool has = l > 0.0f;                  // a select: a row without a live slot in this split
    const float inv = 1.0f / l;
    const float Lrow = has ? (m + __builtin_amdgcn_logf(l)) * kMlaLn2 : -INFINITY;
    if (head < a.H) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = has ? o[c][4 * g4 + e] * inv : 0.0f;
                emit(head, 32 * wave + 8 * c + 2 * g4 + h, v, Lrow);
            }
    }
}
#undef MLA_VISIBLE

}  // namespace

template <bool PAGED>
__global__ void __launch_bounds__(256, 2) fa2_mla_decode_split_kernel(MlaArgs a)
{
    mla_split_body<PAGED, 2>(a);
}

template <bool PAGED>
__global__ void __launch_bounds__(256, 2) fa2_mla_decode_fp8_split_kernel(MlaArgs a)
{
    mla_split_body<PAGED, kMlaPF8, 1>(a);
}

template <bool PAGED>
__global__ void __launch_bounds__(256, 2) fa2_mla_decode_sparse_kernel(MlaArgs a)
{
    mla_sparse_body<PAGED>(a);
}

// rows x 128 lanes, a lane owns four columns of one row: partials in, ascending s, fp32, one rounding.  fa2_decode_combine.inc's
// arithmetic without the sink: the partials of a row are loaded kMlaCombineBatch at a time, all loads of a batch ahead of their
// use; indices past the last split are clamped and their terms selected away.
__global__ void __launch_bounds__(256) fa2_mla_combine_kernel(MlaArgs a)
{
    const size_t R = (size_t)a.B * a.H * a.Nq;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = t / kMlaC4;
    const int c4 = (int)(t % kMlaC4);
    if (row >= R) return;
    const int last = a.n_splits - 1;
    float m = -INFINITY;
    for (int s0 = 0; s0 < a.n_splits; s0 += 2 * kMlaCombineBatch) {
        float ls[2 * kMlaCombineBatch];
#pragma unroll
        for (int i = 0; i < 2 * kMlaCombineBatch; ++i) ls[i] = a.wsL[(size_t)min(s0 + i, last) * R + row];
#pragma unroll
        for (int i = 0; i < 2 * kMlaCombineBatch; ++i) m = fmaxf(m, ls[i]);
    }
    const float m0 = m == -INFINITY ? 0.0f : m;
    float sum = 0.0f;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s0 = 0; s0 < a.n_splits; s0 += kMlaCombineBatch) {
        float ls[kMlaCombineBatch];
        f32x4 os[kMlaCombineBatch];
#pragma unroll
        for (int i = 0; i < kMlaCombineBatch; ++i) {
            const size_t at = (size_t)min(s0 + i, last) * R + row;
            ls[i] = a.wsL[at];
            os[i] = *reinterpret_cast<const f32x4*>(a.wsO + at * kMlaLatent + 4 * c4);
        }
#pragma unroll
        for (int i = 0; i < kMlaCombineBatch; ++i) {
            const bool has = s0 + i <= last && ls[i] != -INFINITY;      // a select: an empty split's O_s is left out
            const float w = __builtin_amdgcn_exp2f((ls[i] - m0) * kLog2e);
            sum += has ? w : 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = has ? acc[e] + w * os[i][e] : acc[e];
        }
    }
    const bool none = m == -INFINITY;
    const float inv = 1.0f / sum;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : acc[e] * inv;
    *reinterpret_cast<bf16x4*>((__bf16*)a.O + row * kMlaLatent + 4 * c4) = mla_bf16x4(acc);
    if (c4 == 0) a.L[row] = none ? -INFINITY : m + __builtin_amdgcn_logf(sum) * kMlaLn2;
}

namespace {

inline long long mla_row_blocks(int H, int q_len) { return ((long long)H * q_len + kMlaTile - 1) / kMlaTile; }

// n_splits B H q_len (512 + 1) floats rounded up to 256 bytes; 0: it does not fit
inline size_t mla_partials_bytes(int B, int H, int q_len, int n_splits)
{
    const unsigned __int128 bytes = (unsigned __int128)n_splits * B * H * q_len * (kMlaLatent + 1) * sizeof(float);
    if (bytes > SIZE_MAX / 2) return 0;
    return ((size_t)bytes + 255) & ~(size_t)255;
}

struct MlaCall {
    const void* Q; const void* C; const int* block_table; const int* seqlens_k; void* O; float* L;
    int B, H, q_len, kv_capacity, n_pages, page_size, max_pages, kv_lora_rank, rope_dim;
    float scale;
    int causal, n_splits;
    void* ws; size_t ws_bytes; void* stream;
    const float* descale = nullptr;      // fp8 only; never read by the host
    const int* indices = nullptr; int topk = 0;      // sparse only; never read by the host
};

// fp8: the latent columns of the cache are e4m3 codes (a 640-byte row); every check and its order are shared
int mla_run(const MlaCall& c, bool paged, bool fp8 = false)
{
    if (!c.Q || !c.C || !c.O || !c.L || (paged && !c.block_table)) return FA2_ERR_NULL_POINTER;
    if (c.B <= 0 || c.H <= 0 || c.q_len <= 0 || !(c.scale > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    int kv_capacity = c.kv_capacity;
    if (paged) {
        if (c.n_pages <= 0 || c.page_size <= 0 || c.max_pages <= 0 || c.page_size % kMlaTile) return FA2_ERR_INVALID_SHAPE;
        // key indices are ints, and the kernel forms begin = split chunk <= len + n_splits kMlaTile and kb + 4 kMlaTile (the family's bound)
        if ((long long)c.max_pages * c.page_size > 0x7fffffffLL - (kDecodeMaxSplits + 2) * kDecodeKB) return FA2_ERR_INVALID_SHAPE;
        kv_capacity = c.max_pages * c.page_size;
    } else {
        if (kv_capacity <= 0) return FA2_ERR_INVALID_SHAPE;
        // one sequence, one buffer resource (a 576-wide row whatever the widths asked for: those are refused below)
        if ((long long)kv_capacity * (fp8 ? kMlaRowB8 : kMlaRowB) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    }
    if (c.n_splits < 0 || c.n_splits > kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
    if ((long long)c.B * c.H * c.q_len > 0x7fffffffLL - kMlaTile) return FA2_ERR_INVALID_SHAPE;      // the rows of O and L
    if (c.kv_lora_rank != kMlaLatent || c.rope_dim != kMlaRope) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    const int n_splits = c.n_splits ? c.n_splits : fa2_mla_decode_num_splits(c.B, c.H, c.q_len, kv_capacity, c.kv_lora_rank, c.rope_dim);
    if ((long long)c.B * mla_row_blocks(c.H, c.q_len) > 0x7fffffffLL / n_splits) return FA2_ERR_INVALID_SHAPE;
    const size_t need = n_splits > 1 ? mla_partials_bytes(c.B, c.H, c.q_len, n_splits) : 0;
    if (n_splits > 1 && !need) return FA2_ERR_INVALID_SHAPE;
    if (n_splits > 1 && (!c.ws || c.ws_bytes < need || ((uintptr_t)c.ws & 15))) return FA2_ERR_WORKSPACE;
    MlaArgs a{};
    a.Q = c.Q; a.C = c.C; a.seqlens = c.seqlens_k; a.O = c.O; a.L = c.L;
    a.wsO = (float*)c.ws;
    a.wsL = n_splits > 1 ? (float*)c.ws + (size_t)n_splits * c.B * c.H * c.q_len * kMlaLatent : nullptr;
    a.B = c.B; a.H = c.H; a.Nq = c.q_len; a.Ncap = kv_capacity; a.n_splits = n_splits;
    a.scale = c.scale; a.causal = c.causal ? 1 : 0;
    a.descale = fp8 ? c.descale : nullptr;
    if (paged) { a.block_table = c.block_table; a.n_pages = c.n_pages; a.page_size = c.page_size; a.max_pages = c.max_pages; }
    const hipStream_t stream = (hipStream_t)c.stream;
    const unsigned grid = (unsigned)(c.B * mla_row_blocks(c.H, c.q_len) * n_splits);
    hipError_t e;
    if (fp8)
        e = paged ? launch_lds<fa2_mla_decode_fp8_split_kernel<true>>(dim3(grid), dim3(256), kMlaLds, stream, a)
                  : launch_lds<fa2_mla_decode_fp8_split_kernel<false>>(dim3(grid), dim3(256), kMlaLds, stream, a);
    else
        e = paged ? launch_lds<fa2_mla_decode_split_kernel<true>>(dim3(grid), dim3(256), kMlaLds, stream, a)
                  : launch_lds<fa2_mla_decode_split_kernel<false>>(dim3(grid), dim3(256), kMlaLds, stream, a);
    if (e == hipSuccess && n_splits > 1) {
        const size_t threads = (size_t)c.B * c.H * c.q_len * kMlaC4;      // < 2^31 x 128: the grid fits
        hipLaunchKernelGGL(fa2_mla_combine_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e;
}

inline long long mla_sparse_groups(int B, int H, int q_len) { return (long long)B * q_len * ((H + kMlaTile - 1) / kMlaTile); }

// the sparse calls: mla_run's checks in mla_run's order, with indices among the pointers and topk among the shapes
int mla_sparse_run(const MlaCall& c, bool paged)
{
    if (!c.Q || !c.C || !c.indices || !c.O || !c.L || (paged && !c.block_table)) return FA2_ERR_NULL_POINTER;
    if (c.B <= 0 || c.H <= 0 || c.q_len <= 0 || c.topk <= 0 || !(c.scale > 0.0f)) return FA2_ERR_INVALID_SHAPE;
    int kv_capacity = c.kv_capacity;
    if (paged) {
        if (c.n_pages <= 0 || c.page_size <= 0 || c.max_pages <= 0 || c.page_size % kMlaTile) return FA2_ERR_INVALID_SHAPE;
        if ((long long)c.max_pages * c.page_size > 0x7fffffffLL - (kDecodeMaxSplits + 2) * kDecodeKB) return FA2_ERR_INVALID_SHAPE;
        kv_capacity = c.max_pages * c.page_size;
    } else {
        if (kv_capacity <= 0) return FA2_ERR_INVALID_SHAPE;
        if ((long long)kv_capacity * kMlaRowB > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;      // one sequence, one buffer resource
    }
    // slots are ints, and the kernel forms begin = split chunk <= topk + n_splits kMlaTile and kb + 4 kMlaTile
    if (c.topk > 0x7fffffff - (kDecodeMaxSplits + 2) * kDecodeKB) return FA2_ERR_INVALID_SHAPE;
    if (c.n_splits < 0 || c.n_splits > kDecodeMaxSplits) return FA2_ERR_INVALID_SHAPE;
    if ((long long)c.B * c.H * c.q_len > 0x7fffffffLL - kMlaTile) return FA2_ERR_INVALID_SHAPE;      // the rows of O and L
    if (c.kv_lora_rank != kMlaLatent || c.rope_dim != kMlaRope) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    const int n_splits = c.n_splits ? c.n_splits : fa2_mla_sparse_num_splits(c.B, c.H, c.q_len, c.topk, c.kv_lora_rank, c.rope_dim);
    const long long groups = mla_sparse_groups(c.B, c.H, c.q_len);
    if (groups > 0x7fffffffLL / n_splits) return FA2_ERR_INVALID_SHAPE;
    const size_t need = n_splits > 1 ? mla_partials_bytes(c.B, c.H, c.q_len, n_splits) : 0;
    if (n_splits > 1 && !need) return FA2_ERR_INVALID_SHAPE;
    if (n_splits > 1 && (!c.ws || c.ws_bytes < need || ((uintptr_t)c.ws & 15))) return FA2_ERR_WORKSPACE;
    MlaArgs a{};
    a.Q = c.Q; a.C = c.C; a.seqlens = c.seqlens_k; a.O = c.O; a.L = c.L;
    a.indices = c.indices; a.topk = c.topk;
    a.wsO = (float*)c.ws;
    a.wsL = n_splits > 1 ? (float*)c.ws + (size_t)n_splits * c.B * c.H * c.q_len * kMlaLatent : nullptr;
    a.B = c.B; a.H = c.H; a.Nq = c.q_len; a.Ncap = kv_capacity; a.n_splits = n_splits;
    a.scale = c.scale; a.causal = c.causal ? 1 : 0;
    if (paged) { a.block_table = c.block_table; a.n_pages = c.n_pages; a.page_size = c.page_size; a.max_pages = c.max_pages; }
    const hipStream_t stream = (hipStream_t)c.stream;
    const unsigned grid = (unsigned)(groups * n_splits);
    hipError_t e = paged ? launch_lds<fa2_mla_decode_sparse_kernel<true>>(dim3(grid), dim3(256), kMlaLds, stream, a)
                         : launch_lds<fa2_mla_decode_sparse_kernel<false>>(dim3(grid), dim3(256), kMlaLds, stream, a);
    if (e == hipSuccess && n_splits > 1) {      // the dense decode's combine: the partials have its layout
        const size_t threads = (size_t)c.B * c.H * c.q_len * kMlaC4;
        hipLaunchKernelGGL(fa2_mla_combine_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, a);
        e = hipGetLastError();
    }
    return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e;
}

}  // namespace
}  // namespace fa2

extern "C" {

int fa2_mla_decode_num_splits(int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim)
{
    if (B <= 0 || H <= 0 || q_len <= 0 || kv_capacity <= 0 || kv_lora_rank != fa2::kMlaLatent || rope_dim != fa2::kMlaRope) return 1;
    const long long groups = (long long)B * fa2::mla_row_blocks(H, q_len);
    const long long fill = (fa2::kDecodeCUs + groups - 1) / groups;             // smallest s with groups x s >= the CU count
    const long long room = std::max(1, kv_capacity / fa2::kDecodeMinSplitKeys);   // a split of a full cache keeps that many keys
    return (int)std::min<long long>(std::min(fill, room), fa2::kDecodeMaxSplits);
}

size_t fa2_mla_decode_workspace_bytes(int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim, int n_splits)
{
    if (B <= 0 || H <= 0 || q_len <= 0 || kv_capacity <= 0 || kv_lora_rank != fa2::kMlaLatent || rope_dim != fa2::kMlaRope) return 0;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return 0;
    if (n_splits == 0) n_splits = fa2_mla_decode_num_splits(B, H, q_len, kv_capacity, kv_lora_rank, rope_dim);
    if (n_splits == 1) return 0;
    return fa2::mla_partials_bytes(B, H, q_len, n_splits);
}

int fa2_forward_mla_decode(const void* Q, const void* ckv_cache, const int* seqlens_k, void* O, float* L,
                           int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim, float softmax_scale,
                           int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream)
{
    return fa2::mla_run({Q, ckv_cache, nullptr, seqlens_k, O, L, B, H, q_len, kv_capacity, 0, 0, 0, kv_lora_rank, rope_dim, softmax_scale,
                         causal, n_splits, workspace, workspace_bytes, stream}, false);
}

int fa2_forward_mla_decode_paged(const void* Q, const void* ckv_pages, const int* block_table, const int* seqlens_k, void* O,
                                 float* L, int B, int H, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                                 int kv_lora_rank, int rope_dim, float softmax_scale, int causal, int n_splits, void* workspace,
                                 size_t workspace_bytes, void* stream)
{
    return fa2::mla_run({Q, ckv_pages, block_table, seqlens_k, O, L, B, H, q_len, 0, n_pages, page_size, max_pages_per_seq, kv_lora_rank,
                         rope_dim, softmax_scale, causal, n_splits, workspace, workspace_bytes, stream}, true);
}

int fa2_forward_mla_decode_fp8kv(const void* Q, const void* ckv_cache, const float* latent_descale, const int* seqlens_k, void* O,
                                 float* L, int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim,
                                 float softmax_scale, int causal, int n_splits, void* workspace, size_t workspace_bytes,
                                 void* stream)
{
    return fa2::mla_run({Q, ckv_cache, nullptr, seqlens_k, O, L, B, H, q_len, kv_capacity, 0, 0, 0, kv_lora_rank, rope_dim, softmax_scale,
                         causal, n_splits, workspace, workspace_bytes, stream, latent_descale}, false, true);
}

int fa2_forward_mla_decode_paged_fp8kv(const void* Q, const void* ckv_pages, const int* block_table, const float* latent_descale,
                                       const int* seqlens_k, void* O, float* L, int B, int H, int q_len, int n_pages,
                                       int page_size, int max_pages_per_seq, int kv_lora_rank, int rope_dim, float softmax_scale,
                                       int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream)
{
    return fa2::mla_run({Q, ckv_pages, block_table, seqlens_k, O, L, B, H, q_len, 0, n_pages, page_size, max_pages_per_seq, kv_lora_rank,
                         rope_dim, softmax_scale, causal, n_splits, workspace, workspace_bytes, stream, latent_descale}, true, true);
}

int fa2_mla_sparse_num_splits(int B, int H, int q_len, int topk, int kv_lora_rank, int rope_dim)
{
    if (B <= 0 || H <= 0 || q_len <= 0 || topk <= 0 || kv_lora_rank != fa2::kMlaLatent || rope_dim != fa2::kMlaRope) return 1;
    const long long groups = fa2::mla_sparse_groups(B, H, q_len);
    const long long fill = (fa2::kDecodeCUs + groups - 1) / groups;      // smallest s with groups x s >= the CU count
    const long long room = std::max(1, topk / fa2::kDecodeMinSplitKeys);  // the family's floor, unmeasured for a gather
    return (int)std::min<long long>(std::min(fill, room), fa2::kDecodeMaxSplits);
}

size_t fa2_mla_sparse_workspace_bytes(int B, int H, int q_len, int topk, int kv_lora_rank, int rope_dim, int n_splits)
{
    if (B <= 0 || H <= 0 || q_len <= 0 || topk <= 0 || kv_lora_rank != fa2::kMlaLatent || rope_dim != fa2::kMlaRope) return 0;
    if (n_splits < 0 || n_splits > fa2::kDecodeMaxSplits) return 0;
    if (n_splits == 0) n_splits = fa2_mla_sparse_num_splits(B, H, q_len, topk, kv_lora_rank, rope_dim);
    if (n_splits == 1) return 0;
    return fa2::mla_partials_bytes(B, H, q_len, n_splits);
}

int fa2_forward_mla_decode_sparse(const void* Q, const void* ckv_cache, const int* indices, const int* seqlens_k, void* O, float* L,
                                  int B, int H, int q_len, int topk, int kv_capacity, int kv_lora_rank, int rope_dim,
                                  float softmax_scale, int causal, int n_splits, void* workspace, size_t workspace_bytes,
                                  void* stream)
{
    return fa2::mla_sparse_run({Q, ckv_cache, nullptr, seqlens_k, O, L, B, H, q_len, kv_capacity, 0, 0, 0, kv_lora_rank, rope_dim,
                                softmax_scale, causal, n_splits, workspace, workspace_bytes, stream, nullptr, indices, topk}, false);
}

int fa2_forward_mla_decode_sparse_paged(const void* Q, const void* ckv_pages, const int* block_table, const int* indices,
                                        const int* seqlens_k, void* O, float* L, int B, int H, int q_len, int topk, int n_pages,
                                        int page_size, int max_pages_per_seq, int kv_lora_rank, int rope_dim, float softmax_scale,
                                        int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream)
{
    return fa2::mla_sparse_run({Q, ckv_pages, block_table, seqlens_k, O, L, B, H, q_len, 0, n_pages, page_size, max_pages_per_seq,
                                kv_lora_rank, rope_dim, softmax_scale, causal, n_splits, workspace, workspace_bytes, stream, nullptr,
                                indices, topk}, true);
}

}  // extern "C"
