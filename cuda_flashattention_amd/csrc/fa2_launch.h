// fa2_launch.h -- host-side launcher declarations (internal; the public surface is
// include/fa2_mi355x.h).  Each launcher validates nothing: fa2_capi.cpp owns argument
// checking and status codes, the launchers only pick a template instance and enqueue it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace fa2 {

// One forward problem: BH independent [Nq, d] query slabs against [Nk, d] key/value slabs
// (BH / kv_group of them: query head h reads K/V slab h / kv_group).
// Plain attention has Nq == Nk; a ring step runs Nq local query rows against the Nk rows of
// the resident K/V shard and carries (Oacc, Lrun, Mrun) between launches.
struct FwdArgs {
    const void* Q;    // [BH][Nq][d]   bf16
    const void* K;    // [BH / kv_group][Nk][d]   bf16
    const void* V;    // [BH / kv_group][Nk][d]   bf16
    void* O;          // [BH][Nq][d]   bf16 (written when finalize != 0)
    float* L;         // [BH][Nq]      natural-log LSE when finalize, running sum l otherwise
    float* Oacc;      // [BH][Nq][d]   fp32 un-normalised accumulator (ring state) or nullptr
    float* M;         // [BH][Nq]      running max in natural (scaled) units (ring state) or nullptr
    int BH, Nq, Nk, d;
    float scale;
    int causal;       // keys j > i + causal_shift are masked
    int causal_shift; // global key index of the shard's first key minus that of the first query
    int resume;       // 1: start from (Oacc, L, M); 0: start from (0, 0, -inf)
    int finalize;     // 1: write O = acc / l and L = m + ln l; 0: store state
    int q_hs, k_hs;   // rows between consecutive heads of Q/O/Oacc/L/M and of K/V (0: Nq, Nk -- dense slabs).
                      // Larger strides address a row range of every head (the zig-zag chunks of the causal ring).
    int kv_group;     // query heads per K/V head (>= 1, divides the head count; 1 = multi-head attention)
    const float* sink;   // [sink_heads] fp32 attention sinks (fa2_forward_sink) or nullptr; read by finalising launches only
    int sink_heads;      // H_q: BH flattens the batch, head h of it reads sink[h % sink_heads]
};

hipError_t launch_fwd1_bf16(const FwdArgs& a, hipStream_t stream);     // generated main loop: one wave per SIMD (d = 128), two (d = 64)

// Packed variable-length batches (fa2_forward_varlen / fa2_backward_varlen and their _qk forms): tensors are head slabs [H][T][d]
// in which sequence i owns rows [cu_seqlens[i], cu_seqlens[i + 1]) -- of Q's T_q rows by one list and of K's T_k rows by a second
// one in a two-sided plan; one launch covers every sequence.  A workgroup's unit of work is one item
// of a table the host built (fa2_varlen_plan_build) and the caller uploaded: a 256-row block of one sequence's queries (forward,
// dQ kernel) or a 256-key block of its keys (dK/dV kernel).
struct VarlenItem {
    int q_row0, k_row0;   // the sequence's first row in Q / O / dO / dQ / L and in K / V / dK / dV
    int len_q, len_k;     // its lengths on the two sides (a row-block item may have len_k = 0, a key-block item len_q = 0); the
                          // causal mask of the view is shifted by len_k - len_q (the last query sees the last key)
    int block;            // which 256-row (256-key) block of the sequence
};
// a: the whole packed problem -- BH = H_q, q_hs = T_q, k_hs = T_k, pointers at row 0 of head 0; Nq, Nk, causal_shift, resume,
// finalize are per item
struct VarlenFwdArgs { FwdArgs a; const VarlenItem* items; int n_items; };      // items: DEVICE memory, row-block items
hipError_t launch_fwd1_varlen_bf16(const VarlenFwdArgs& v, hipStream_t stream);
// acc (fp32) = (init) or += src (bf16): `rows` runs of `cols` elements, `pitch` elements apart in both.
hipError_t launch_accumulate_bf16(float* acc, const void* src, size_t rows, size_t cols, size_t pitch, int init, hipStream_t stream);
// Ring epilogue: O = bf16(Oacc / l), L = m + ln l for `rows` consecutive rows (l arrives in L).
hipError_t launch_finalize_state(const float* Oacc, const float* M, float* L, void* O, size_t rows, int d, hipStream_t stream);

// Merging partial attention results (fa2_merge.hip; fa2_merge_states): n parts (O_i bf16 [rows][d], L_i fp32 [rows]) over disjoint
// key sets -> the attention over their union.  The part pointers travel BY VALUE in the kernel's argument block.
constexpr int kMergeMaxParts = 8;
struct MergeArgs {
    const void* O[kMergeMaxParts]; const float* L[kMergeMaxParts];      // entries [n, 8) are never read
    int n;
    void* Oout; float* Lout;      // the merged O and L: written by the forward, read by the backward
    size_t rows;
};
struct MergeBwdArgs {
    MergeArgs m;
    const void* dO; const float* dL;      // dL may be nullptr (= 0)
    void* dO_parts[kMergeMaxParts]; float* dL_parts[kMergeMaxParts];
};
hipError_t launch_merge_fwd(const MergeArgs& a, int d, hipStream_t stream);        // d = 64 | 128
hipError_t launch_merge_bwd(const MergeBwdArgs& b, int d, hipStream_t stream);

// Split-KV decode over a KV cache (fa2_decode.hip; fa2_forward_decode): Q, O [B][Hq][Nq][d] bf16, K, V [B][Hkv][Ncap][d] bf16,
// L [B][Hq][Nq]; seqlens (DEVICE, int [B]) and sink (DEVICE, fp32 [Hq]) may be nullptr.  n_splits >= 2: every split writes its
// normalised fp32 partial to wsO [n_splits][B Hq Nq][d] and its LSE to wsL [n_splits][B Hq Nq], and a combine launch follows.
constexpr int kDecodeTile = 32;            // keys of one MFMA tile: one wave's step
constexpr int kDecodeKB = 128;             // the key block: one round of the four waves; a split's first key is a multiple of it
constexpr int kDecodeMaxRows = 32;         // G Nq: the query rows of a K/V head fill the 32 columns of one tile
constexpr int kDecodeMaxSplits = 256;
constexpr int kDecodeCUs = 256;            // compute units of an MI355X: what the default split count fills
constexpr int kDecodeMinSplitKeys = 256;   // the default gives a split of a full cache at least this many keys
struct DecodeArgs {
    const void* Q; const void* K; const void* V; const int* seqlens; const float* sink;
    void* O; float* L; float* wsO; float* wsL;
    int B, Hq, Hkv, Nq, Ncap, n_splits;
    float scale;
    int causal;
    // fa2_forward_decode_paged: K, V are page pools [n_pages][Hkv][page_size][d], Ncap = max_pages page_size, and key j of
    // sequence b is row j % page_size of page block_table[b][j / page_size] (DEVICE, int [B][max_pages]).  All zero: contiguous.
    const int* block_table;
    int n_pages, page_size, max_pages;
    // fa2_forward_decode_fp8kv / _paged_fp8kv: kv_fp8 = 1, K and V hold OCP e4m3 bytes, the stored value of head h being
    // x / descale[h] (DEVICE, fp32 [Hkv]; nullptr = 1: scores softmax_scale k_descale[h] (Q . K8), O = v_descale[h] P V8).  All zero: bf16.
    const float* k_descale; const float* v_descale;
    int kv_fp8;
    // fa2_forward_decode_window / _paged_window: window_left >= 0, query i of sequence b sees keys [pos_i - window_left, pos_i],
    // pos_i = i + len_b - Nq (causal only); rows and table entries below lo_b = max(0, len_b - Nq - window_left) are never read.
    // Negative: no window, the kernels above (every other entry point sets -1).
    int window_left;
};
int decode_num_splits(int B, int H_kv, int kv_capacity);      // pure host arithmetic: fa2_decode_num_splits
hipError_t launch_decode(const DecodeArgs& a, int d, hipStream_t stream);      // d = 64 | 128; 1 <= G Nq <= 32; block_table: paged; kv_fp8: e4m3

// Extend attention (fa2_forward_extend, include/fa2_extend_mi355x.h): launch_decode's arguments with any G Nq >= 1 -- the group's
// rows go in blocks of kExtendRows, two 32-row tiles per wave, grid B Hkv ceil(G Nq / kExtendRows) n_splits -- and its partials.
#ifndef FA2_EXTEND_ROWS      // 32: one row tile per wave, the grid-only form (an A/B build: tools/gpu_extend_ab.py)
#define FA2_EXTEND_ROWS 64
#endif
constexpr int kExtendRows = FA2_EXTEND_ROWS;
hipError_t launch_extend(const DecodeArgs& a, int d, hipStream_t stream);

// Ragged extend attention (fa2_forward_extend_ragged, include/fa2_extend_ragged_mi355x.h): a q_len per sequence, token-major rows.
// a: launch_extend's with B sequences, Nq unused (every sequence brings its own), Q [T][Hq][d] with q_stride elements between
// tokens, O [T][Hq][d], L [T][Hq], partials [n_splits][T Hq].  The PLAN (DEVICE, ints, written by launch_extend_ragged_plan
// from cu_seqlens_q alone) is where a workgroup learns its sequence and row block:
//   header [kRaggedPlanHeader]: B, G = Hq / Hkv, T, the number of work items, the first owned token, one past the last, 0, 0
//   seq [B][2]: (start_b, q_b), 0 <= start_b, start_b + q_b <= T, the sequences tiling [first token, last) in order of b
//   items [max_blocks][2]: (b, row block j of the [G][q_b] slab), in order of b; (-1, 0) from the header's count on.
// A workgroup whose header does not name the call's B, G and T leaves at once, and so does one whose entries are out of range.
constexpr int kRaggedPlanHeader = 8;
struct ExtendRaggedArgs {
    DecodeArgs a;
    const int* plan;
    int T, max_blocks;
    long long q_stride;
};
long long extend_ragged_max_blocks(int B, int H_q, int H_kv, int total_q);      // floor(G T / 64) + min(B, T); host arithmetic
hipError_t launch_extend_ragged_plan(const int* cu_seqlens_q, int B, int G, int T, int* plan, hipStream_t stream);
hipError_t launch_extend_ragged(const ExtendRaggedArgs& x, int d, hipStream_t stream);

// fp8 (OCP e4m3) forward, d = 128: Q, K, V fp8 [BH][N][128]; O bf16; Vt: [BH][128][Npad] fp8 scratch the
// launcher fills with V transposed (Npad = N rounded up to 64); kn: [BH][Npad / 64] fp32 scratch it fills with the largest
// |k| of every 64 keys (fa2_fwd_fp8.hip: where the softmax needs no lane maxima).
struct FwdFp8Args {
    const void* Q; const void* K; const void* V;
    void* Vt;
    float* kn;
    void* O;
    float* L;
    int BH, N, Npad, d;
    float scale;      // what multiplies q . k of the STORED e4m3 values: softmax_scale x q_descale x k_descale
    int causal;
    float o_scale;    // what multiplies O: v_descale (1 = V holds its own values)
};
hipError_t launch_fwd_fp8(const FwdFp8Args& a, hipStream_t stream);

struct BwdArgs {
    const void* Q; const void* K; const void* V; const void* O; const void* dO;  // bf16
    const float* L;   // [BH][q_hs] natural-log LSE over ALL keys of the row (pointer at row q_row0 of head 0, like Q)
    void* dQ; void* dK; void* dV;   // bf16
    float* D;         // [BH][q_hs] workspace plane: rowsum(dO o O)                (dense, NOT offset by q_row0)
    float* RC;        // [2][BH][q_hs] workspace planes: -L/scale and -D, the row constants of the dK/dV kernel
    int BH, Nq, Nk, d;
    int q_hs, k_hs;   // rows between consecutive heads of Q/O/dO/dQ/L and of K/V/dK/dV (>= Nq, Nk; dense: == Nq, Nk)
    int q_row0;       // the block's rows are rows [q_row0, q_row0 + Nq) of every head (indexes the workspace planes)
    float scale;
    int causal;       // key j is visible to local row i iff j <= i + causal_shift
    int causal_shift;
    int phases;       // bit 0: D = rowsum(dO o O), bit 1: dQ kernel, bit 2: dK/dV kernel (7 = all)
    int reserve_cus;  // single-kernel form: CUs its persistent grid leaves free (for a communication kernel on another stream)
    int kv_group;     // grouped-query attention: query heads per K/V head (>= 1, divides BH; 1 = multi-head).  K, V, dK, dV
                      // then hold BH / kv_group slabs and query head h works against slab h / kv_group.  The two kernels of
                      // fa2_bwd_bf16.hip take it on any problem (rectangular, packed); the single kernel on dense square ones only
};

// The gradient of the attention sinks (fa2_backward_sink): dsink[h] = - sum over the batch and the rows of exp(sink[h] - L) D,
// one more kernel behind kernel 0 (phase bit 0) over the D plane it wrote.  Handed BESIDE BwdArgs: no other kernel sees it.
// dL (fa2_backward_lse): the gradient of L, addressed like BwdArgs::L, or nullptr; kernel 0 alone reads it (D' = D - dL, so the
// sinks' gradient above is taken over D').  sink and dsink are nullptr together in a call that only brings dL.
struct SinkGrad { const float* sink; float* dsink; int heads; const float* dL = nullptr; };      // heads = H_q (BH = batch x heads)

hipError_t launch_bwd_bf16(const BwdArgs& a, hipStream_t stream, const SinkGrad* sg = nullptr);
// The two-kernel backward over a packed variable-length batch.  a: the whole packed problem -- BH = H_q, q_hs = T_q, k_hs = T_k,
// Nq = T_q for the D kernel (one dense launch over H_q x T_q rows), q_row0 / Nq / Nk / causal_shift per item in the other two;
// D / RC dense [H_q][T_q] planes.
struct VarlenBwdArgs {
    BwdArgs a;
    const VarlenItem* row_items; const VarlenItem* key_items;      // DEVICE memory
    int n_row_items, n_key_items;
};
hipError_t launch_bwd_varlen_bf16(const VarlenBwdArgs& v, hipStream_t stream, const SinkGrad* sg = nullptr);
// Single-kernel five-product backward (fa2_bwd_fused.hip): d = 128 or 64, a dense square problem or (d = 128, mode 1) an unmasked
// rectangular block; causal with mode 1 only.  Which problems come here: the routing rule at fa2_backward (include/fa2_mi355x.h),
// applied by fa2_capi.cpp alone (device check included).
// dQacc: [BH][NP][128] fp32 scratch (NP = N rounded up to 256); ctl: bwd_fused_ctl_bytes of scratch; mode 0 = dQ by fp32
// atomics (N % 256 == 0 only), 1 = dQ handed from key block to key block in a fixed order (deterministic; any N: a ragged
// launch also needs rcpad, 2 BH NP floats, for the padded row-constant planes).  hipErrorInvalidValue for shapes it does not take.
size_t bwd_fused_ctl_bytes(int BH, int N);
// kv_group > 1 (dense square problems, mode 1): the kernel stores every unit's dK / dV per QUERY head into `kvpart`
// (bwd_fused_kvpart_bytes: bf16 dK [BH][Nk][d] | dV [BH][Nk][d]) and fa2_bwd_fused_dkdv_out_kernel adds the kv_group partials of
// every K/V head, in ascending query-head order in fp32, into dK / dV.
size_t bwd_fused_kvpart_bytes(int BH, int N, int d);
hipError_t launch_bwd_fused_bf16(const BwdArgs& a, float* dQacc, int* ctl, int mode, hipStream_t stream, float* rcpad = nullptr,
                                 void* kvpart = nullptr, const SinkGrad* sg = nullptr);
// Whether the current device has the layout the ordered hand-off (mode 1) was validated on; *why = a static sentence.
bool bwd_fused_device_ok(const char** why);
// Synchronises `stream` and reads the error word a chained launch leaves in its control block (non-zero: a bounded wait
// ran out and the output pass turned dQ into NaNs).
hipError_t bwd_fused_read_error(const int* ctl, int* err, hipStream_t stream);
hipError_t bwd_fused_clear_error(int* ctl, hipStream_t stream);      // error word <- 0 (a backward on this workspace without a hand-off)

// fp32 family (exact f32 MFMA, any d <= 128, any N): the reference-signature drop-ins.
struct F32Args {
    const float* Q; const float* K; const float* V; float* O; float* L;
    const float* dO; float* dQ; float* dK; float* dV; float* D;
    int BH, N, d;
    float scale;
    int causal;
    int phases;       // backward only, as BwdArgs::phases
    // forward only -- resumable step (ring): Nk keys in the resident shard (0 = N), running max
    // in M, running sum in L and the un-normalised accumulator in O itself between steps,
    // exactly the reference's state layout (ring_attention_kernel.cu:67-79, :125-137).
    int Nk;
    float* M;
    int resume, finalize;   // plain forward: resume = 0, finalize = 1
};
hipError_t launch_fwd_f32(const F32Args& a, hipStream_t stream);
hipError_t launch_bwd_f32(const F32Args& a, hipStream_t stream);

// Enqueues kernel K (one struct argument) with `lds` bytes of dynamic LDS, raising K's dynamic-LDS limit on the current device
// the first time (one flag per kernel instance and device; a benign race: the attribute is idempotent).
template <auto K, typename A>
inline hipError_t launch_lds(dim3 grid, dim3 block, int lds, hipStream_t stream, const A& arg)
{
    static bool done[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        done[dev] = true;
    }
    hipLaunchKernelGGL(K, grid, block, lds, stream, arg);
    return hipGetLastError();
}

// FlashAttention-1 restatement (fa1_f32.hip): one head, fp32, didactic baseline row.
hipError_t launch_fa1_f32(const float* Q, const float* K, const float* V, float* O, float* l, float* m, int N, int d, int Bc,
                          hipStream_t stream);

// Element-wise helpers (fa2_util.hip).
hipError_t launch_fill_f32(float* p, size_t n, float value, hipStream_t stream);
hipError_t launch_mfma_probe(const void* in, float* out, int iters, int blocks, hipStream_t stream);
hipError_t launch_f32_to_bf16(const float* src, void* dst, size_t n, hipStream_t stream);
hipError_t launch_bf16_to_f32(const void* src, float* dst, size_t n, hipStream_t stream);
hipError_t launch_read_clocks(unsigned long long* out, hipStream_t stream);

}  // namespace fa2
