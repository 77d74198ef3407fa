/*
 * fa2_mi355x.h -- C ABI of the MI355X-native FlashAttention-2 hot path (libfa2_mi355x.so).
 *
 * This is the drop-in boundary for the three host wrappers the reference
 * (terryye/cuda_FlashAttention) calls from its test mains -- there is no registry or FFI in
 * the reference, the wrappers ARE its operator interface:
 *
 *   flash_attention_2_forward   src/02_flash_attention_v2_forward/flash_attention_kernel.cu:300-309
 *                               (cleaned copy src/03_flash_attention_v2_ring/common/flash_attention_kernel.cu:133-172)
 *   flash_attention_2_backward  src/02_flash_attention_v2_backward/flash_attention_backward_kernel.cu:249-262
 *   ring_attention_forward      src/03_flash_attention_v2_ring/common/ring_attention_kernel.cu:143-156
 *                               (declared in fa2_ring_mi355x.h: it needs RCCL)
 *
 * Conventions (all entry points):
 *   - plain C, raw DEVICE pointers and sizes, no framework types;
 *   - tensors are contiguous row-major [B][H][N][d] ("head slabs" [N][d], each an independent
 *     instance of the reference's single-head problem); L is [B][H][N] fp32 and holds the
 *     NATURAL-log logsumexp of the scaled scores, exactly what the reference stores
 *     (flash_attention_kernel.cu:291-294);
 *   - the caller owns every tensor; the library never allocates in the extended entry points;
 *   - stream-ordered and asynchronous: work is enqueued on `stream` (a hipStream_t passed as
 *     void*; NULL = the default stream) and the call returns; nothing synchronises;
 *   - return value: FA2_OK (0) or a negative status.  The library never aborts -- the
 *     reference's assert()/exit() policy (cuda_helper.h:74-82, nccl_utils.h:11-18,
 *     flash_attention_kernel.cu:317) becomes status codes.
 */
#ifndef FA2_MI355X_H
#define FA2_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------- */
#define FA2_OK                     0
#define FA2_ERR_NULL_POINTER      -1
#define FA2_ERR_INVALID_SHAPE     -2   /* B, H, N <= 0, scale <= 0, ... */
#define FA2_ERR_UNSUPPORTED_HEAD_DIM -3 /* bf16/fp8: d must be 64 or 128; fp32: 1 <= d <= 128 */
#define FA2_ERR_UNSUPPORTED_DTYPE -4
#define FA2_ERR_WORKSPACE         -5   /* workspace NULL or smaller than *_workspace_bytes() */
#define FA2_ERR_UNSUPPORTED       -6   /* combination not implemented (e.g. causal ring) */
#define FA2_ERR_HANDOFF_TIMEOUT   -7   /* fa2_backward_status: a bounded wait of the single-kernel backward ran out; dQ is NaN */
#define FA2_ERR_HIP_BASE          -1000 /* -(1000 + hipError_t) */
#define FA2_ERR_RCCL_BASE         -2000 /* -(2000 + ncclResult_t) */

/* ---- element types of Q/K/V/O/dO/dQ/dK/dV -------------------------------------------- */
#define FA2_DTYPE_BF16 0   /* primary: bf16 in, fp32 accumulate on v_mfma_f32_32x32x16_bf16 */
#define FA2_DTYPE_F32  1   /* the reference's type: exact f32 MFMA (v_mfma_f32_32x32x2_f32)  */
#define FA2_DTYPE_FP8_E4M3 2 /* forward only: OCP e4m3 Q/K/V on v_mfma_f32_32x32x64_f8f6f4, O in bf16, d = 128 */

const char* fa2_version(void);
const char* fa2_status_string(int status);

/* ======================================================================================
 * Reference-signature drop-ins: single head, fp32, default stream -- argument for argument
 * the reference's wrappers, with `void` widened to an int status.  Any seq_len >= 1, any
 * 1 <= head_dim <= 128 (the reference asserts head_dim <= 64 / 128).
 * ==================================================================================== */

/* replaces flash_attention_2_forward (02_forward/flash_attention_kernel.cu:300-309) */
int flash_attention_2_forward(const float* Q, const float* K, const float* V,
                              float* O, float* L,
                              int seq_len, int head_dim, float softmax_scale);

/* replaces flash_attention_2_backward (02_backward/flash_attention_backward_kernel.cu:249-262).
 * Like the reference it overwrites dQ, dK, dV (the reference memsets dK, dV itself, :282-283).
 * Scratch for D = rowsum(dO o O) comes from a per-device cache owned by the library. */
int flash_attention_2_backward(const float* Q, const float* K, const float* V,
                               const float* O, const float* L, const float* dO,
                               float* dQ, float* dK, float* dV,
                               int seq_len, int head_dim, float softmax_scale);

/* replaces flash_attention (01_flash_attention_v1/main.cu:7-20), the FlashAttention-1 step of the reference's staircase:
 * O = softmax(Q K^T / sqrt(d)) V for one fp32 head with the running row sums l and row maxima m written beside it
 * (m + ln l is the row's log-sum-exp).  Bc is the number of keys per staged K/V tile, as in the reference (whose tests sweep
 * Bc in {1, 2, 4}, main.cu:300-345): 1 <= Bc, values above 64 are clamped to 64 (the kernel's LDS tile); M is accepted and,
 * as in the reference's own wrapper (main.cu:22), not used.  A didactic baseline (scalar fp32, no MFMA): the fast path is flash_attention_2_forward. */
int flash_attention(const float* Q, const float* K, const float* V, float* O, float* l, float* m,
                    int N, int d, int Bc, int M);

/* ======================================================================================
 * Extended entry points: (B, H), dtype, causal mask, stream.
 * ==================================================================================== */

/* O = softmax(scale * Q K^T [+ causal mask]) V ;  L = logsumexp rows.
 * dtype BF16: Q,K,V,O bf16, d in {64,128}.  dtype F32: Q,K,V,O fp32, 1 <= d <= 128.
 * bf16 numerics: a row's softmax reference is set by the first keys it sees (64 at d = 128, 128 at d = 64; lazily, as the
 * reference's running maximum would be) and afterwards only lifted in steps of 64 ln 2 when the row's sum has outgrown 2^30 --
 * in fp32 sums and bf16 probabilities a lagging reference changes nothing but rounding.  A 256-row block one of whose rows
 * would leave the safe range that way (scores jumping by more than ~48 natural units within 256 / 512 consecutive keys) is
 * computed a second time with the running maximum followed key block by key block: same results, twice the time for that
 * block.  NaN inputs give NaN outputs. */
int fa2_forward(const void* Q, const void* K, const void* V, void* O, float* L,
                int B, int H, int seq_len, int head_dim, float softmax_scale,
                int dtype, int causal, void* stream);

/* fp8 (OCP e4m3) forward, BASELINE configs[4]: Q, K, V are e4m3 [B][H][N][128], O is bf16, L fp32.  The
 * kernel reads V through a transposed copy ([B][H][128][N rounded up to 64], e4m3) that this call writes
 * into `workspace` first, followed by the largest key norm of every 64 keys ([B][H][N / 64] fp32: where scale |q| |k|
 * cannot reach a row's rescale threshold the kernel skips that row's running-maximum update -- same results)
 * (fa2_forward_fp8_workspace_bytes).  fa2_forward(..., FA2_DTYPE_FP8_E4M3, ...) is
 * the same call with the workspace taken from the stream-ordered allocator.  No counterpart in the
 * reference (fp32 end to end): parity is against the oracle fed the e4m3-rounded inputs. */
size_t fa2_forward_fp8_workspace_bytes(int B, int H, int seq_len, int head_dim);
int fa2_forward_fp8(const void* Q, const void* K, const void* V, void* O, float* L,
                    int B, int H, int seq_len, int head_dim, float softmax_scale, int causal,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The same for tensors stored as x / descale (per-tensor scaling, what an fp8 producer that uses e4m3's range hands over):
 * the scores are softmax_scale (q_descale Q)(k_descale K)^T and O = P (v_descale V).  fa2_forward_fp8 is this call with the
 * three descales 1 -- i.e. for tensors whose own values fit e4m3 (|x| <= 448); a caller with scaled tensors who uses that
 * entry point must fold q_descale k_descale into softmax_scale and multiply O by v_descale himself.  L is the log-sum-exp
 * of the DESCALED scores either way.  Each of the three descales must be positive and finite: zero, a negative number, NaN and
 * +inf are refused with FA2_ERR_INVALID_SHAPE before anything is launched. */
int fa2_forward_fp8_scaled(const void* Q, const void* K, const void* V, void* O, float* L,
                           int B, int H, int seq_len, int head_dim, float softmax_scale,
                           float q_descale, float k_descale, float v_descale, int causal,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of scratch fa2_backward needs for this problem: D and the row-constant planes, plus -- for the shapes the
 * single-kernel backward takes (rule (a) of fa2_backward) -- the fp32 running sums of dQ (B H NP 128 x 4 bytes at either
 * head_dim, NP = seq_len rounded up to a multiple of 256), a small control block and, when NP != seq_len, padded
 * row-constant planes. */
size_t fa2_backward_workspace_bytes(int B, int H, int seq_len, int head_dim, int dtype);

/* dQ, dK, dV from Q, K, V, O, L (forward outputs) and dO.  Deterministic: no floating-point atomics, every
 * gradient element is summed in a fixed order (the reference's smem + global atomicAdd scheme,
 * flash_attention_backward_kernel.cu:208-231, is not reproduced).  Two implementations for bf16 (fp32 has kernels of its own):
 *   - the SINGLE KERNEL (csrc/fa2_bwd_fused.hip, head_dim 128 or 64, causal or not) forms the five block products once; a
 *     workgroup owns 256 keys (dK, dV in registers) and the dQ tiles are summed key block after key block in a fixed order
 *     through the L2 of the XCD the head is pinned to.  Its loops run on seq_len rounded up to a multiple of 256 (keys past
 *     the end masked, rows past the end given row constants that make P vanish, nothing past the end stored);
 *   - the TWO KERNELS: a dQ kernel and a dK/dV kernel (seven products, csrc/fa2_bwd_bf16.hip).
 * THE ROUTING RULE, which every backward entry point follows (fa2_backward_plan reports it for a problem): bf16 runs the single
 * kernel iff
 *   (a) its padding costs less than what the two kernels cost more:
 *       head_dim 128 -- 5 roundup(N, 256) <= 7 roundup(N, 64) (the other form's two extra block products on 64-key tiles):
 *         129 <= N <= 256 and every N >= 321;
 *       head_dim 64 -- 13 roundup(N, 256) <= 14 roundup(N, 64) (the single kernel is ~10 % ahead there, so the padding may cost
 *         7 %): every N >= 2369 and every multiple of 256; below 2369 the lengths 193-256, 449-512, 705-768, 897-1024,
 *         1153-1280, 1409-1536, 1601-1792, 1857-2048, 2113-2304;
 *   (b) the environment variable FA2_BACKWARD_PATH is not "two_kernel" (read once per process), and
 *   (c) the device is the layout the hand-off was validated on (PLACEMENT ASSUMPTION below);
 * every other problem runs the two kernels.  fa2_backward_block applies the rule to two block shapes, given phase bits 1 and 2
 * and the full workspace of fa2_backward_workspace_bytes(B, H, q_head_stride, ...): a DENSE SQUARE block (q_len = kv_len, dense
 * strides, q_row0 = 0, causal only with shift 0) with (a) on its length, and an UNMASKED (non-causal) rectangular, head-strided
 * block of head_dim 128 with q_len a multiple of 32 and >= 512 and kv_len a multiple of 256 and <= roundup(q_head_stride, 256),
 * with (a) on q_head_stride (the zig-zag causal ring's half blocks).
 * PLACEMENT ASSUMPTION of the single kernel: its workgroups read HW_REG_XCC_ID and hand running sums to each other through the
 * L2 of that XCC (plain stores, sc1 loads); validated on gfx950 in SPX mode (one device = 8 XCCs x 32 CUs).  On any other
 * device layout (a partitioned GPU, another architecture) this call runs the two kernels instead: fa2_backward_plan.
 * A hand-off that times out (every wait is bounded) leaves dQ all NaN and dK / dV complete: fa2_backward_status. */
int fa2_backward(const void* Q, const void* K, const void* V, const void* O, const float* L,
                 const void* dO, void* dQ, void* dK, void* dV,
                 int B, int H, int seq_len, int head_dim, float softmax_scale,
                 int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream);

/* Which implementation fa2_backward runs for this problem ON THE CURRENT DEVICE: 1 = the single five-product kernel,
 * 2 = the dQ + dK/dV kernels (or the fp32 kernels); negative = status.  *reason (may be NULL) receives a static sentence.
 * The single kernel hands running dQ sums from workgroup to workgroup through the L2 of the XCC both run on (they read
 * HW_REG_XCC_ID and take work from that XCC's queue); that was validated on gfx950 exposing all 256 CUs (SPX mode).  On a
 * partitioned GPU or another architecture fa2_backward silently uses the two kernels instead -- this call says so. */
int fa2_backward_plan(int B, int H, int seq_len, int head_dim, int dtype, int causal, const char** reason);

/* Synchronises `stream` and reports how the last fa2_backward / fa2_backward_phases / fa2_backward_fused call on that
 * workspace ended: FA2_OK, or FA2_ERR_HANDOFF_TIMEOUT when a workgroup of the single-kernel backward gave up waiting for
 * the key block before it (every such wait is bounded, 2^22 polls).  CONTRACT: the launch itself returns FA2_OK either way
 * (it is asynchronous); after a time-out EVERY element of dQ is NaN (the output pass poisons it) while dK and dV are
 * complete and correct -- they never depend on the hand-off.  A caller that consumes dK / dV without looking at dQ should
 * call this once per step (it costs a stream synchronisation and a 4-byte copy).  Shapes that run the two kernels have no
 * hand-off: the call only synchronises. */
int fa2_backward_status(const void* workspace, size_t workspace_bytes, int B, int H, int seq_len, int head_dim, int dtype,
                        void* stream);

/* ---- Grouped-query attention (GQA; H_kv = 1: multi-query attention), bf16, head_dim 64 or 128, causal or not, any seq_len.
 * H_q query heads share H_kv key/value heads, H_q % H_kv == 0 (any group size G = H_q / H_kv, powers of two or not): query head h
 * attends K/V head h / G.  Layouts stay dense: Q, O, dO, dQ are [B][H_q][N][d], K, V, dK, dV are [B][H_kv][N][d], L is
 * [B][H_q][N] -- no expanded copy of K / V and no [B][H_q] copy of dK / dV is ever formed by the caller.
 * fa2_forward_gqa: the forward kernels of fa2_forward with the K/V slab of head h / G; a query head's arithmetic does not depend
 * on where its K/V live, so O and L are bit-identical to fa2_forward on K, V repeated to H_q heads.
 * fa2_backward_gqa: `phases` as in fa2_backward_phases (7 = the routing rule picks; 6 = the two kernels whatever the shape, on
 * what a call with bit 0 left in the workspace; 8 or 8|1 = the single kernel, FA2_ERR_UNSUPPORTED where it does not apply).  THE ROUTING RULE is that of fa2_backward
 * for the multi-head problem (B, H_q, seq_len, head_dim) -- rule (a) depends on seq_len and head_dim only, (b) and (c) on the
 * process and the device -- and fa2_backward_gqa_plan reports it (always equal to fa2_backward_plan(B, H_q, ...)).
 *   - two kernels: the dQ kernel reads K/V of head h / G; a dK/dV workgroup owns 256 keys of a K/V head and walks the query tiles
 *     of its G query heads one after the other on top of the same accumulators (grid: key blocks x B H_kv), storing once;
 *   - single kernel: a unit stays (query head, key block) and the dQ hand-off is unchanged; every unit stores its dK / dV per
 *     query head as bf16 partials into the workspace, and a reduction kernel adds the G partials of every K/V head in ascending
 *     query-head order in fp32 and writes bf16 dK / dV (G == 1: no partials, no extra launch).
 * dQ is bit-identical to fa2_backward's on the repeated K, V.  DETERMINISTIC like fa2_backward: every sum has a fixed order, no
 * floating-point atomics.
 * WORKSPACE: fa2_backward_gqa_workspace_bytes = fa2_backward_workspace_bytes(B, H_q, ...) plus, where rule (a) admits the single
 * kernel and G > 1, the partials (2 B H_q seq_len head_dim x 2 bytes), placed BEHIND everything the multi-head layout holds:
 * fa2_backward_status(workspace, bytes, B, H_q, seq_len, head_dim, dtype, stream) finds the control block where it always was
 * and works on the workspace of a grouped launch.  With H_kv == H_q the three calls enqueue exactly what fa2_forward /
 * fa2_backward_phases enqueue, and the workspace is that of fa2_backward_workspace_bytes.
 * Status codes: H_kv <= 0 or H_q % H_kv != 0 -> FA2_ERR_INVALID_SHAPE; fp32 and fp8 -> FA2_ERR_UNSUPPORTED_DTYPE (GQA is bf16 in
 * this version); everything else as in the multi-head calls, checked in the same order.  Not covered: the ring, the resumable
 * forward steps and fa2_backward_block. */
int fa2_forward_gqa(const void* Q, const void* K, const void* V, void* O, float* L,
                    int B, int H_q, int H_kv, int seq_len, int head_dim, float softmax_scale,
                    int dtype, int causal, void* stream);
size_t fa2_backward_gqa_workspace_bytes(int B, int H_q, int H_kv, int seq_len, int head_dim, int dtype);
int fa2_backward_gqa(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                     void* dQ, void* dK, void* dV,
                     int B, int H_q, int H_kv, int seq_len, int head_dim, float softmax_scale,
                     int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases);
int fa2_backward_gqa_plan(int B, int H_q, int H_kv, int seq_len, int head_dim, int dtype, int causal,
                          const char** reason);

/* ---- Packed variable-length attention ("varlen", cu_seqlens), bf16, head_dim 64 or 128, causal (within each sequence) or
 * not, H_q % H_kv == 0 (multi-head, GQA and MQA).  A ragged batch -- documents of 37, 300 and 5000 tokens -- in ONE launch
 * sequence, without padding and without a loop of per-document calls.  Self-attention: a sequence has the same length on the
 * query and on the key side.
 * LAYOUT: packed head slabs, as everywhere in this ABI.  With T = cu_seqlens[n_seqs], Q, O, dO, dQ are [H_q][T][d], K, V, dK, dV
 * are [H_kv][T][d], L is [H_q][T] fp32; sequence i owns rows [cu_seqlens[i], cu_seqlens[i+1]) of every head.  A caller that
 * holds [T][H][d] transposes first.  Sequences of length 0 are allowed and cost nothing.
 * THE PLAN.  cu_seqlens is HOST data, like every other size here.  fa2_varlen_plan_build (pure host code, no device needed)
 * validates it and writes a blob of at most fa2_varlen_plan_bytes(n_seqs, T) bytes into plan_host: a header (magic, version,
 * n_seqs, T, the two item counts, the longest length, and a word that is 0 in this one-list plan and the key side's row count
 * in a two-sided one, see fa2_varlen_plan_build_qk below: 8 ints) and two lists of items, each five ints
 * {q_row0, k_row0, len_q, len_k, block} -- both sides are carried; they are equal in a one-list plan.  ROW-BLOCK items (256 query rows of one sequence) are the units of the forward and of the dQ
 * kernel, KEY-BLOCK items (256 keys) those of the dK/dV kernel.  ORDER, deterministic and the same with or without the causal
 * mask: sequences by descending length, ties by index; within a sequence row blocks descend and key blocks ascend (the heaviest
 * first under a causal mask, indifferent without one); a sequence's blocks are adjacent, so its K / V stay in one XCD's L2.
 * The caller copies the blob to the device ONCE per batch layout and reuses it for every layer and step.  The launch calls take
 * both copies: the host copy for validation and grid sizes, the device copy (4-byte aligned) for the kernels to read; they
 * must hold the same bytes.
 * ROUTING.  Forward: the generated-body forward kernels of fa2_forward, one 256-row block per workgroup (the two-block pairing
 * of the dense causal launch does not carry over), grid = row-block items x H_q.  Backward: ALWAYS the two kernels (D over all
 * H_q x T rows in one dense launch, then dQ over row-block items x H_q and dK/dV over key-block items x H_kv, a dK/dV
 * workgroup walking the G query heads of its group as in fa2_backward_gqa).  The single five-product kernel hands dQ sums
 * through a persistent grid laid out for dense square heads; ragged units are a separate piece of work.  Workspace
 * (fa2_backward_varlen_workspace_bytes): D and the two row-constant planes, nothing else.
 * A block's arithmetic does not depend on where its sequence lives: sequence i of the packed forward is bit-identical to
 * fa2_forward_gqa on that sequence alone as [1][H][len_i][d], and the packed backward to fa2_backward_gqa with phases 1, then 6.
 * A sequence never reads another's rows: every buffer resource ends where the sequence ends.  DETERMINISTIC: no atomics, every
 * sum in a fixed order.  Nothing synchronises and nothing is allocated: the launch calls may be captured in a graph.
 * STATUS CODES, in this order: NULL pointers (the plan's included) -> FA2_ERR_NULL_POINTER; H_q, T, scale, H_kv not dividing
 * H_q, total_rows different from the plan's T, a blob without the magic, plan_bytes smaller than the blob, a two-sided plan
 * (these two calls would read K as T_q rows: it belongs to the _qk calls) -> FA2_ERR_INVALID_SHAPE; head_dim -> FA2_ERR_UNSUPPORTED_HEAD_DIM; fp32 and fp8 -> FA2_ERR_UNSUPPORTED_DTYPE; workspace ->
 * FA2_ERR_WORKSPACE.  fa2_varlen_plan_build: NULL -> FA2_ERR_NULL_POINTER; n_seqs < 1, cu_seqlens[0] != 0, a decreasing entry,
 * T < 1 or T above 4194303 rows (the 2 GiB-per-plane rule of every call, at the widest row) -> FA2_ERR_INVALID_SHAPE; plan_bytes
 * too small for this cu_seqlens -> FA2_ERR_WORKSPACE.  fa2_varlen_plan_bytes returns 0 for n_seqs < 1 or total_rows < 1.
 * NOT COVERED in this version: the single-kernel backward on packed batches, fp32 and fp8, the ring.
 * (Different query and key lengths per sequence: the _qk calls below.  A paged KV cache is read at decode, by
 * fa2_forward_decode_paged; a prompt chunk takes contiguous keys.) */
size_t fa2_varlen_plan_bytes(int n_seqs, int total_rows);
int fa2_varlen_plan_build(const int* cu_seqlens_host, int n_seqs, void* plan_host, size_t plan_bytes);
int fa2_forward_varlen(const void* Q, const void* K, const void* V, void* O, float* L,
                       int H_q, int H_kv, int total_rows, int head_dim, float softmax_scale, int dtype, int causal,
                       const void* plan_host, const void* plan_dev, size_t plan_bytes, void* stream);
size_t fa2_backward_varlen_workspace_bytes(int H_q, int H_kv, int total_rows, int head_dim, int dtype);
int fa2_backward_varlen(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                        void* dQ, void* dK, void* dV,
                        int H_q, int H_kv, int total_rows, int head_dim, float softmax_scale, int dtype, int causal,
                        const void* plan_host, const void* plan_dev, size_t plan_bytes,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- Different query and key lengths ("qk"): cross-attention, a prompt chunk against a longer contiguous KV cache (chunked
 * prefill), and ragged batches of either.  bf16, head_dim 64 or 128, H_q % H_kv == 0 (multi-head, GQA, MQA), causal or not,
 * DETERMINISTIC (no atomics).
 * DENSE LAYOUT: Q, O, dO, dQ [B][H_q][q_len][d]; K, V, dK, dV [B][H_kv][kv_len][d]; L [B][H_q][q_len]; q_len >= 1, kv_len >= 1.
 * PACKED LAYOUT: Q, O, dO, dQ [H_q][T_q][d]; K, V, dK, dV [H_kv][T_k][d]; L [H_q][T_q].  Sequence i owns query rows
 * [cu_q[i], cu_q[i+1]) and key rows [cu_k[i], cu_k[i+1]); T_q >= 1 and T_k >= 1; any single sequence may have len_q == 0,
 * len_k == 0, or both.
 * CAUSAL MASK, BOTTOM-RIGHT ALIGNED: key j is visible to query i of the same sequence iff j <= i + (len_k - len_q).  The last
 * query sees every key; with len_q == len_k this is the mask of every other call; the shift len_k - len_q may be negative.
 * A QUERY ROW THAT SEES NO KEY (causal with len_q > len_k, or len_k == 0) has O = 0 and L = -inf (the log-sum-exp of nothing); in
 * the backward its dQ = 0 and it contributes nothing to dK or dV.  A sequence with len_q == 0 < len_k gets dK = dV = 0 written
 * for its keys.  Every output element of every row in [0, T) is written by every call, and for finite inputs no NaN and no Inf
 * appears in O, dQ, dK or dV (the backward gives such a row finite row constants under which P vanishes, as the single kernel
 * does for rows past the end).
 * DENSE CALLS.  q_len == kv_len enqueues exactly what fa2_forward_gqa / fa2_backward_gqa enqueue -- the same routing rule, the same
 * workspace size, bit-identical results.  q_len != kv_len: the forward runs one 256-row block per workgroup when causal (the
 * two-block pairing balances a square's triangle only); the backward ALWAYS runs the two deterministic kernels (`phases` as
 * fa2_backward_gqa; bit 3, the single kernel, -> FA2_ERR_UNSUPPORTED), a dK/dV workgroup walking the query tiles of its group's
 * heads as in fa2_backward_gqa, and fa2_backward_qk_workspace_bytes is D plus the two row-constant planes over [B][H_q][q_len].
 * THE TWO-SIDED PLAN.  fa2_varlen_plan_build_qk takes two lists of n_seqs + 1 offsets.  With cu_seqlens_k_host NULL or
 * element-wise equal to the query list it writes BYTE FOR BYTE what fa2_varlen_plan_build writes (a one-list plan).  Otherwise:
 * the same magic, version and item format; the header's last word holds T_k (it is 0 in a one-list plan), its "longest length"
 * the longest len_q.  ORDER: sequences by descending len_q x len_k (64-bit), ties by index -- the one-list order when the lengths
 * are equal; row-block items for every sequence with len_q > 0 (len_k == 0 included), blocks descending; key-block items for
 * every sequence with len_k > 0 (len_q == 0 included), blocks ascending.  The two item counts may differ.
 * fa2_varlen_plan_bytes_qk(n_seqs, T_q, T_k) bounds the blob (0 for n_seqs < 1, T_q < 1 or T_k < 1).  Validation, per list:
 * offsets start at 0, never decrease, end at a total >= 1 and within the row limit of fa2_varlen_plan_build ->
 * FA2_ERR_INVALID_SHAPE otherwise; NULL query list or plan -> FA2_ERR_NULL_POINTER; plan_bytes too small -> FA2_ERR_WORKSPACE.
 * PACKED CALLS.  fa2_forward_varlen_qk / fa2_backward_varlen_qk take both kinds of plan; with a one-list plan they require
 * total_k == total_q and are fa2_forward_varlen / fa2_backward_varlen.  Kernels, grids and the bit-identity of a sequence with the
 * dense call on that sequence alone (here: fa2_forward_qk, and fa2_backward_qk with phases 1, then 6, for sequences with both
 * lengths >= 1) are those of the packed calls above; the workspace is D and the two row-constant planes over [H_q][T_q].
 * STATUS CODES of every call with tensors, in this order: NULL pointers -> FA2_ERR_NULL_POINTER; B, H_q, a length or total, scale,
 * H_kv not dividing H_q, totals different from the plan's, a blob without the magic or longer than plan_bytes ->
 * FA2_ERR_INVALID_SHAPE; head_dim -> FA2_ERR_UNSUPPORTED_HEAD_DIM; fp32 and fp8 -> FA2_ERR_UNSUPPORTED_DTYPE; workspace ->
 * FA2_ERR_WORKSPACE; then (dense rectangle, phases bit 3) FA2_ERR_UNSUPPORTED.
 * NOT COVERED: the single-kernel backward on rectangles, fp32 and fp8, the ring, strided K / V, sliding windows.  (One or a
 * few new tokens against a long cache: fa2_forward_decode below; against a pool of pages: fa2_forward_decode_paged.) */
int fa2_forward_qk(const void* Q, const void* K, const void* V, void* O, float* L,
                   int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                   int dtype, int causal, void* stream);
size_t fa2_backward_qk_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, int dtype);
int fa2_backward_qk(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                    void* dQ, void* dK, void* dV,
                    int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                    int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases);
size_t fa2_varlen_plan_bytes_qk(int n_seqs, int total_q, int total_k);
int fa2_varlen_plan_build_qk(const int* cu_seqlens_q_host, const int* cu_seqlens_k_host, int n_seqs, void* plan_host,
                             size_t plan_bytes);
int fa2_forward_varlen_qk(const void* Q, const void* K, const void* V, void* O, float* L,
                          int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                          const void* plan_host, const void* plan_dev, size_t plan_bytes, void* stream);
size_t fa2_backward_varlen_qk_workspace_bytes(int H_q, int H_kv, int total_q, int total_k, int head_dim, int dtype);
int fa2_backward_varlen_qk(const void* Q, const void* K, const void* V, const void* O, const float* L, const void* dO,
                           void* dQ, void* dK, void* dV,
                           int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                           const void* plan_host, const void* plan_dev, size_t plan_bytes,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- Attention sinks: one learned logit per query head that joins every row's softmax and carries no value (GPT-OSS, the
 * StreamingLLM line).  bf16, head_dim 64 or 128, every problem of the _qk calls above (square, rectangular, grouped, dense and
 * packed); the signatures are theirs with `sink` after V and `dsink` after dV.
 * DEFINITION.  sink is fp32 [H_q] in DEVICE memory, in natural units: it is NOT multiplied by softmax_scale.  For every (batch,
 * query head h, row i), with S_ij = softmax_scale q_i . k_j over the keys j visible to row i and s_h = sink[h]:
 *     L_i = log(exp(s_h) + sum_j exp S_ij),    P_ij = exp(S_ij - L_i),    O_i = sum_j P_ij v_j
 * -- the row's probabilities sum to 1 - exp(s_h - L_i), the rest stays with the sink.  L is the sink-INCLUSIVE log-sum-exp.
 * sink[h] = -inf means "no sink for this head": O, L, dQ, dK, dV of that head are bit for bit those of the calls without a
 * sink, and dsink[h] = 0.  A ROW THAT SEES NO KEY (causal with q_len > kv_len, a packed sequence without keys) has O = 0, dQ = 0
 * and L = s_h (-inf only if s_h = -inf); it adds nothing to dsink.  +inf and NaN in sink are the caller's error; the values live
 * in device memory and are not checked.
 * FORWARD: the kernels of fa2_forward_qk / fa2_forward_varlen_qk; the sink never meets their main loop.  A finished row has
 * Lrow = its log-sum-exp over the keys; the epilogue stores L' = max(Lrow, s) + log1p(exp(-|Lrow - s|)) and scales O by
 * exp(Lrow - L') = sigmoid(Lrow - s).
 * BACKWARD: the kernels of fa2_backward_qk / fa2_backward_varlen_qk, unchanged -- handed the sink-inclusive L and the sink-scaled
 * O they form P = exp(S - L) and D = rowsum(dO o O) (the sink's value is 0: dP_sink = 0) and with them the right dQ, dK, dV.
 * Routing, `phases`, the workspace (fa2_backward_sink_workspace_bytes = fa2_backward_qk_workspace_bytes, the packed one
 * likewise) and fa2_backward_status are those of fa2_backward_qk, the single kernel included where it takes the shape.
 * dsink[h] = - sum over the batch and the rows of exp(s_h - L_row) D_row (fp32 [H_q], DEVICE memory) is written by one more
 * kernel that runs with PHASE BIT 0, behind the D kernel, over the D plane in the workspace: a call without bit 0 leaves dsink
 * as it is.  DETERMINISTIC: one workgroup per query head, a fixed summation order, no floating-point atomics.  Nothing is
 * allocated and nothing synchronises: the calls may be captured in a graph.
 * STATUS CODES: a NULL sink or dsink (like every other NULL tensor) -> FA2_ERR_NULL_POINTER; then those of the _qk calls in
 * their order, fp32 and fp8 -> FA2_ERR_UNSUPPORTED_DTYPE.  fa2_forward_varlen_sink / fa2_backward_varlen_sink take both kinds of
 * plan; a one-list plan requires total_k == total_q.
 * NOT COVERED: the resumable forward steps and fa2_forward_state_finalize (no sink argument: a ring schedule finalises without
 * one), the ring, fp8 and fp32 (cuda_flashattention_amd.ops raises ValueError for a sink beside tensors that are not bf16). */
int fa2_forward_sink(const void* Q, const void* K, const void* V, const float* sink, void* O, float* L,
                     int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                     int dtype, int causal, void* stream);
size_t fa2_backward_sink_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, int dtype);
int fa2_backward_sink(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L, const void* dO,
                      void* dQ, void* dK, void* dV, float* dsink,
                      int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                      int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases);
int fa2_forward_varlen_sink(const void* Q, const void* K, const void* V, const float* sink, void* O, float* L,
                            int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                            const void* plan_host, const void* plan_dev, size_t plan_bytes, void* stream);
size_t fa2_backward_varlen_sink_workspace_bytes(int H_q, int H_kv, int total_q, int total_k, int head_dim, int dtype);
int fa2_backward_varlen_sink(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L,
                             const void* dO, void* dQ, void* dK, void* dV, float* dsink,
                             int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                             const void* plan_host, const void* plan_dev, size_t plan_bytes,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- A gradient for L, and merging partial results.  Every bf16 forward returns the row log-sum-exp L beside O; these calls
 * make it a differentiable output and combine (O, L) pairs computed over DIFFERENT KEY SETS into the attention over their union
 * (context-parallel and ring attention written in autograd, a prompt chunk against a prefix cache held in another allocation,
 * cascade / shared-prefix inference, z-loss).
 * fa2_backward_lse / fa2_backward_varlen_lse are fa2_backward_sink / fa2_backward_varlen_sink with `dL` behind dO: fp32, DEVICE
 * memory, shaped and addressed like L, the gradient of the loss with respect to L.  dL/dS_ij = P_ij, so dS = P o (dP - D + dL): the
 * D kernel stores D' = rowsum(dO o O) - dL and every other kernel runs unchanged; dsink = - sum exp(s_h - L) D' (dL/ds_h =
 * exp(s_h - L)).  dL takes effect with PHASE BIT 0, like dsink.  A row with L = -inf (no visible key, no sink) ignores its dL,
 * whatever it holds.  dL may be NULL (= 0); sink and dsink are NULL together (no sink) or non-NULL together, FA2_ERR_NULL_POINTER
 * otherwise.  With sink == NULL and dL == NULL the calls are fa2_backward_qk / fa2_backward_varlen_qk bit for bit; routing,
 * `phases`, status codes and the workspace (fa2_backward_qk_workspace_bytes / fa2_backward_varlen_qk_workspace_bytes) are theirs.
 * fa2_merge_states: n_parts (1..8) parts O_i (bf16 [rows][head_dim]) and L_i (fp32 [rows]), `rows` the flattened leading
 * dimensions ([B][H][N] or a packed [H][T]), head_dim 64 or 128:
 *     L = log sum_i exp L_i,    O = bf16(sum_i exp(L_i - L) O_i)         (fp32, ascending i: the same bits on every run)
 * O_parts / L_parts (and dO_parts / dL_parts) are HOST arrays of n_parts DEVICE pointers, read during the call.  A part with
 * L_i = -inf on a row is left out of that row (its O_i row may hold anything); all parts -inf: O = 0, L = -inf; one part: its bits.
 * fa2_merge_states_backward: from the parts, the merged O and L, dO (bf16) and dL (fp32 or NULL), with w_i = exp(L_i - L):
 *     dO_i = bf16(w_i dO),    dL_i = w_i (dL + rowsum(dO o (O_i - O)))   (0 and 0 where L_i = -inf)
 * -- feed them to fa2_backward_lse of the call that produced part i.  O and dO_i may not alias.  Nothing is allocated, nothing
 * synchronises.  STATUS CODES: a NULL array, tensor or array entry -> FA2_ERR_NULL_POINTER; n_parts outside 1..8 or rows == 0 ->
 * FA2_ERR_INVALID_SHAPE; then FA2_ERR_UNSUPPORTED_HEAD_DIM, FA2_ERR_UNSUPPORTED_DTYPE (bf16 only). */
int fa2_backward_lse(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L, const void* dO,
                     const float* dL, void* dQ, void* dK, void* dV, float* dsink,
                     int B, int H_q, int H_kv, int q_len, int kv_len, int head_dim, float softmax_scale,
                     int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream, int phases);
int fa2_backward_varlen_lse(const void* Q, const void* K, const void* V, const float* sink, const void* O, const float* L,
                            const void* dO, const float* dL, void* dQ, void* dK, void* dV, float* dsink,
                            int H_q, int H_kv, int total_q, int total_k, int head_dim, float softmax_scale, int dtype, int causal,
                            const void* plan_host, const void* plan_dev, size_t plan_bytes,
                            void* workspace, size_t workspace_bytes, void* stream);
int fa2_merge_states(const void* const* O_parts, const float* const* L_parts, int n_parts, void* O, float* L, size_t rows,
                     int head_dim, int dtype, void* stream);
int fa2_merge_states_backward(const void* const* O_parts, const float* const* L_parts, const void* O, const float* L, const void* dO,
                              const float* dL, void* const* dO_parts, float* const* dL_parts, int n_parts, size_t rows, int head_dim,
                              int dtype, void* stream);

/* ---- Decode: one or a few new query tokens per sequence against a preallocated KV cache, the keys split over the GPU.
 * bf16, head_dim 64 or 128, H_q % H_kv == 0, forward only (inference: there is no backward).
 * LAYOUT.  Q, O [B][H_q][q_len][d]; K_cache, V_cache [B][H_kv][kv_capacity][d], contiguous; L [B][H_q][q_len] fp32.
 * seqlens_k: int32 [B] in DEVICE memory, or NULL (every sequence has kv_capacity keys).  Sequence b attends keys [0, len_b) of its
 * own cache rows, len_b = min(max(seqlens_k[b], 0), kv_capacity): the clamp is done in the kernel, no loop bound and no address
 * comes from the stored value.  The host never reads seqlens_k, and nothing the host decides depends on it: a captured graph of
 * this call serves every decode step as the lengths grow.  Cache rows at and beyond len_b may hold anything (NaNs included): they
 * are read as zeros and never enter a product.
 * MASK.  The q_len queries are the sequence's LAST q_len tokens, already in the cache: with causal != 0 key j is visible to query i
 * iff j <= i + len_b - q_len (bottom-right, as everywhere here); causal == 0: every query sees all len_b keys.  A row without a
 * visible key (len_b == 0, or causal with i + len_b - q_len < 0) has O = 0 and L = -inf.
 * sink: fp32 [H_q] DEVICE memory or NULL, the semantics of fa2_forward_sink: L' = logaddexp(L, sink[h]), O scaled by exp(L - L');
 * sink[h] = -inf: no sink for that head; a keyless row has L = sink[h].
 * WORK SPLIT.  One workgroup per (sequence, K/V head, key split); the M = (H_q / H_kv) q_len query rows of a K/V head share one
 * 32-row MFMA tile, so a K/V head is streamed ONCE for its whole group.  1 <= M <= 32; a larger M returns FA2_ERR_UNSUPPORTED:
 * that is a prefill chunk, and fa2_forward_qk takes it.  Split s of n_splits covers keys [s chunk, min((s + 1) chunk, len_b)) with
 * chunk = roundup(ceil(len_b / n_splits), 128), computed on the device; a short sequence leaves its later splits empty.  With
 * n_splits > 1 every split writes an fp32 partial (normalised O_s, L_s) into the workspace and a second kernel on the same
 * stream combines them in ascending s in fp32 (L = logsumexp L_s, O = sum exp(L_s - L) O_s), applies the sink and rounds to bf16
 * once.  With n_splits == 1 the one kernel writes O and L itself and no workspace is needed.  DETERMINISTIC: plain launches, no
 * atomics, no communication between workgroups, every sum in a fixed order.  Nothing is allocated, nothing synchronises.
 * n_splits: 1..256, or 0 = fa2_decode_num_splits(B, H_kv, kv_capacity, head_dim), a pure host function: the smallest s with
 * B H_kv s >= 256 (the MI355X's compute units), limited so that a split of a full cache keeps at least 256 keys, and to 256.
 * fa2_decode_workspace_bytes resolves n_splits == 0 the same way; it is 0 for one split, else n_splits B H_q q_len (d + 1) x 4
 * bytes rounded up to 256.  The workspace must be 16-byte aligned.
 * (O, L) is what fa2_merge_states takes: a cache held in two allocations is two calls (the first with causal = 0 and no sink, the
 * last carrying the mask and the sink) and a merge.
 * STATUS CODES, in this order: NULL Q, K_cache, V_cache, O or L -> FA2_ERR_NULL_POINTER; B, heads, lengths, scale <= 0, H_kv not
 * dividing H_q, n_splits outside 0..256, a (b, head) cache slab of 2 GiB or more (kv_capacity x head_dim x 2 bytes; the whole
 * cache may be larger) -> FA2_ERR_INVALID_SHAPE; FA2_ERR_UNSUPPORTED_HEAD_DIM; FA2_ERR_UNSUPPORTED_DTYPE (bf16 only); workspace
 * NULL, misaligned or too small while the resolved split count is > 1 -> FA2_ERR_WORKSPACE; M > 32 -> FA2_ERR_UNSUPPORTED.
 * NOT COVERED: [B][N][H][d] layouts, M > 32, fp32 caches, a backward, the ring.  (A cache held as a pool of
 * pages with a block table: fa2_forward_decode_paged below; e4m3 caches: the _fp8kv calls below; a sliding window:
 * fa2_forward_decode_window below; WRITING the cache: fa2_kv_append, fa2_kvcache_mi355x.h.) */
int fa2_decode_num_splits(int B, int H_kv, int kv_capacity, int head_dim);
size_t fa2_decode_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, int n_splits);
int fa2_forward_decode(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                       void* O, float* L, int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                       int dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Paged decode: fa2_forward_decode over a KV cache held as a POOL OF PAGES with a per-sequence block table, the way serving
 * stacks hold it.  The same kernels' body, the same split rule, combine, sink, mask and determinism; what differs is where a
 * 32-key tile's rows are found.  bf16, head_dim 64 or 128, forward only.
 * POOL.  K_pages, V_pages [n_pages][H_kv][page_size][d] bf16, contiguous: head-major like every layout here, the rows of one
 * (page, head) are contiguous.  page_size >= 32 and page_size % 32 == 0 (it need not be a power of two): a 32-key tile never
 * crosses a page.  The pool may exceed 4 GiB: a page's address is 64-bit arithmetic, and one buffer resource spans one tile.
 * The pool is only read.
 * TABLE.  block_table: int32 [B][max_pages_per_seq] in DEVICE memory.  Logical key j of sequence b is row j % page_size of page
 * block_table[b][j / page_size].  Entries may repeat, within a sequence and across sequences (shared prefix pages).  The host
 * never reads the table, and nothing the host decides depends on it: a captured graph of this call serves every step as
 * sequences grow into new pages and pages are reassigned, the table and seqlens_k updated in place.
 * CAPACITY.  kv_capacity = max_pages_per_seq x page_size is the logical capacity, and everything fa2_forward_decode says holds
 * with it: len_b = min(max(seqlens_k[b], 0), kv_capacity), clamped in the kernel; seqlens_k == NULL: every sequence has
 * kv_capacity keys; the bottom-right mask; rows without a visible key (O = 0, L = -inf or the sink); sink; n_splits (0 =
 * fa2_decode_num_splits(B, H_kv, kv_capacity, head_dim)); chunk = roundup(ceil(len_b / n_splits), 128); the workspace
 * (fa2_decode_workspace_bytes with that kv_capacity, 16-byte aligned); the combine; (O, L) as fa2_merge_states takes them.  With
 * the same n_splits the result is bit for bit fa2_forward_decode's on the gathered contiguous cache of that capacity: the
 * tiles, their order and every sum are the same.
 * PAGE CLAMP.  A table entry becomes an address only after min(max(entry, 0), n_pages - 1), in the kernel: the length clamp's
 * contract.  An out-of-range entry IN USE gives an unspecified result and no access outside the pool.
 * PAST THE LENGTH.  Table entries for pages at or beyond ceil(len_b / page_size) may hold anything: they are never read, and no
 * table read (prefetches included) falls outside [0, B x max_pages_per_seq).  Rows of the last used page at or beyond len_b, and
 * every unused page, may hold anything, NaNs included: they are read as zeros and never enter a product.
 * STATUS CODES, in this order: NULL Q, K_pages, V_pages, block_table, O or L -> FA2_ERR_NULL_POINTER; B, heads, q_len, n_pages,
 * page_size, max_pages_per_seq or scale <= 0, H_kv not dividing H_q, page_size % 32 != 0, max_pages_per_seq x page_size above
 * INT_MAX - 33024 (the kernel's key arithmetic, up to len_b + (n_splits + 2) x 128, stays in int), n_splits outside 0..256, a grid B H_kv n_splits above INT_MAX -> FA2_ERR_INVALID_SHAPE; FA2_ERR_UNSUPPORTED_HEAD_DIM;
 * FA2_ERR_UNSUPPORTED_DTYPE (bf16 only); workspace NULL, misaligned or too small while the resolved split count is > 1 ->
 * FA2_ERR_WORKSPACE; M = (H_q / H_kv) q_len > 32 -> FA2_ERR_UNSUPPORTED.
 * NOT COVERED: token-major pages [n_pages][page_size][H_kv][d] (permute such a pool once, when it is allocated), page_size 16; and
 * what fa2_forward_decode leaves out: M > 32, a backward, the ring.  (e4m3 pages:
 * fa2_forward_decode_paged_fp8kv below; a sliding window: fa2_forward_decode_paged_window below; WRITING the pool through the same table: fa2_kv_append_paged, fa2_kvcache_mi355x.h.) */
int fa2_forward_decode_paged(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                             const int* seqlens_k, const float* sink, void* O, float* L,
                             int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                             int head_dim, float softmax_scale, int dtype, int causal, int n_splits,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- Decode over fp8 KV caches: fa2_forward_decode and fa2_forward_decode_paged with K and V stored in OCP e4m3
 * (FA2_DTYPE_FP8_E4M3: torch.float8_e4m3fn, gfx950's native encoding; not e5m2, not the fnuz form), one byte per element: half
 * the cache's footprint and half the traffic of a call that is bound by that traffic.  Q and O stay bf16, L fp32; P stays bf16.
 * LAYOUT.  K_cache, V_cache [B][H_kv][kv_capacity][d], K_pages, V_pages [n_pages][H_kv][page_size][d]: the bf16 layouts, one byte
 * per element.  K and V are both e4m3.
 * DESCALES.  k_descale, v_descale: fp32 [H_kv] in DEVICE memory, or NULL (= 1).  The cache holds x / descale[h_kv], so the scores
 * are softmax_scale x k_descale[h] x (Q . K8), O = v_descale[h] x P V8 and L is the log-sum-exp of those scores (then the sink).
 * They are positive and finite by contract; like seqlens_k the kernel reads them when it runs and the host never does, so a
 * captured graph serves a cache whose descales are updated in place.  The kernel widens e4m3 to bf16 in registers (exact), folds
 * k_descale into the scalar every score is multiplied by and multiplies the fp32 result (a split's partial) by v_descale before
 * the one rounding to bf16; both products are the bf16 MFMAs of the bf16 call, so the result is that call's on the dequantised
 * cache up to the rounding of the descaled values to bf16, which this call does not do.
 * EVERYTHING ELSE is the bf16 sibling's, word for word: seqlens_k and its clamp, the bottom-right mask, rows without a key, sink,
 * n_splits and fa2_decode_num_splits, the workspace (fa2_decode_workspace_bytes: the same for both element sizes) and the combine,
 * the block table, its clamp and shared pages, determinism, and paged == contiguous bit for bit at equal n_splits.  Cache bytes
 * at or beyond a length and in unused pages may hold anything, the e4m3 NaN codes 0x7F and 0xFF included: they are read as zeros.
 * dtype is Q's and O's (FA2_DTYPE_BF16); kv_dtype is the caches' (FA2_DTYPE_FP8_E4M3).
 * STATUS CODES: the sibling's, in its order; either dtype other than the above -> FA2_ERR_UNSUPPORTED_DTYPE where the sibling
 * reports its dtype (after the head_dim); the contiguous slab limit is kv_capacity x head_dim x 1 byte below 2 GiB.
 * NOT COVERED: fp8 Q or an fp8 second product, per-token or per-page scales, e5m2, and what the siblings leave out.  (A sliding
 * window over e4m3 caches: the _window calls below.  The quantising append that writes these caches with these descales: fa2_kv_append, fa2_kv_append_paged, fa2_kvcache_mi355x.h.) */
int fa2_forward_decode_fp8kv(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                             const float* k_descale, const float* v_descale, void* O, float* L,
                             int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                             int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream);
int fa2_forward_decode_paged_fp8kv(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                                   const int* seqlens_k, const float* sink, const float* k_descale, const float* v_descale,
                                   void* O, float* L,
                                   int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                                   int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- Decode with a sliding window: the four calls above (bf16 or e4m3 caches, contiguous or paged) for a layer that sees only
 * the last keys, the way GPT-OSS (128 keys and a sink), Mistral and Gemma layers do.  The same kernels' body with a lower bound
 * on the key range; the combine, the sink (applied after the combine), GQA (M <= 32), determinism and "nothing allocated, nothing
 * synchronised" are the siblings'.
 * WINDOW.  window_left is the number of keys BEFORE a query's own position that it sees.  With pos_i = i + len_b - q_len (the
 * bottom-right position used everywhere here) key j is visible to query i iff pos_i - window_left <= j <= pos_i.  A model's
 * sliding_window = 128 "including itself" is window_left = 127; flash-attn's window_size = (left, 0) is window_left = left.
 * window_left = -1: no window.  The window is a causal one: window_left >= 0 with causal == 0 returns FA2_ERR_UNSUPPORTED.  A row
 * with pos_i < 0 has no key, as in the siblings: O = 0, L = -inf or the sink.  window_left may be INT_MAX.
 * KEY RANGE.  lo_b = max(0, len_b - q_len - window_left) is the lowest key any row of sequence b may see.  The splits share
 * [base_b, len_b), base_b = rounddown(lo_b, 128): chunk = roundup(ceil((len_b - base_b) / n_splits), 128) and split s covers
 * [base_b + s chunk, min(base_b + (s + 1) chunk, len_b)), computed on the device from len_b.  Splits start on multiples of 128 and
 * the 32-key tiles are those of the plain call, so with q_len == 1 and lo_b a multiple of 128 the result is bit for bit the plain
 * call's on the cache rows from lo_b on, at equal n_splits.  The host reads neither lengths nor table nor descales: one captured
 * graph serves every step as the lengths grow and the window slides.
 * BEFORE THE WINDOW (the "past the length" contract, mirrored).  Cache rows below lo_b may hold anything, NaNs and the e4m3 NaN
 * codes included.  Paged: every table entry of a page that lies wholly below lo_b may hold anything (stale, -1, out of range): it
 * is never read, prefetches included, which is what lets a server free the pages behind the window.  Tiles wholly below lo_b are
 * not loaded; the one 32-key tile that straddles lo_b lies in a page that holds a visible key, and its rows below lo_b never
 * reach a product as data (K's scores are selected away, V's rows are zeroed in registers).  Rows in [lo_b, len_b) are real data.
 * n_splits: 1..256, or 0 = fa2_decode_window_num_splits(B, H_kv, q_len, kv_capacity, head_dim, window_left), a pure host function:
 * fa2_decode_num_splits on min(kv_capacity, window_left + q_len + 127), the most keys a sequence's splits can share.  Pass its
 * result to fa2_decode_workspace_bytes as n_splits.
 * ROUTING.  window_left == -1 or window_left >= kv_capacity - 1 excludes no key of any length: the call IS the sibling's, its
 * kernels and its default split count, bit for bit (fa2_decode_window_num_splits then equals fa2_decode_num_splits).
 * dtype is Q's and O's (FA2_DTYPE_BF16); kv_dtype is the caches', FA2_DTYPE_BF16 or FA2_DTYPE_FP8_E4M3.  k_descale, v_descale: as
 * in the _fp8kv calls, NULL = 1; they belong to e4m3 caches, and a non-NULL one beside a bf16 cache is refused.
 * STATUS CODES: the siblings', in their order; window_left < -1 -> FA2_ERR_INVALID_SHAPE, the last of the shape checks; a kv_dtype
 * other than the two, or a descale beside a bf16 cache -> FA2_ERR_UNSUPPORTED_DTYPE where the siblings report their dtype;
 * window_left >= 0 with causal == 0 -> FA2_ERR_UNSUPPORTED, after M > 32.
 * NOT COVERED: non-causal and right-sided windows, a window in the training forward or backward, a ring-buffer (modulo) cache
 * layout, a window per sequence or per head, and what the siblings leave out (M > 32, a backward, the ring). */
int fa2_decode_window_num_splits(int B, int H_kv, int q_len, int kv_capacity, int head_dim, int window_left);
int fa2_forward_decode_window(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                              const float* k_descale, const float* v_descale, void* O, float* L,
                              int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                              int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream,
                              int window_left);
int fa2_forward_decode_paged_window(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                                    const int* seqlens_k, const float* sink, const float* k_descale, const float* v_descale,
                                    void* O, float* L,
                                    int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                                    int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                                    void* workspace, size_t workspace_bytes, void* stream, int window_left);

/* fa2_backward restricted to some of its kernels -- bit 0: D = rowsum(dO o O) and the row constants into the
 * workspace, bit 1: the dQ kernel, bit 2: the dK/dV kernel, bit 3: the single five-product kernel and its output
 * pass (FA2_ERR_UNSUPPORTED for shapes or devices it does not take, and in combination with bits 1 or 2).  7 = fa2_backward (which picks the implementation);
 * 6 = the two-kernel form whatever the shape.  For profiling and for callers that overlap the two independent
 * kernels on separate streams; bits 1, 2 and 3 need what bit 0 produced in the same workspace. */
int fa2_backward_phases(const void* Q, const void* K, const void* V, const void* O, const float* L,
                        const void* dO, void* dQ, void* dK, void* dV,
                        int B, int H, int seq_len, int head_dim, float softmax_scale,
                        int dtype, int causal, void* workspace, size_t workspace_bytes, void* stream,
                        int phases);

/* The backward of a rectangular BLOCK of the score matrix: q_len query rows (a row range of every head,
 * consecutive heads q_head_stride rows apart in Q / O / dO / dQ / L; 0 = q_len) against kv_len keys (K / V /
 * dK / dV, heads kv_head_stride rows apart; 0 = kv_len).  dQ = this block's contribution to the rows' dQ,
 * dK / dV = the rows' contribution to the keys' gradients; L must be the log-sum-exp over ALL keys of the
 * row (not only this block's), which is what makes blocks add up -- the unit of work of the ring backward.
 * With causal != 0 key j is visible to local query i iff j <= i + causal_shift.  The workspace is
 * fa2_backward_workspace_bytes(B, H, q_head_stride ? q_head_stride : q_len, ...): its planes are dense
 * [B][H][q_head_stride] and the block's rows are rows [q_row0, q_row0 + q_len) of every head (the tensor
 * pointers address row q_row0 of head 0), so phase bit 0 (D = rowsum(dO o O)) may be run once over the
 * dense local tensors (q_row0 = 0, q_len = q_head_stride) and reused by every block of them.  bf16 only.
 * fa2_backward is the block q_len = kv_len = seq_len, strides 0, q_row0 0, shift 0.
 * phases as fa2_backward_phases bits 0..2.  With bits 1 and 2 both set (6 or 7) the block runs the single five-product kernel
 * where the routing rule of fa2_backward (its block shapes included) takes it, the dQ and dK/dV kernels otherwise.  A single
 * bit (2 or 4) always runs that kernel.
 * FA2_PHASE_LEAVE_ROOM (bit 4) asks the single kernel to leave some of the device's CUs free: its persistent workgroups fill a
 * CU's register file for the whole launch, so a kernel on another stream that must run CONCURRENTLY (the ring backward's RCCL
 * exchange of the previous step's dK / dV pieces) would otherwise wait for the launch to end.  How many: bits 8..15 of
 * `phases`, FA2_PHASE_LEAVE_CUS(n) with 1 <= n <= 255; 0 there (plain FA2_PHASE_LEAVE_ROOM) = 16.  A run-time argument, so
 * that a multi-GPU run can tune it without a rebuild (fa2_ring_ctx_set_reserved_cus).  No effect on the results. */
#define FA2_PHASE_LEAVE_ROOM 16
#define FA2_PHASE_LEAVE_CUS(n) (FA2_PHASE_LEAVE_ROOM | (((n) & 0xff) << 8))
int fa2_backward_block(const void* Q, const void* K, const void* V, const void* O, const float* L,
                       const void* dO, void* dQ, void* dK, void* dV,
                       int B, int H, int q_len, int kv_len, int head_dim, float softmax_scale, int dtype,
                       int q_head_stride, int kv_head_stride, int q_row0, int causal, int causal_shift,
                       void* workspace, size_t workspace_bytes, void* stream, int phases);

/* The single-kernel five-product backward (csrc/fa2_bwd_fused.hip) with the way dQ is summed over the key-block
 * workgroups of a head chosen by the caller -- mode 1: handed from key block to key block in a fixed order by a
 * persistent grid (deterministic; what fa2_backward uses), mode 0: fp32 atomics (NOT bit-reproducible; kept as the
 * measured alternative; seq_len a multiple of 256 and d = 128 only).  bf16, non-causal (fa2_backward
 * also takes the causal case), a head_dim and seq_len that rule (a) of fa2_backward admits, mode 1 only on the device of rule
 * (c); FA2_ERR_UNSUPPORTED otherwise.  FA2_BACKWARD_PATH does not apply.  Workspace: fa2_backward_fused_workspace_bytes (= fa2_backward_workspace_bytes). */
size_t fa2_backward_fused_workspace_bytes(int B, int H, int seq_len, int head_dim);
int fa2_backward_fused(const void* Q, const void* K, const void* V, const void* O, const float* L,
                       const void* dO, void* dQ, void* dK, void* dV,
                       int B, int H, int seq_len, int head_dim, float softmax_scale, int mode,
                       void* workspace, size_t workspace_bytes, void* stream);

/* One resumable forward step: folds the kv_len keys/values of a resident shard into the running
 * state of q_len local query rows -- the unit of work of ring_attention_forward_kernel
 * (ring_attention_kernel.cu:13-140).  State between steps: Mrun = running max (natural units),
 * L = running sum l, and the un-normalised accumulator -- for bf16 in Oacc (fp32
 * [B][H][q_len][d]), for fp32 in O itself (Oacc ignored), as the reference keeps it (:125-137).
 * first != 0 starts from (0, 0, -inf) instead of loading the state; last != 0 writes
 * O = acc / l and L = m + ln l (:112-124) instead of storing the state.  Non-causal. */
int fa2_forward_step(const void* Q, const void* K, const void* V,
                     void* O, float* L, float* Oacc, float* M,
                     int B, int H, int q_len, int kv_len, int head_dim, float softmax_scale,
                     int dtype, int first, int last, void* stream);

/* fa2_forward_step (bf16 only) over a ROW RANGE of every head: consecutive heads are q_head_stride rows
 * apart in Q / O / Oacc / L / M and kv_head_stride rows apart in K / V (0 = q_len / kv_len, dense); the
 * pointers address the first row of the range in head 0.  With causal != 0 key j is visible to local
 * query i iff j <= i + causal_shift.  This is the unit of work of the causal zig-zag ring, where a
 * step folds half of the local keys into all local rows, or all of them into half of the rows. */
int fa2_forward_step_strided(const void* Q, const void* K, const void* V,
                             void* O, float* L, float* Oacc, float* M,
                             int B, int H, int q_len, int kv_len, int head_dim, float softmax_scale,
                             int dtype, int first, int last, int q_head_stride, int kv_head_stride,
                             int causal, int causal_shift, void* stream);

/* Turns the bf16 step state of `rows` consecutive rows into results: O = acc / l (bf16), L = m + ln l
 * (on entry L holds l) -- what last != 0 does inside a step, for schedules whose last step does not
 * touch every row. */
int fa2_forward_state_finalize(void* O, float* L, const float* Oacc, const float* M,
                               size_t rows, int head_dim, int dtype, void* stream);

/* acc[i] = (init ? 0 : acc[i]) + src[i] for n bf16 values: fp32 running sums of bf16 contributions (the
 * ring backward adds each step's gradients this way). */
int fa2_accumulate_bf16(float* acc, const void* src, size_t n, int init, void* stream);
/* The same over `rows` runs of `cols` contiguous elements that start `pitch` elements apart in both acc and
 * src (a row range of every head of a [B][H][N][d] tensor). */
int fa2_accumulate_bf16_2d(float* acc, const void* src, size_t rows, size_t cols, size_t pitch, int init, void* stream);

/* Measurement aid: a small kernel on `stream` writes, for every XCC x of the device it reaches (x = HW_REG_XCC_ID < 16), two
 * 64-bit device counters to out32[2 x], out32[2 x + 1] (DEVICE memory, 32 x 8 = 256 bytes, 16-byte aligned, zeroed by the
 * caller: an XCC the device does not have keeps zeros, and each slot takes the MAXIMUM over the XCC's workgroups): shader-clock
 * ticks (s_memtime: every CU has a counter of its own, offset from its neighbours'; the maximum over all CUs of an XCC is the
 * same CU's in every sample, so only differences taken on the SAME XCC mean anything) and ticks of the constant 100 MHz
 * reference (s_memrealtime).  Bracket a
 * stretch of work with two calls into two buffers: per XCC, d(ticks) / d(reference ticks) x 100 MHz is the mean shader clock
 * it held over the stretch (cuda_flashattention_amd.ops.mean_shader_clock_mhz averages the XCCs present in both). */
int fa2_read_clocks(unsigned long long* out32, void* stream);

/* Measurement aid: `workgroups` workgroups of four waves (one per SIMD) each run 4 x iters back-to-back
 * v_mfma_f32_32x32x16_bf16 on the operands at `operands` (DEVICE memory, 1024 x 16 bytes of bf16 the caller fills -- random
 * values: the clock a device holds depends on the data) and write workgroups x 256 floats to `out`.  4 x iters x workgroups x 4 x
 * 32768 flops: timed by the caller with one workgroup per CU, it is what THIS device sustains on bare MFMAs -- the ceiling
 * bench.py reports beside the nominal peak, because devices of one pool differ by several per cent on power-limited kernels. */
int fa2_mfma_probe(const void* operands, float* out, int iters, int workgroups, void* stream);

/* Element-wise helpers (grid-stride, HBM-bound). */
int fa2_fill_f32(float* dst, size_t n, float value, void* stream);      /* init_array, cuda_helper.h:60-65 */
int fa2_convert_f32_to_bf16(const float* src, void* dst, size_t n, void* stream);
int fa2_convert_bf16_to_f32(const void* src, float* dst, size_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_MI355X_H */
