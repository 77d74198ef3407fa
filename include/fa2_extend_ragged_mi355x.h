/*
 * fa2_extend_ragged_mi355x.h -- C ABI of RAGGED EXTEND ATTENTION (libfa2_mi355x.so, csrc/fa2_extend_ragged.hip, kernels in
 * csrc/fa2_decode.hip): extend attention (fa2_extend_mi355x.h) with a q_len PER SEQUENCE and TOKEN-MAJOR Q, O and L -- one call
 * for a continuous-batching step that mixes prompt chunks, speculative verification and plain decodes.
 *
 * SEMANTICS.  fa2_forward_extend_ragged is fa2_forward_extend and fa2_forward_extend_ragged_paged is fa2_forward_extend_paged,
 * word for word (fa2_extend_mi355x.h, fa2_mi355x.h), with two differences.
 * 1. A q_len per sequence.  cu_seqlens_q (int32 [B + 1], DEVICE): sequence b owns tokens cu[b] .. cu[b + 1] - 1 of the packed
 *    batch, q_b = cu[b + 1] - cu[b]; q_b = 0 is allowed (nothing is read or written for that sequence).  The host passes
 *    total_q = T only, the number of packed tokens and the size of Q, O and L; it reads no cu_seqlens_q, length, table or
 *    descale, so one captured graph of {plan, ragged extend} serves every step while the mix changes.  Everything the siblings
 *    define with q_len uses q_b: the q_b queries are the sequence's last q_b cached tokens, key j is visible to token i iff
 *    j <= i + len_b - q_b, pos_i = i + len_b - q_b, lo_b = max(0, len_b - q_b - window_left), and a row with pos_i < 0 has
 *    O = 0 and L = -inf (or the sink).
 * 2. Token-major rows.  Q is bf16 [T][H_q][d] with q_token_stride elements between tokens (>= H_q x d and a multiple of 8: the
 *    Q slice of a fused QKV output goes in as it is), O bf16 [T][H_q][d] contiguous, L fp32 [T][H_q].  Row (token t, head h) has
 *    flat index t x H_q + h: the row order fa2_merge_states takes.
 * Everything else is the siblings': caches bf16 or e4m3 with device-side descales, contiguous [B][H_kv][kv_capacity][d] or a pool
 * with a block table; seqlens_k clamped on the device; the sink; window_left -1 or >= 0 (causal only); garbage allowed past a
 * length and before the window; table entries clamped; deterministic, no allocation, no synchronisation.
 *
 * THE PLAN.  The host cannot size a grid from the q_b, so a small kernel runs first, ONE launch per step (it depends on
 * cu_seqlens_q and G = H_q / H_kv only: a model builds it once per step and every layer reuses it):
 *   fa2_extend_ragged_plan(cu_seqlens_q, B, H_q, H_kv, total_q, plan, plan_bytes, stream)
 * writes into the caller's buffer (int32, 16-byte aligned, fa2_extend_ragged_plan_bytes): a header of 8 ints (B, G, T, the
 * number of work items, the first owned token, one past the last owned token, 0, 0); per sequence a sanitised (start_b, q_b);
 * and the list of work items (b, row block), one per 64 rows of a sequence's [G][q_b] slab, in order of b, the unused tail
 * marked (-1, 0).  fa2_extend_ragged_max_blocks = floor(G x T / 64) + min(B, T) bounds the items on the host, and the attention
 * grid is max_blocks x H_kv x n_splits (the split innermost); a workgroup reads its item with scalar loads and leaves at once
 * on a tail entry.
 * THE PLAN IS THE SAFETY CONTRACT.  The attention kernels read (start_b, q_b) from the plan and never from cu_seqlens_q.  The
 * plan kernel stores the running maximum of cu clamped to [0, T]: c_i = clamp(max(cu[0..i]), 0, T), start_b = c_b,
 * q_b = c_{b+1} - c_b.  Whatever the caller's tensor holds: 0 <= start_b, start_b + q_b <= T, the sum of the q_b is at most T,
 * the work items number at most max_blocks.  A cu_seqlens_q that is not non-decreasing within [0, T] is the CALLER'S ERROR
 * with this defined outcome (a decreasing entry gives an empty sequence, an entry out of range is clamped).  A plan whose
 * header does not name the call's B, G and T (built for another batch, or never built) makes every workgroup leave without
 * a store; a plan entry out of range does the same for its workgroup.  Tokens of no sequence (below cu[0], from cu[B] on) keep
 * what O and L held.
 *
 * ROUTING.  Every sequence runs the extend kernels' arithmetic (fa2_extend_mi355x.h): a workgroup is (work item, K/V head,
 * split), two 32-row tiles per wave, the split ranges from len_b on the device, the block's clip from q_b.  A sequence with
 * G x q_b <= 32 runs through the same two-tile body with the second tile as padding.  With the same n_splits a row's O and L are
 * bit for bit what fa2_forward_extend / _paged gives for it when called on that sequence alone (B = 1, q_len = q_b).
 * n_splits >= 2: fp32 partials [n_splits][T x H_q] in the workspace and a combine launch over the owned tokens' rows.
 * fa2_extend_ragged_num_splits (n_splits = 0), pure host arithmetic: min(ceil(256 / workgroups), max(1, span / 256), 256) with
 * workgroups = H_kv x max(min(B, total_q), ceil(G x total_q / 64)) and span = kv_capacity, or min(kv_capacity, window_left +
 * total_q + 127) under a window that can exclude a key (window_left < kv_capacity - 1).  Invalid arguments: 1.
 * fa2_extend_ragged_workspace_bytes: 0 for one split (and for invalid arguments), else n_splits x total_q x H_q x (head_dim + 1)
 * x 4 rounded up to 256; n_splits = 0 is the default above.  16-byte aligned.
 * fa2_extend_ragged_plan_bytes: (8 + 2 x B + 2 x max_blocks) x 4 rounded up to 16; 0 for invalid arguments.
 *
 * STATUS CODES, the siblings' in the siblings' order, all decided before any HIP call: NULL Q, K, V, O, L, block_table or plan
 * (fa2_extend_ragged_plan: NULL cu_seqlens_q or plan) -> FA2_ERR_NULL_POINTER; B, H_q, total_q, head_dim <= 0, softmax_scale not
 * > 0, B x H_q above INT_MAX / 64, H_q % H_kv != 0, q_token_stride below H_q x head_dim or no multiple of 8, kv_capacity (n_pages,
 * page_size, max_pages_per_seq) <= 0, page_size % 32 != 0, max_pages_per_seq x page_size above INT_MAX - 33024, n_splits outside
 * 0..256, a contiguous (b, head) slab above INT_MAX bytes, window_left < -1, total_q x H_q above INT_MAX - 64 ->
 * FA2_ERR_INVALID_SHAPE; head_dim other than 64 or 128 -> FA2_ERR_UNSUPPORTED_HEAD_DIM; dtype not bf16, kv_dtype neither bf16 nor
 * e4m3, a descale beside a bf16 cache -> FA2_ERR_UNSUPPORTED_DTYPE; the grid max_blocks x H_kv x n_splits above INT_MAX or a
 * workspace size that overflows -> FA2_ERR_INVALID_SHAPE; plan_bytes below fa2_extend_ragged_plan_bytes or a plan that is not
 * 16-byte aligned -> FA2_ERR_WORKSPACE; n_splits > 1 with a workspace that is NULL, too small or not 16-byte aligned ->
 * FA2_ERR_WORKSPACE; window_left >= 0 without causal -> FA2_ERR_UNSUPPORTED.
 * NOT COVERED: in THIS header a ragged KV append or a ragged rotary append (n_new per sequence): the step's other half, driven by
 * the same plan, is fa2_rope_kv_append_ragged (fa2_rope_ragged_mi355x.h); tree masks for speculative decoding, a
 * backward, token-major pools, a longest-first order of the work items, a one-tile instantiation for sequences of at most 32
 * rows, and what the siblings leave out.
 */
#ifndef FA2_EXTEND_RAGGED_MI355X_H
#define FA2_EXTEND_RAGGED_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

long long fa2_extend_ragged_max_blocks(int B, int H_q, int H_kv, int total_q);
size_t fa2_extend_ragged_plan_bytes(int B, int H_q, int H_kv, int total_q);
int fa2_extend_ragged_plan(const int* cu_seqlens_q, int B, int H_q, int H_kv, int total_q, void* plan, size_t plan_bytes,
                           void* stream);
int fa2_extend_ragged_num_splits(int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, int window_left);
size_t fa2_extend_ragged_workspace_bytes(int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, int n_splits,
                                         int window_left);

int fa2_forward_extend_ragged(const void* Q, long long q_token_stride, const void* K_cache, const void* V_cache,
                              const void* plan, size_t plan_bytes, const int* seqlens_k, const float* sink,
                              const float* k_descale, const float* v_descale, void* O, float* L,
                              int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim, float softmax_scale,
                              int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes,
                              void* stream, int window_left);

int fa2_forward_extend_ragged_paged(const void* Q, long long q_token_stride, const void* K_pages, const void* V_pages,
                                    const int* block_table, const void* plan, size_t plan_bytes, const int* seqlens_k,
                                    const float* sink, const float* k_descale, const float* v_descale, void* O, float* L,
                                    int B, int H_q, int H_kv, int total_q, int n_pages, int page_size, int max_pages_per_seq,
                                    int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                                    void* workspace, size_t workspace_bytes, void* stream, int window_left);

#ifdef __cplusplus
}
#endif
#endif /* FA2_EXTEND_RAGGED_MI355X_H */
