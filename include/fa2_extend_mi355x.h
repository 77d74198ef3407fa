/*
 * fa2_extend_mi355x.h -- C ABI of EXTEND ATTENTION (libfa2_mi355x.so, csrc/fa2_extend.hip, kernels in csrc/fa2_decode.hip): the
 * decode calls of fa2_mi355x.h for ANY number of query rows per K/V head.  "Extend" is the serving stacks' name for queries
 * appended to a cache: speculative-decoding verification, MQA and wide groups at q_len 1, chunked prefill and prefix-cache hits
 * over a paged or e4m3 cache.  The caches are the ones fa2_kv_append (fa2_kvcache_mi355x.h) writes.
 *
 * SEMANTICS.  fa2_forward_extend is fa2_forward_decode_window and fa2_forward_extend_paged is fa2_forward_decode_paged_window,
 * argument for argument and word for word (fa2_mi355x.h), without the limit (H_q / H_kv) x q_len <= 32:
 *   Q, O [B][H_q][q_len][d] bf16, L [B][H_q][q_len] fp32, d 64 or 128, H_q % H_kv == 0; dtype is Q's (FA2_DTYPE_BF16);
 *   caches bf16 or OCP e4m3 (kv_dtype) with k_descale, v_descale (fp32 [H_kv], DEVICE, NULL = 1; refused beside bf16 caches);
 *   contiguous [B][H_kv][kv_capacity][d], or a pool [n_pages][H_kv][page_size][d] with an int32 block table
 *   [B][max_pages_per_seq] (page_size % 32 == 0, kv_capacity = max_pages_per_seq x page_size);
 *   seqlens_k (int32 [B], DEVICE, or NULL = kv_capacity) is read and clamped to [0, kv_capacity] on the device; the q_len
 *   queries are the sequence's last q_len tokens, already in the cache; causal is the bottom-right mask (key j visible to
 *   query i iff j <= i + len_b - q_len); window_left is -1 (none) or >= 0 (keys pos_i - window_left .. pos_i, causal only);
 *   sink (fp32 [H_q], DEVICE, or NULL) as fa2_forward_sink; a row without a visible key has O = 0 and L = -inf (L = sink with
 *   one); rows past a length and before the window may hold anything, NaNs included, and table entries there are never read;
 *   a table entry in use is clamped to [0, n_pages).
 * The call is deterministic, allocates nothing and does not synchronise; the host reads no length, table or descale, so one
 * captured graph of {append, extend} serves every step.  (O, L) is what fa2_merge_states takes.
 *
 * ROUTING.  M = (H_q / H_kv) x q_len <= 32: the call IS the sibling's (fa2_forward_decode_window / _paged_window): its kernels,
 * its default split count, bit for bit.  M > 32: the extend kernels.  A workgroup is (sequence, K/V head, block of 64 rows,
 * split); the rows of a group are the contiguous slab [H_q / H_kv][q_len], block j owning rows 64 j .. 64 j + 63, and every wave
 * carries two 32-row MFMA tiles, so the K/V head is streamed once per 64 rows.  The split ranges are the siblings' (from len_b,
 * on the device, shared by the blocks of a sequence); a block skips the key tiles none of its rows sees (behind the largest
 * kmax of its rows; under a window, before the tile of the smallest kmin).  A row's arithmetic does not depend on its tile or
 * block: with the same n_splits a row's O and L are bit for bit what the sibling gives for it when called on a slice of at most
 * 32 rows (one group member at a time, the same q_len).  n_splits >= 2: fp32 partials in the workspace and the siblings' combine
 * launch.
 * fa2_extend_num_splits: the default (n_splits = 0), pure host arithmetic: M <= 32: fa2_decode_window_num_splits.  Otherwise the
 * siblings' rule on B x H_kv x ceil(M / 64) workgroups: min(ceil(256 / workgroups), max(1, span / 256), 256), span = kv_capacity,
 * or min(kv_capacity, window_left + q_len + 127) under a window that can exclude a key (window_left < kv_capacity - 1).  A
 * prefill chunk (256 workgroups or more) resolves to one split and needs no workspace.  Invalid arguments: 1.
 * fa2_extend_workspace_bytes: 0 for one split (and for invalid arguments or a size above SIZE_MAX / 2), else
 * n_splits x B x H_q x q_len x (head_dim + 1) x 4 rounded up to 256; n_splits = 0 is the default above.  16-byte aligned.
 *
 * STATUS CODES, the siblings' in the siblings' order, all decided before any HIP call: NULL Q, K, V, O, L or block_table ->
 * FA2_ERR_NULL_POINTER; B, H_q, q_len, head_dim <= 0, softmax_scale not > 0, B x H_q above INT_MAX / 64, q_len x head_dim x 4
 * above INT_MAX, H_q % H_kv != 0, kv_capacity (n_pages, page_size, max_pages_per_seq) <= 0, page_size % 32 != 0,
 * max_pages_per_seq x page_size above INT_MAX - 33024, n_splits outside 0..256, a contiguous (b, head) slab above INT_MAX bytes,
 * window_left < -1, B x H_q x q_len above INT_MAX - 64 -> FA2_ERR_INVALID_SHAPE; head_dim other than 64 or 128 ->
 * FA2_ERR_UNSUPPORTED_HEAD_DIM; dtype not bf16, kv_dtype neither bf16 nor e4m3, a descale beside a bf16 cache ->
 * FA2_ERR_UNSUPPORTED_DTYPE; the grid B x H_kv x ceil(M / 64) x n_splits above INT_MAX or a workspace size that overflows ->
 * FA2_ERR_INVALID_SHAPE; n_splits > 1 with a workspace that is NULL, too small or not 16-byte aligned -> FA2_ERR_WORKSPACE;
 * window_left >= 0 without causal -> FA2_ERR_UNSUPPORTED.  There is no row limit.
 * AGAINST fa2_forward_qk.  A caller whose cache is contiguous bf16 with equal lengths could also call fa2_forward_qk on it.  Measured
 * on one MI355X (profiles/extend_times.json, d = 128): that call takes 1.35 - 1.41 times this one's time at q_len = 512 (32 heads on 8,
 * 8192 and 32768 keys) and 8 - 40 times at q_len 8 and 1; no measured q_len favours it.
 * A q_len PER SEQUENCE (ragged batches, cu_seqlens_q) and token-major Q / O are fa2_forward_extend_ragged / _paged
 * (fa2_extend_ragged_mi355x.h): these calls give all B sequences one q_len and take Q, O as [B][H_q][q_len][d].
 * NOT COVERED: tree masks for speculative decoding, a backward, token-major pools, and what the siblings leave out: per-token
 * or per-page scales, e5m2, pages that are no multiple of 32 keys, head dims other than 64 and 128, fp8 queries.
 */
#ifndef FA2_EXTEND_MI355X_H
#define FA2_EXTEND_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_extend_num_splits(int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, int window_left);
size_t fa2_extend_workspace_bytes(int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, int n_splits,
                                  int window_left);

int fa2_forward_extend(const void* Q, const void* K_cache, const void* V_cache, const int* seqlens_k, const float* sink,
                       const float* k_descale, const float* v_descale, void* O, float* L,
                       int B, int H_q, int H_kv, int q_len, int kv_capacity, int head_dim, float softmax_scale,
                       int dtype, int kv_dtype, int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream,
                       int window_left);

int fa2_forward_extend_paged(const void* Q, const void* K_pages, const void* V_pages, const int* block_table,
                             const int* seqlens_k, const float* sink, const float* k_descale, const float* v_descale,
                             void* O, float* L,
                             int B, int H_q, int H_kv, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                             int head_dim, float softmax_scale, int dtype, int kv_dtype, int causal, int n_splits,
                             void* workspace, size_t workspace_bytes, void* stream, int window_left);

#ifdef __cplusplus
}
#endif
#endif /* FA2_EXTEND_MI355X_H */
