/*
 * fa2_mla_sparse_mi355x.h -- C ABI of SPARSE MLA DECODE ATTENTION (libfa2_mi355x.so, csrc/fa2_mla_decode.hip): the absorbed-form
 * MLA decode of fa2_mla_mi355x.h over a SET of cache rows per query token, named by an index tensor (DeepSeek-V3.2's lightning
 * indexer picks the top-k cache rows of a token, shared by all its heads), for contiguous and paged bf16 latent caches.
 *
 * SEMANTICS.  Q, the cache, seqlens_k, block_table, O, L, softmax_scale and causal mean what fa2_mla_mi355x.h says: Q
 * [B][H][q_len][576] bf16; the latent cache [B][kv_capacity][576] bf16, or a pool [n_pages][page_size][576] with block_table
 * [B][max_pages_per_seq] (page_size % 32 == 0, an entry in use clamped to [0, n_pages), the pool may exceed 4 GiB);
 *   indices int32 [B][q_len][topk], dense, DEVICE, topk >= 1 and NOT required to be a multiple of 32.  Entry (b, i, t) is a LOGICAL
 *   key position of sequence b: the cache row, or the position that goes through the block table.  One index row serves all H
 *   heads of query token i.
 *   Entry j = indices[b][i][t] is LIVE iff 0 <= j < len_b (len_b the clamped seqlens_k[b], or kv_capacity when it is NULL) and,
 *   when causal, j <= i + len_b - q_len.  An entry that is not live (-1 padding, a stale position, garbage, INT_MIN, INT_MAX)
 *   contributes nothing: neither its cache row nor its table entry is read.  Cache rows past a length, and rows no live index
 *   names, may hold NaNs; a table entry is read only for a live index.
 *   DUPLICATES in an index row are counted once per occurrence: a position named twice has twice the weight.
 *   S = softmax_scale x Q C[j]^T over 576 columns for the live j; O [B][H][q_len][512] bf16 = softmax(S) C[j, :512]; L
 *   [B][H][q_len] fp32, the natural-log LSE.  A row with no live entry has O = 0 and L = -inf.
 * The call is deterministic (no atomics, no waits between workgroups), allocates nothing and does not synchronise; the host reads
 * no length, index or table, so one captured graph serves every step with indices and seqlens_k rewritten in place.
 *
 * WORK SPLIT.  A workgroup is (sequence b, query token i, block of 32 heads, slot split): the split runs over the SLOT LIST, not
 * the keys.  Split s covers slots [s chunk, min((s + 1) chunk, topk)), chunk = roundup(ceil(topk / n_splits), 32): topk is a host
 * value, nothing about the split is computed from a length.  With n_splits >= 2 every split writes an fp32 partial (O_s [512],
 * L_s; -inf without a live slot) into the workspace and the dense decode's combine folds them in ascending s with ONE rounding.
 * fa2_mla_sparse_num_splits: the default (n_splits = 0), the family's rule with the slot count in place of the capacity:
 * min(ceil(256 / (B x q_len x ceil(H / 32))), max(1, topk / 256), 256).  Invalid arguments: 1.
 * fa2_mla_sparse_workspace_bytes: fa2_mla_decode_workspace_bytes' layout and formula: 0 for one split (and for invalid arguments
 * or a size above SIZE_MAX / 2), else n_splits x B x H x q_len x (512 + 1) x 4 rounded up to 256.  16-byte aligned.
 *
 * STATUS CODES, in this order, all decided before any HIP call: NULL Q, cache, indices, O, L or block_table ->
 * FA2_ERR_NULL_POINTER; B, H, q_len, topk <= 0, softmax_scale not > 0, kv_capacity (n_pages, page_size, max_pages_per_seq) <= 0,
 * page_size % 32 != 0, a capacity above INT_MAX - 33024 keys (paged) or a contiguous sequence above INT_MAX bytes, topk above
 * INT_MAX - 33024, n_splits outside 0..256, B x H x q_len above INT_MAX - 32 -> FA2_ERR_INVALID_SHAPE; (kv_lora_rank, rope_dim)
 * other than (512, 64) -> FA2_ERR_UNSUPPORTED_HEAD_DIM; the grid B x q_len x ceil(H / 32) x n_splits above INT_MAX or a workspace
 * size that overflows -> FA2_ERR_INVALID_SHAPE; n_splits > 1 with a workspace that is NULL, too small or not 16-byte aligned ->
 * FA2_ERR_WORKSPACE.
 *
 * NOT COVERED: e4m3 latent caches under indices, physical pool-slot indices, an index row per head, the indexer itself, sinks
 * and windows, a backward.
 */
#ifndef FA2_MLA_SPARSE_MI355X_H
#define FA2_MLA_SPARSE_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_mla_sparse_num_splits(int B, int H, int q_len, int topk, int kv_lora_rank, int rope_dim);
size_t fa2_mla_sparse_workspace_bytes(int B, int H, int q_len, int topk, int kv_lora_rank, int rope_dim, int n_splits);

int fa2_forward_mla_decode_sparse(const void* Q, const void* ckv_cache, const int* indices, const int* seqlens_k, void* O, float* L,
                                  int B, int H, int q_len, int topk, int kv_capacity, int kv_lora_rank, int rope_dim,
                                  float softmax_scale, int causal, int n_splits, void* workspace, size_t workspace_bytes,
                                  void* stream);

int fa2_forward_mla_decode_sparse_paged(const void* Q, const void* ckv_pages, const int* block_table, const int* indices,
                                        const int* seqlens_k, void* O, float* L, int B, int H, int q_len, int topk, int n_pages,
                                        int page_size, int max_pages_per_seq, int kv_lora_rank, int rope_dim, float softmax_scale,
                                        int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_MLA_SPARSE_MI355X_H */
