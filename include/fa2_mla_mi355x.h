/*
 * fa2_mla_mi355x.h -- C ABI of MLA DECODE ATTENTION (libfa2_mi355x.so, csrc/fa2_mla_decode.hip): a decode step of multi-head
 * latent attention (DeepSeek-V2 / V3 / R1, Kimi K2) in absorbed form, which is multi-query attention over ONE latent cache row
 * per token.  A cache row is kv_lora_rank + rope_dim = 512 + 64 = 576 bf16 wide: the compressed KV followed by the rotary key.
 * The score uses all 576 columns, the value is the first 512 columns of the same row.
 *
 * SEMANTICS.  All tensors bf16 and dense:
 *   Q [B][H][q_len][576]: per head q_nope W_UK (512 columns) followed by q_rope (64 columns);
 *   the latent cache, contiguous [B][kv_capacity][576], or a pool [n_pages][page_size][576] with an int32 block table
 *   [B][max_pages_per_seq] (page_size % 32 == 0, kv_capacity = max_pages_per_seq x page_size; pages may be shared; the pool may
 *   exceed 4 GiB); an entry in use is clamped to [0, n_pages);
 *   seqlens_k (int32 [B], DEVICE, or NULL = kv_capacity) is read and clamped to [0, kv_capacity] on the device;
 *   S = softmax_scale x Q C^T over 576 columns; O [B][H][q_len][512] = softmax(S) C[:, :512] in bf16; L [B][H][q_len] fp32, the
 *   natural-log LSE.  The q_len queries are the sequence's last q_len tokens, already in the cache; causal is the bottom-right
 *   mask (key j visible to query i iff j <= i + len_b - q_len).  A row without a visible key has O = 0 and L = -inf.
 *   softmax_scale is explicit: the model's scale belongs to its un-absorbed head width, which 576 does not tell.
 * Rows past a length may hold anything, NaNs included, and table entries beyond ceil(len_b / page_size) are never read.  The call
 * is deterministic (no atomics, no waits between workgroups), allocates nothing and does not synchronise; the host reads no
 * length and no table, so one captured graph serves every step.
 *
 * WORK SPLIT.  The M = H x q_len rows of a sequence are one slab [M][576]; a workgroup is (sequence, block of 32 rows, key split).
 * Split s covers keys [s chunk, min((s + 1) chunk, len_b)), chunk = roundup(ceil(len_b / n_splits), 32), on the device.  With
 * n_splits >= 2 every split writes an fp32 partial (O_s [512], L_s) into the workspace and a combine launch folds them in
 * ascending s with ONE rounding to bf16.
 * fa2_mla_decode_num_splits: the default (n_splits = 0), pure host arithmetic on the capacity, never on a length:
 * min(ceil(256 / (B x ceil(M / 32))), max(1, kv_capacity / 256), 256).  Invalid arguments: 1.
 * fa2_mla_decode_workspace_bytes: 0 for one split (and for invalid arguments or a size above SIZE_MAX / 2), else
 * n_splits x B x H x q_len x (512 + 1) x 4 rounded up to 256; n_splits = 0 is the default above.  16-byte aligned.
 *
 * STATUS CODES, in this order, all decided before any HIP call: NULL Q, cache, O, L or block_table -> FA2_ERR_NULL_POINTER;
 * B, H, q_len <= 0, softmax_scale not > 0, kv_capacity (n_pages, page_size, max_pages_per_seq) <= 0,
 * page_size % 32 != 0, a capacity above INT_MAX - 33024 keys (paged) or a contiguous sequence above INT_MAX bytes, n_splits
 * outside 0..256, B x H x q_len above INT_MAX - 32 -> FA2_ERR_INVALID_SHAPE; (kv_lora_rank, rope_dim) other than (512, 64) ->
 * FA2_ERR_UNSUPPORTED_HEAD_DIM; the grid B x ceil(M / 32) x n_splits above INT_MAX or a workspace size that overflows ->
 * FA2_ERR_INVALID_SHAPE; n_splits > 1 with a workspace that is NULL, too small or not 16-byte aligned -> FA2_ERR_WORKSPACE.
 *
 * NOT COVERED: e4m3 latent caches, sinks, sliding windows, ragged / token-major Q (the cache's append: fa2_mla_append_mi355x.h),
 * merging with fa2_merge_states (O is 512 wide), a backward, other latent widths.
 */
#ifndef FA2_MLA_MI355X_H
#define FA2_MLA_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_mla_decode_num_splits(int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim);
size_t fa2_mla_decode_workspace_bytes(int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim, int n_splits);

int fa2_forward_mla_decode(const void* Q, const void* ckv_cache, const int* seqlens_k, void* O, float* L,
                           int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim, float softmax_scale,
                           int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream);

int fa2_forward_mla_decode_paged(const void* Q, const void* ckv_pages, const int* block_table, const int* seqlens_k, void* O,
                                 float* L, int B, int H, int q_len, int n_pages, int page_size, int max_pages_per_seq,
                                 int kv_lora_rank, int rope_dim, float softmax_scale, int causal, int n_splits, void* workspace,
                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_MLA_MI355X_H */
