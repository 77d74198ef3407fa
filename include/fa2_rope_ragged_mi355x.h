/*
 * fa2_rope_ragged_mi355x.h -- C ABI of the RAGGED rotary-embedding KV-cache append (libfa2_mi355x.so,
 * csrc/fa2_rope_append_ragged.hip): the append of fa2_rope_mi355x.h with an n_new PER SEQUENCE and TOKEN-MAJOR tensors -- the
 * half of a continuous-batching step that writes the cache, beside the ragged extend that reads it (fa2_extend_ragged_mi355x.h).
 * ONE launch rotates and appends the K of the step's packed tokens, appends their V, and writes the rotated queries token-major,
 * exactly as fa2_forward_extend_ragged reads them.  A step is: seqlens_k[b] += q_b (the caller's); fa2_extend_ragged_plan, once;
 * then per layer fa2_rope_kv_append_ragged and fa2_forward_extend_ragged(Q_out, plan, ...).  One captured graph serves every
 * step while the mix of prompt chunks, speculative verification and plain decodes changes; the host reads no device value.
 *
 * SEMANTICS.  fa2_rope_kv_append_ragged is fa2_rope_kv_append and fa2_rope_kv_append_ragged_paged is fa2_rope_kv_append_paged,
 * word for word (fa2_rope_mi355x.h, fa2_kvcache_mi355x.h), with these differences.
 * 1. n_new per sequence, from the plan.  The call takes plan, plan_bytes and total_q = T, the plan being the buffer
 *    fa2_extend_ragged_plan filled; it never takes cu_seqlens_q.  Packed token t with start_b <= t < start_b + q_b is token
 *    t - start_b of sequence b's q_b newest; its position is pos = seqlens_k[b] - q_b + (t - start_b), formed by
 *    kv_append_pos(len, q_b, t - start_b, capacity) of csrc/fa2_kv_append_addr.h: the cache row, the table row, and the position
 *    the ragged extend's mask gives that query.  seqlens_k holds the lengths AFTER the append.  q_b = 0 is allowed.
 * 2. Token-major tensors.  Q is bf16 [T][H_q][d] by q_stride_t and q_stride_h (elements); K_new and V_new are bf16 [T][H_kv][d] by
 *    ONE shared pair new_stride_t, new_stride_h.  Strides are non-negative multiples of 8, the last dimension is contiguous,
 *    every pointer is 16-byte aligned: the three slices of a fused [T][(H_q + 2 H_kv) d] projection output go in as they are.
 * 3. A plain ragged append is the same call.  rot_dim = 0 means "no rotation": cos_table and sin_table may then be NULL and
 *    n_positions is ignored.  H_q = 0 with Q = Q_out = NULL means "K/V only".  With both the call is byte for byte fa2_kv_append
 *    (fa2_kv_append_paged) on every sequence.  Otherwise rot_dim is a multiple of 16 in [16, head_dim], as in the siblings.
 * Everything else is the siblings': the four cache kinds (contiguous | paged, bf16 | e4m3); lengths, table and descales read on
 * the device; the e4m3 expression and the uncontracted fp32 rotation (fa2_rope_mi355x.h, ARITHMETIC); both pair forms and
 * partial rot_dim; the write-or-drop rule (written iff 0 <= pos < capacity and, paged, the table entry lies in [0, n_pages);
 * nothing is clamped into range); PAGES WRITTEN BY ONE CALL MUST BELONG TO ONE SEQUENCE EACH; no allocation, no
 * synchronisation, no atomics, deterministic.  A sequence's cache rows and its owned tokens' Q_out rows are bit for bit what
 * fa2_rope_kv_append / _paged writes when called on that sequence alone (B = 1, n_new = q_b).
 *
 * THE PLAN.  plan: the int32 buffer of fa2_extend_ragged_plan, 16-byte aligned, plan_bytes >= (8 + 2 B) x 4.  The kernel reads
 * the header's B, G and T and the B sanitised pairs (start_b, q_b) behind the 8-int header, nothing else: not the work items, not
 * cu_seqlens_q.  THE PLAN IS THE SAFETY CONTRACT, as in the ragged extend.  A header that does not name the call's B and T --
 * and, when H_q > 0, the call's G = H_q / H_kv -- makes every wave leave without a single store, Q_out included (a K/V-only call
 * takes a plan built for any G).  A pair that fails start >= 0, q > 0, q <= T - start owns nothing.  A token's owner is found by
 * csrc/fa2_rope_ragged_owner.h and nothing else: a search of ceil(log2 B) steps, the count from the host.  Whatever the plan
 * buffer holds, every store lands inside the caches, the pool or Q_out; no loop bound comes from device memory.
 *
 * Q_OUT.  bf16 [T][H_q][d] CONTIGUOUS: what fa2_forward_extend_ragged takes with q_token_stride = H_q x d.  EVERY row t < T is
 * written (under a plan that names the call): the rotated row (the source bits for rot_dim = 0) if its token is owned and
 * 0 <= pos < capacity, else +0.0 throughout -- a dropped position, and a token no sequence owns (below plan[4], from plan[5] on).
 * K and V of such tokens are dropped, never clamped.  A bad block-table entry drops K and V only.  Q_out overlapping any input
 * is undefined.
 * WORK SPLIT.  A wave covers a group of consecutive PACKED tokens of one head j (j < H_kv a K/V head, the others Q heads); a
 * lane owns 16 bytes of a row and finds its token's owner itself, so a group may straddle sequences and un-owned tokens.  The
 * grid depends on host values only (capped; the kernel strides).  No LDS.
 *
 * STATUS CODES, the siblings' in the siblings' order, all decided before any HIP call: NULL K_new, V_new, cache, seqlens_k,
 * block_table or plan, a NULL cos_table or sin_table with rot_dim != 0, exactly one of Q and Q_out NULL, or both NULL with
 * H_q != 0 -> FA2_ERR_NULL_POINTER; B, H_kv, total_q, kv_capacity (n_pages, page_size, max_pages_per_seq) or head_dim <= 0,
 * H_q < 0, H_q no multiple of H_kv, page_size % 32 != 0, max_pages_per_seq x page_size above INT_MAX - 33024, a contiguous
 * (b, head) slab of 2 GiB or more, rot_dim neither 0 nor a multiple of 16 in [16, head_dim], rot_dim != 0 with
 * n_positions < capacity, interleaved neither 0 nor 1, (H_q + H_kv) x total_q above INT_MAX, a negative stride or one that is no
 * multiple of 8, a pointer that is not 16-byte aligned -> FA2_ERR_INVALID_SHAPE; head_dim other than 64 or 128 ->
 * FA2_ERR_UNSUPPORTED_HEAD_DIM; dtype not bf16, kv_dtype neither bf16 nor e4m3 -> FA2_ERR_UNSUPPORTED_DTYPE; a non-NULL descale
 * beside a bf16 cache -> FA2_ERR_UNSUPPORTED; plan_bytes below (8 + 2 B) x 4 or a plan that is not 16-byte aligned ->
 * FA2_ERR_WORKSPACE.
 * NOT COVERED: explicit position_ids, tree masks for speculative decoding, token-major pools, per-token scales, a backward,
 * reordering the work items, a norm of the rows (a per-head RMSNorm of Q and K in front of the rotation is
 * fa2_norm_rope_kv_append_ragged, fa2_rope_norm_mi355x.h), and what the siblings leave out.
 */
#ifndef FA2_ROPE_RAGGED_MI355X_H
#define FA2_ROPE_RAGGED_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_rope_kv_append_ragged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                              const float* cos_table, const float* sin_table, const void* plan, size_t plan_bytes,
                              const int* seqlens_k, const float* k_descale, const float* v_descale,
                              int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim,
                              int rot_dim, int n_positions, int interleaved,
                              long long q_stride_t, long long q_stride_h, long long new_stride_t, long long new_stride_h,
                              int dtype, int kv_dtype, void* stream);

int fa2_rope_kv_append_ragged_paged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                                    const int* block_table, const float* cos_table, const float* sin_table,
                                    const void* plan, size_t plan_bytes, const int* seqlens_k,
                                    const float* k_descale, const float* v_descale,
                                    int B, int H_q, int H_kv, int total_q, int n_pages, int page_size,
                                    int max_pages_per_seq, int head_dim,
                                    int rot_dim, int n_positions, int interleaved,
                                    long long q_stride_t, long long q_stride_h, long long new_stride_t, long long new_stride_h,
                                    int dtype, int kv_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_ROPE_RAGGED_MI355X_H */
