/*
 * fa2_rope_norm_mi355x.h -- C ABI of the ragged rotary-embedding KV-cache append WITH A PER-HEAD QK RMSNorm IN FRONT OF THE ROTATION
 * (libfa2_mi355x.so, csrc/fa2_norm_rope_append_ragged.hip): the append of fa2_rope_ragged_mi355x.h for models that normalise
 * every query row and key row over head_dim, with a learned weight [head_dim] for Q and another for K, before they rotate it
 * (Qwen3, Gemma 3 and others).  ONE launch normalises, rotates and appends the K of the step's packed tokens, appends their V
 * untouched, and writes the normalised, rotated queries token-major, exactly as fa2_forward_extend_ragged reads them: the three
 * slices of the fused QKV projection output still go in as they are, with no framework norm and no normalised copy of Q and K
 * in between.  A step is unchanged: seqlens_k[b] += q_b; fa2_extend_ragged_plan, once; then per layer
 * fa2_norm_rope_kv_append_ragged and fa2_forward_extend_ragged(Q_out, plan, ...), all in one captured graph.
 *
 * SEMANTICS.  fa2_norm_rope_kv_append_ragged is fa2_rope_kv_append_ragged and fa2_norm_rope_kv_append_ragged_paged is
 * fa2_rope_kv_append_ragged_paged, argument for argument and word for word (fa2_rope_ragged_mi355x.h), with three additions
 * behind sin_table:
 *   q_weight  fp32 [head_dim] in DEVICE memory, contiguous, 16-byte aligned, read on the device.  NULL only when H_q == 0.
 *   k_weight  fp32 [head_dim], the same rules.  Never NULL.
 *   eps       a host value, finite and > 0.
 * THE CALLER BUILDS THE WEIGHTS, as it builds cos and sin: Gemma's (1 + w), and a checkpoint's bf16 weight, are folded or
 * converted to fp32 once by the caller.  Every live Q row (a row with 0 <= pos < capacity whose token is owned) and every K row
 * that is written is first replaced by its RMSNorm n (ARITHMETIC), a bf16 row; everything after that is the sibling's, on n:
 * THE CALL IS BIT FOR BIT fa2_rope_kv_append_ragged (_paged) APPLIED TO THE NORMALISED bf16 TENSORS.  With rot_dim = 0 it
 * stores n itself (K through the cache's store, Q into Q_out); elements past a partial rot_dim are n's.  V is copied untouched.
 * The sibling's contract holds unchanged: the plan is the safety contract (a header that does not name the call's B, T and,
 * with Q heads, G ends every wave before its first store); ownership comes from csrc/fa2_rope_ragged_owner.h alone and cache
 * addresses from csrc/fa2_kv_append_addr.h alone (kv_append_pos); the write-or-drop rule (written iff 0 <= pos < capacity and,
 * paged, the table entry lies in [0, n_pages); nothing is clamped); EVERY Q_out row t < T is written, +0.0 throughout for a
 * dropped position and for a token no sequence owns; the four cache kinds (contiguous | paged, bf16 | e4m3) and the e4m3
 * expression clamp(float(y) / descale[h], -448, 448) on the rotated bf16 y; both pair forms and partial rot_dim; PAGES WRITTEN BY
 * ONE CALL MUST BELONG TO ONE SEQUENCE EACH; no allocation, no synchronisation, no atomics, deterministic, capturable.
 *
 * ARITHMETIC.  All IEEE fp32, every fl ONE rounding, no contraction into a fused multiply-add anywhere.  For a row of d bf16
 * elements x_i widened (exactly) to fp32, the lane that owns elements 8c .. 8c+7 and the row's d / 8 lanes:
 *   1. q_i = fl(x_i * x_i).
 *   2. per lane, left to right: s = ((((((q0 + q1) + q2) + q3) + q4) + q5) + q6) + q7.
 *   3. a butterfly over the row's lanes: for m = 1, 2, 4 (and 8 at d = 128), s = fl(s + s[lane ^ m]).  fp32 addition commutes,
 *      so every lane of the row ends with the same bits.  The order is part of the contract: another order changes r's last bit
 *      on a large share of rows.
 *   4. r = fl(1 / fl(sqrt(fl(fl(s * (1 / d)) + eps)))); 1 / d is a power of two; sqrt and the division are correctly rounded, never
 *      a native or approximate reciprocal square root.
 *   5. n_i = bf16_rne(fl(fl(x_i * r) * w_i)): ONE rounding to bf16, after the weight.  This is Gemma 3's form.  HF Qwen3's
 *      extra rounding of x * r to bf16 BEFORE the weight is a different, less exact expression and is not reproduced -- as HF's
 *      all-bf16 rotation is not (fa2_rope_mi355x.h, ARITHMETIC).
 *   6. the rotation of csrc/fa2_rope_rotate.h (fa2_rope_mi355x.h, ARITHMETIC), unchanged, on the bf16 row n.
 * An all-zero row has s = 0, r = 1 / sqrt(eps) and n_i = +-0 by the signs of x_i and w_i.  For a NaN result only NaN-ness is
 * specified.  A rotate-half lane normalises its partner's raw chunk with the same r and the partner's eight weights: the bits the
 * partner lane computes for itself.  Rows that are not live contribute nothing; the butterfly runs on every lane.
 *
 * STATUS CODES, the sibling's in the sibling's order, all decided before any HIP call, with: a NULL k_weight, or a NULL q_weight
 * with H_q > 0 -> FA2_ERR_NULL_POINTER (with the other NULL pointers); eps zero, negative, infinite or NaN, or a weight that is
 * not 16-byte aligned -> FA2_ERR_INVALID_SHAPE (with the other shapes and alignments); then FA2_ERR_UNSUPPORTED_HEAD_DIM,
 * FA2_ERR_UNSUPPORTED_DTYPE, FA2_ERR_UNSUPPORTED and, last, FA2_ERR_WORKSPACE as in fa2_rope_ragged_mi355x.h.
 * NOT COVERED: the uniform [B][H][n_new][d] call (a uniform batch is a ragged batch; fa2_rope_kv_append stays without a norm),
 * bf16 weights, a norm of V, a norm over anything but the whole head_dim, LayerNorm (a mean or a bias), HF Qwen3's intermediate
 * bf16 rounding, a backward, and what the sibling leaves out (explicit position_ids, tree masks, token-major pools, per-token
 * scales).
 */
#ifndef FA2_ROPE_NORM_MI355X_H
#define FA2_ROPE_NORM_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_norm_rope_kv_append_ragged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                                   const float* cos_table, const float* sin_table, const float* q_weight, const float* k_weight,
                                   float eps, const void* plan, size_t plan_bytes,
                                   const int* seqlens_k, const float* k_descale, const float* v_descale,
                                   int B, int H_q, int H_kv, int total_q, int kv_capacity, int head_dim,
                                   int rot_dim, int n_positions, int interleaved,
                                   long long q_stride_t, long long q_stride_h, long long new_stride_t, long long new_stride_h,
                                   int dtype, int kv_dtype, void* stream);

int fa2_norm_rope_kv_append_ragged_paged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                                         const int* block_table, const float* cos_table, const float* sin_table,
                                         const float* q_weight, const float* k_weight, float eps,
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
#endif /* FA2_ROPE_NORM_MI355X_H */
