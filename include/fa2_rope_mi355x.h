/*
 * fa2_rope_mi355x.h -- C ABI of the rotary-embedding KV-cache append (libfa2_mi355x.so, csrc/fa2_rope_append.hip): ONE launch
 * that rotates the n_new newest tokens' K and writes it into the cache, copies their V into the cache, and writes the step's
 * rotated queries in the layout the decode calls take.  It is fa2_kv_append / fa2_kv_append_paged (fa2_kvcache_mi355x.h) with
 * rotary position embedding (RoPE) in front, under the same contract: lengths, block table, descales and the cos/sin tables are
 * read on the device when the kernel runs and never by the host, nothing is allocated, nothing synchronises, no atomics and no
 * communication between workgroups, so the call is deterministic and one captured graph of {this call, decode} serves every
 * decode step: seqlens_k += n_new; fa2_rope_kv_append; fa2_forward_decode(Q_out, ...).  Status codes are those of fa2_mi355x.h.
 *
 * POSITION.  seqlens_k: int32 [B] in DEVICE memory, REQUIRED, the lengths AFTER the append.  Token t of sequence b has position
 * pos = seqlens_k[b] - n_new + t, formed in 64 bits (any int32 length): the append's logical row, the position the decode's mask
 * gives query t, and the row of the cos/sin tables its rotation uses.  The host checks n_positions >= capacity (kv_capacity, or
 * max_pages_per_seq x page_size), so a row inside the cache is always inside the tables and no table read depends on an
 * unchecked device value.
 * TABLES.  cos_table, sin_table: fp32 [n_positions][rot_dim / 2], contiguous, in DEVICE memory, 16-byte aligned.  The caller
 * builds them, so any frequency scaling scheme (linear, NTK, YaRN, Llama-3) is the caller's.  rot_dim is a multiple of 16 with
 * 16 <= rot_dim <= head_dim; elements rot_dim .. d-1 of a row pass through unrotated (partial rotary).
 * PAIRS.  interleaved == 0: the rotate-half (NeoX, HF) form, pairs (i, i + rot_dim/2).  interleaved == 1: the GPT-J form, pairs
 * (2i, 2i + 1).  Both use table column i, i < rot_dim/2.
 * ARITHMETIC.  For a pair (x1, x2) of bf16 values widened to fp32 (exact), c = cos[pos][i], s = sin[pos][i]:
 *     y1 = bf16_rne(fl(fl(x1*c) - fl(x2*s)))        y2 = bf16_rne(fl(fl(x2*c) + fl(x1*s)))
 * every fl ONE IEEE fp32 rounding: the products are NOT contracted into a fused multiply-add.  Byte for byte
 * (x1.float()*c - x2.float()*s).bfloat16() and (x2.float()*c + x1.float()*s).bfloat16() in torch.  HF's all-bf16 arithmetic
 * (tables cast to bf16, each product rounded to bf16, then the sum) is a DIFFERENT and less exact expression and is not
 * reproduced.  For a NaN result only NaN-ness is specified.
 * K.  Rotated, then stored exactly as fa2_kv_append stores it: into a bf16 cache the rotated bf16 bits; into an e4m3 cache
 * clamp(float(y) / descale[h], -448, 448) rounded to nearest even, y the rotated value AFTER its rounding to bf16.  The call is
 * byte for byte {rotate in torch to bf16, then fa2_kv_append}.  The write-or-drop rule (written iff 0 <= pos < capacity and, paged,
 * the table entry lies in [0, n_pages); nothing is clamped into range), the table-entry rule (only entries of written rows are
 * read), the limits, the alignment and PAGES WRITTEN BY ONE CALL MUST BELONG TO ONE SEQUENCE EACH are fa2_kv_append's and
 * fa2_kv_append_paged's, word for word; destinations are formed by csrc/fa2_kv_append_addr.h and nothing else.
 * V.  Never rotated: handled exactly as the append handles it.
 * SOURCES.  K_new, V_new: bf16 [B][H_kv][n_new][d] by the three element strides new_stride_*, as in fa2_kv_append.  Q: bf16
 * [B][H_q][n_new][d] by its OWN three element strides q_stride_* (batch, head, token), last dimension contiguous: the Q slice of
 * a fused QKV output, or a separate [B][n_new][H_q][d] tensor, is passed as it is.  Strides are non-negative multiples of 8, every
 * pointer is 16-byte aligned.
 * Q_OUT.  bf16 [B][H_q][n_new][d] CONTIGUOUS, what the decode takes.  EVERY row t < n_new is written: the rotated row if
 * 0 <= pos < capacity, else +0.0 throughout (no table row exists for such a position, and an unwritten row would make a replay
 * depend on old memory).  A bad block-table entry drops the token's K and V only: Q depends on pos alone.  Q and Q_out may both
 * be NULL with H_q = 0 (a K/V-only call).  Q_out overlapping any input is undefined.
 * WORK SPLIT.  The append's, extended over heads: a wave covers whole rows of one (sequence, head j), j < H_kv a K/V head,
 * the others Q heads; a lane owns 16 bytes of a row.  The grid depends on host values only (capped; the kernel strides).  No LDS.
 * STATUS CODES, in this order, all decided before any HIP call: NULL K_new, V_new, cache, cos_table, sin_table, seqlens_k or
 * block_table, exactly one of Q and Q_out NULL, or both NULL with H_q != 0 -> FA2_ERR_NULL_POINTER; B, H_kv, n_new, kv_capacity
 * (n_pages, page_size, max_pages_per_seq) or head_dim <= 0, H_q < 0, page_size % 32 != 0, max_pages_per_seq x page_size above
 * INT_MAX - 33024, a contiguous (b, head) slab of 2 GiB or more, rot_dim no multiple of 16 or outside [16, head_dim],
 * n_positions < capacity, interleaved neither 0 nor 1, B x (H_q + H_kv) x n_new above INT_MAX, a negative stride or one that is no
 * multiple of 8, a pointer that is not 16-byte aligned -> FA2_ERR_INVALID_SHAPE; head_dim other than 64 or 128 ->
 * FA2_ERR_UNSUPPORTED_HEAD_DIM; dtype not bf16, kv_dtype neither bf16 nor e4m3 -> FA2_ERR_UNSUPPORTED_DTYPE; a non-NULL descale
 * beside a bf16 cache -> FA2_ERR_UNSUPPORTED.
 * NOT COVERED: a position other than the cache row (explicit position_ids, multimodal 3-D RoPE), cos/sin computed in the kernel
 * from a base frequency, HF's bf16 arithmetic, a backward, RoPE for the training forward, ragged n_new (an n_new per sequence and
 * token-major tensors are fa2_rope_kv_append_ragged, fa2_rope_ragged_mi355x.h), head_dim other than 64 or 128.
 */
#ifndef FA2_ROPE_MI355X_H
#define FA2_ROPE_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_rope_kv_append(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                       const float* cos_table, const float* sin_table, const int* seqlens_k,
                       const float* k_descale, const float* v_descale,
                       int B, int H_q, int H_kv, int n_new, int kv_capacity, int head_dim,
                       int rot_dim, int n_positions, int interleaved,
                       long long q_stride_b, long long q_stride_h, long long q_stride_t,
                       long long new_stride_b, long long new_stride_h, long long new_stride_t,
                       int dtype, int kv_dtype, void* stream);

int fa2_rope_kv_append_paged(const void* Q, void* Q_out, const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                             const int* block_table, const float* cos_table, const float* sin_table, const int* seqlens_k,
                             const float* k_descale, const float* v_descale,
                             int B, int H_q, int H_kv, int n_new, int n_pages, int page_size,
                             int max_pages_per_seq, int head_dim,
                             int rot_dim, int n_positions, int interleaved,
                             long long q_stride_b, long long q_stride_h, long long q_stride_t,
                             long long new_stride_b, long long new_stride_h, long long new_stride_t,
                             int dtype, int kv_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_ROPE_MI355X_H */
