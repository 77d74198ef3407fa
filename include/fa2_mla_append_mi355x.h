/*
 * fa2_mla_append_mi355x.h -- C ABI of the MLA LATENT-CACHE APPEND (libfa2_mi355x.so, csrc/fa2_mla_append.hip): the producer of
 * the 576-wide latent cache that fa2_forward_mla_decode / _paged read (fa2_mla_mi355x.h), and of the Q they take.  ONE launch
 * normalises the n_new newest tokens' compressed KV (the models' kv_a_layernorm: an RMSNorm over the 512 latent columns only),
 * rotates their 64-wide rotary key, writes both into ONE cache row per token, and assembles the step's queries
 * Q_out [B][H][n_new][576] from the absorbed q_nope (512 columns, copied) and q_pe (64 columns, rotated).  A decode step is
 * seqlens_k += n_new; fa2_mla_kv_append; fa2_forward_mla_decode(Q_out, ...) in one captured graph, the closure
 * fa2_rope_kv_append gave the plain decode.  Status codes are those of fa2_mi355x.h.
 *
 * SEMANTICS.  The uniform fa2_rope_kv_append contract (fa2_rope_mi355x.h), word for word wherever it applies:
 *   seqlens_k: int32 [B] in DEVICE memory, REQUIRED, the lengths AFTER the append.  Token t of sequence b has position
 *   pos = seqlens_k[b] - n_new + t, formed in 64 bits through kv_append_pos: its cache row, the position the decode's mask gives
 *   query t, and the row of the cos/sin tables.  The cache row is WRITTEN iff 0 <= pos < capacity and, paged, the table entry
 *   lies in [0, n_pages); nothing is clamped into range, and only the table entries of written rows are read.  Destinations come
 *   from csrc/fa2_kv_append_addr.h alone: the latent cache [B][kv_capacity][576] is that file's [B][H_kv = 1][capacity][d = 576],
 *   the pool [n_pages][page_size][576] its paged form with H_kv = 1 (capacity = max_pages_per_seq x page_size).  The host checks
 *   n_positions >= capacity, so no table read depends on an unchecked device value.  Lengths, block table, tables and weight are
 *   read on the device when the kernel runs, never by the host; nothing is allocated, nothing synchronises, no atomics and no
 *   communication between workgroups: the call is deterministic and capturable.  PAGES WRITTEN BY ONE CALL MUST BELONG TO ONE
 *   SEQUENCE EACH.
 * SOURCES.  All bf16, last dimension contiguous, 16-byte aligned, element strides non-negative multiples of 8:
 *   kv_new  [B][n_new][576] by (kv_stride_b, kv_stride_t): c_kv (512) then k_pe (64), the slice of a fused kv_a_proj_with_mqa /
 *           qkv_a_proj output passed as it is;
 *   q_nope  [B][H][n_new][512] by its three strides: the absorbed q_nope W_UK, typically the bmm output viewed from
 *           [H][B x n_new][512];
 *   q_pe    [B][H][n_new][64] by its OWN three strides: the slice at column 128 of [...][H][192].
 * CACHE ROW.  row[:512] = RMSNorm(c_kv; kv_weight, eps), row[512:] = rotate(k_pe, pos).
 *   kv_weight: fp32 [512] in DEVICE memory, 16-byte aligned; the caller converts a checkpoint's bf16 weight once
 *   (fa2_rope_norm_mi355x.h).  The norm is fa2_rope_norm_mi355x.h ARITHMETIC steps 1-5 at d = 512: eight elements a lane and 64
 *   lanes a row, the butterfly m = 1, 2, 4, 8, 16, 32, 1 / 512 a power of two, sqrt and the division correctly rounded, nothing
 *   contracted, ONE rounding to bf16, after the weight.  The rotation is csrc/fa2_rope_rotate.h's (fa2_rope_mi355x.h, ARITHMETIC)
 *   on the 64 columns, rot_dim = rope_dim = 64: cos_table, sin_table fp32 [n_positions][32] contiguous in DEVICE memory, 16-byte
 *   aligned; interleaved == 0 the rotate-half pairs (i, i + 32), == 1 the pairs (2i, 2i + 1).
 * Q_OUT.  bf16 [B][H][n_new][576] CONTIGUOUS, what the decode takes.  EVERY row is written: Q_out[..., :512] the bytes of q_nope,
 *   Q_out[..., 512:] = rotate(q_pe, pos); a row whose position is dropped (pos outside [0, capacity)) is +0.0 in all 576 columns.
 *   A bad table entry drops the cache row only: Q depends on pos alone.  H = 0 with q_nope, q_pe and Q_out all NULL is a
 *   cache-only call (filling the cache after a prefill).  Q_out overlapping an input is undefined.
 * WORK SPLIT.  One wave per unit, four waves per workgroup, no LDS; a token (b, t) is one cache unit and ceil(H / 8) query units
 *   of eight heads.  The grid depends on host values only (capped; the kernel strides over units).
 *
 * STATUS CODES, in this order, all decided before any HIP call: NULL kv_new, cache, cos_table, sin_table, kv_weight, seqlens_k or
 * block_table, some but not all of q_nope, q_pe, Q_out NULL, or all three NULL with H != 0 -> FA2_ERR_NULL_POINTER; B, n_new,
 * kv_capacity (n_pages, page_size, max_pages_per_seq) <= 0, H < 0, page_size % 32 != 0, a capacity above INT_MAX - 33024 keys
 * (paged) or a contiguous sequence above INT_MAX bytes (fa2_forward_mla_decode's limits: a cache this call accepts that call
 * accepts), B x (H + 1) x n_new above INT_MAX, eps not finite or not > 0, interleaved neither 0 nor 1, n_positions < capacity, a
 * negative stride or one that is no multiple of 8, a pointer that is not 16-byte aligned -> FA2_ERR_INVALID_SHAPE;
 * (kv_lora_rank, rope_dim) other than (512, 64) -> FA2_ERR_UNSUPPORTED_HEAD_DIM.
 *
 * NOT COVERED: e4m3 latent caches, ragged n_new / token-major Q (the MLA decode takes a uniform q_len), bf16 weights, a norm of
 * q, explicit position_ids, cos/sin computed in the kernel, other latent widths.
 */
#ifndef FA2_MLA_APPEND_MI355X_H
#define FA2_MLA_APPEND_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_mla_kv_append(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_cache,
                      const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                      const int* seqlens_k,
                      int B, int H, int n_new, int kv_capacity, int kv_lora_rank, int rope_dim,
                      int n_positions, int interleaved,
                      long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                      long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                      long long kv_stride_b, long long kv_stride_t, void* stream);

int fa2_mla_kv_append_paged(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_pages,
                            const int* block_table,
                            const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                            const int* seqlens_k,
                            int B, int H, int n_new, int n_pages, int page_size, int max_pages_per_seq,
                            int kv_lora_rank, int rope_dim,
                            int n_positions, int interleaved,
                            long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                            long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                            long long kv_stride_b, long long kv_stride_t, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_MLA_APPEND_MI355X_H */
