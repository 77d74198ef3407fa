/*
 * fa2_kvcache_mi355x.h -- C ABI of the KV-cache append (libfa2_mi355x.so, csrc/fa2_kv_append.hip): the call that WRITES the
 * caches fa2_forward_decode, fa2_forward_decode_paged and their _fp8kv forms (fa2_mi355x.h) read, under the same contract:
 * lengths, block table and descales are read on the device when the kernel runs and never by the host, nothing is allocated,
 * nothing synchronises, ONE plain launch covers K and V, no atomics and no communication between workgroups, so the call is
 * deterministic and one captured graph of {append, decode} serves every decode step.  Status codes are those of fa2_mi355x.h.
 *
 * THE OPERATION.  Append the n_new newest tokens' K and V of every sequence to its cache: n_new is 1 at a decode step, a few
 * under speculative decoding, thousands for a prompt chunk.
 * POSITION.  seqlens_k: int32 [B] in DEVICE memory, REQUIRED, the lengths AFTER the append -- the same tensor with the same
 * meaning the decode call of the same step reads (its q_len queries are the sequence's last q_len tokens, already in the
 * cache).  A step is: bump the lengths in place, append, decode.  Token t of sequence b goes to logical row
 * pos = seqlens_k[b] - n_new + t, formed in 64 bits (any int32 length, INT_MIN and INT_MAX included).  It is written if and only
 * if 0 <= pos < kv_capacity; every other token is DROPPED -- this is a write, nothing is clamped into range --, and a dropped
 * token does not stop the other tokens of the call.  No loop bound comes from a stored value, and the only address that does
 * is a row that passed that test.
 * SOURCE.  K_new, V_new: bf16, logical shape [B][H_kv][n_new][d], d 64 or 128, given by three ELEMENT strides (batch, head,
 * token) shared by both tensors, the last dimension contiguous: a token-major [B][n_new][H_kv][d] tensor or the K and V slices
 * of a fused QKV projection output are passed as they are.  Strides are non-negative multiples of 8 and all four tensor
 * pointers are 16-byte aligned: a lane loads 16 bytes.  A source that overlaps the cache is undefined.
 * DESTINATION.  The decode calls' layouts: K_cache, V_cache [B][H_kv][kv_capacity][d], or (paged) K_pages, V_pages
 * [n_pages][H_kv][page_size][d]; kv_dtype FA2_DTYPE_BF16 or FA2_DTYPE_FP8_E4M3 (OCP e4m3, one byte per element).  dtype is the
 * source's (FA2_DTYPE_BF16).
 * VALUES.  Into a bf16 cache the source bits are copied.  Into an e4m3 cache head h stores clamp(float(x) / descale[h], -448, 448)
 * rounded to nearest even, the division a correctly rounded fp32 division: byte for byte
 * (x.float() / descale).clamp(-448, 448).to(torch.float8_e4m3fn).  +-inf becomes +-448 (the cast alone would not saturate), NaN
 * becomes a NaN code (0x7F or 0xFF), -0.0 keeps its sign.  k_descale, v_descale: fp32 [H_kv] in DEVICE memory, or NULL (= 1);
 * positive and finite by contract; read when the kernel runs -- the decode's descales.  A non-NULL descale beside a bf16 cache is
 * refused.
 * PAGED.  block_table: int32 [B][max_pages_per_seq] in DEVICE memory.  Row pos is row pos % page_size of page
 * block_table[b][pos / page_size]; kv_capacity = max_pages_per_seq x page_size with the decode's limit; page_size % 32 == 0 as in
 * the decode.  A token whose table entry lies outside [0, n_pages) is DROPPED (the decode clamps such an entry; a write through
 * a clamped entry would corrupt another sequence's page); its neighbours on other pages are written.  Only the entries of rows
 * that are written are read, all inside [0, B x max_pages_per_seq).  The pool may exceed 4 GiB (64-bit addresses).
 * PAGES WRITTEN BY ONE CALL MUST BELONG TO ONE SEQUENCE EACH: two sequences appending to one page is a race.  Shared prefix
 * pages are read-only to an append; allocating pages and copy-on-write stay the allocator's.
 * WORK SPLIT.  A lane moves 16 source bytes of K and of V and stores 16 (bf16) or 8 (e4m3) bytes of each; a wave covers whole
 * rows of one (sequence, K/V head), so the length and the descales are scalar loads per wave and the table entry is one load
 * per row.  The grid depends on host values only (capped; the kernel strides over the rest).  No LDS.
 * STATUS CODES, in this order, all decided before any HIP call: NULL K_new, V_new, cache, seqlens_k or block_table ->
 * FA2_ERR_NULL_POINTER; B, H_kv, n_new, kv_capacity (n_pages, page_size, max_pages_per_seq) or head_dim <= 0, page_size % 32 != 0,
 * max_pages_per_seq x page_size above INT_MAX - 33024, a contiguous (b, head) slab of 2 GiB or more (kv_capacity x head_dim x 2
 * bytes, x 1 for e4m3), B x H_kv x n_new above INT_MAX, a negative stride or one that is no multiple of 8, a pointer that is not
 * 16-byte aligned -> FA2_ERR_INVALID_SHAPE; head_dim other than 64 or 128 -> FA2_ERR_UNSUPPORTED_HEAD_DIM; dtype not bf16,
 * kv_dtype neither bf16 nor e4m3 -> FA2_ERR_UNSUPPORTED_DTYPE; a non-NULL descale beside a bf16 cache -> FA2_ERR_UNSUPPORTED.
 * NOT COVERED: in THESE calls ragged n_new per sequence and packed [T][H][d] sources with cu_seqlens (that is
 * fa2_rope_kv_append_ragged with rot_dim = 0 and H_q = 0, fa2_rope_ragged_mi355x.h), token-major pools (rotary embedding fused
 * into the append is fa2_rope_kv_append, fa2_rope_mi355x.h), per-token or per-page scales, e5m2, a dequantising gather from pages into contiguous keys, page allocation
 * and copy-on-write.
 */
#ifndef FA2_KVCACHE_MI355X_H
#define FA2_KVCACHE_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_kv_append(const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                  const int* seqlens_k, const float* k_descale, const float* v_descale,
                  int B, int H_kv, int n_new, int kv_capacity, int head_dim,
                  long long new_stride_b, long long new_stride_h, long long new_stride_t,
                  int dtype, int kv_dtype, void* stream);

int fa2_kv_append_paged(const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                        const int* block_table, const int* seqlens_k,
                        const float* k_descale, const float* v_descale,
                        int B, int H_kv, int n_new, int n_pages, int page_size,
                        int max_pages_per_seq, int head_dim,
                        long long new_stride_b, long long new_stride_h, long long new_stride_t,
                        int dtype, int kv_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_KVCACHE_MI355X_H */
