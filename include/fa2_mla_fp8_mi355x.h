/*
 * fa2_mla_fp8_mi355x.h -- C ABI of the MLA decode and the MLA latent-cache append over E4M3 LATENT CACHES (libfa2_mi355x.so,
 * csrc/fa2_mla_decode.hip and csrc/fa2_mla_append.hip): fa2_mla_mi355x.h and fa2_mla_append_mi355x.h with an 8-bit latent part.
 * The decode streams the cache once per step and is bound by its bytes; the row drops from 1152 bytes to 640.
 *
 * CACHE ROW.  One token is 640 bytes: bytes [0, 512) are the 512 latent columns as OCP e4m3 codes, bytes [512, 640) the 64 rotary
 * columns in bf16, exactly as in the bf16 row (the rotary key is not normalised and carries the position: it stays in bf16).
 * Contiguous [B][kv_capacity][640] bytes, or a pool [n_pages][page_size][640] behind the int32 block table of fa2_mla_mi355x.h.
 * latent_descale: ONE fp32 per cache, a pointer to one float in DEVICE memory, read on the device when the kernel runs (a captured
 * graph stays valid when the value changes); NULL means 1.0.  The cache holds x / latent_descale -- the family's convention
 * (k_descale / v_descale of fa2_forward_decode_fp8kv, fa2_kvcache_mi355x.h) collapsed to the single MLA "head".
 *
 * DECODE.  fa2_mla_mi355x.h's SEMANTICS on the dequantised row c = (latent_descale x e4m3(row[:512]), bf16(row[512:])):
 * S = softmax_scale x Q c^T over 576 columns, O [B][H][q_len][512] = softmax(S) c[:, :512] in bf16, L fp32.  Q stays bf16 and 576
 * wide.  Lengths, the bottom-right causal mask, keyless rows (O = 0, L = -inf), rows past a length (any bytes, 0xFF -- the e4m3
 * NaN code -- included), the table clamp, the split rule, n_splits, the workspace (fa2_mla_decode_num_splits and
 * fa2_mla_decode_workspace_bytes serve these calls unchanged: the partials are the same), the combine, determinism and graph
 * capture are that header's, word for word.  The codes are widened to bf16 in registers (exact) and both products are the bf16
 * ones; a wave's partial score is latent_descale x s_latent + s_rotary in fp32 (Q is NOT rescaled: that would round it a second
 * time), and latent_descale multiplies the fp32 row of O once, beside 1 / l, before anything is rounded.
 *
 * APPEND.  fa2_mla_append_mi355x.h's contract, word for word, with this row: the RMSNorm result is rounded to bf16 exactly as
 * there and THEN quantised -- clamp(float(y) / latent_descale, +-448) with a correctly rounded division, rounded to nearest even
 * (csrc/fa2_kv_quantise.h, the quantiser of fa2_kv_append) -- so the stored latent bytes are the quantisation of the bf16 append's
 * latent columns and the rotary bytes are its rotary bytes.  Destinations come from csrc/fa2_kv_append_addr.h with a row of 640
 * bytes.  Q_out is unchanged: bf16, 576 wide.
 *
 * STATUS CODES: those of the bf16 calls, in their order, with the 640-byte row in the contiguous limit: a contiguous sequence
 * above INT_MAX bytes is kv_capacity x 640 > INT_MAX.  latent_descale is never read by the host and may be NULL.
 *
 * NOT COVERED: per-token or per-128-column scales, an all-e4m3 576-byte row, fp8 Q or fp8 matrix instructions, and what the two
 * bf16 headers do not cover.
 */
#ifndef FA2_MLA_FP8_MI355X_H
#define FA2_MLA_FP8_MI355X_H

#include "fa2_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int fa2_forward_mla_decode_fp8kv(const void* Q, const void* ckv_cache, const float* latent_descale, const int* seqlens_k, void* O,
                                 float* L, int B, int H, int q_len, int kv_capacity, int kv_lora_rank, int rope_dim,
                                 float softmax_scale, int causal, int n_splits, void* workspace, size_t workspace_bytes,
                                 void* stream);

int fa2_forward_mla_decode_paged_fp8kv(const void* Q, const void* ckv_pages, const int* block_table, const float* latent_descale,
                                       const int* seqlens_k, void* O, float* L, int B, int H, int q_len, int n_pages,
                                       int page_size, int max_pages_per_seq, int kv_lora_rank, int rope_dim, float softmax_scale,
                                       int causal, int n_splits, void* workspace, size_t workspace_bytes, void* stream);

int fa2_mla_kv_append_fp8kv(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_cache,
                            const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                            const float* latent_descale, const int* seqlens_k,
                            int B, int H, int n_new, int kv_capacity, int kv_lora_rank, int rope_dim,
                            int n_positions, int interleaved,
                            long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                            long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                            long long kv_stride_b, long long kv_stride_t, void* stream);

int fa2_mla_kv_append_paged_fp8kv(const void* q_nope, const void* q_pe, void* Q_out, const void* kv_new, void* ckv_pages,
                                  const int* block_table,
                                  const float* cos_table, const float* sin_table, const float* kv_weight, float eps,
                                  const float* latent_descale, const int* seqlens_k,
                                  int B, int H, int n_new, int n_pages, int page_size, int max_pages_per_seq,
                                  int kv_lora_rank, int rope_dim,
                                  int n_positions, int interleaved,
                                  long long q_nope_stride_b, long long q_nope_stride_h, long long q_nope_stride_t,
                                  long long q_pe_stride_b, long long q_pe_stride_h, long long q_pe_stride_t,
                                  long long kv_stride_b, long long kv_stride_t, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FA2_MLA_FP8_MI355X_H */
