// fa2_mla_decode_tile.inc -- one 32-key tile of the workgroup in mla_split_body (fa2_mla_decode.hip), textually included where
// the tile loop stands: the tile's first key is MLA_KB, the wave's column slice of its 32 rows waits in kf[MLA_SL], and the
// partial scores go through exchange buffer MLA_XB.  Behind the first product the slot takes the loads of the tile PF ahead.
// Included text and not a lambda, like fa2_decode_tile.inc.  EB = 1 (e4m3 latent columns): the slot holds raw codes and the tile's
// first product is fa2_mla_decode_fp8_tile.inc; from the exchange on the text is shared.
// MLA_VISIBLE(e): whether key acc_row(e, h) of the tile is visible to the lane's row.  The including body defines it: a key
// position below kmax (mla_split_body), a bit of the tile's live mask (mla_sparse_body, whose load_tile gathers the rows).
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.0f;
        if constexpr (EB == 2) {
        // the latent part of the slice is this wave's 128 columns of V: lane (key r, half h) holds chunk 2 t + h of row r
#pragma unroll
        for (int t = 0; t < 8; ++t) *reinterpret_cast<u32x4*>(vimg + lds_off<128>(r, 2 * t + h)) = kf[MLA_SL][t];
#pragma unroll
        for (int t = 0; t < kMlaKS; ++t) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[MLA_SL][t]), q[t], s, 0, 0, 0);
        } else {
#include "fa2_mla_decode_fp8_tile.inc"
        }
        load_tile(MLA_KB + PF * kMlaTile, MLA_SL);
        if constexpr (PAGED) fetch_entry(MLA_KB + (PF + 1) * kMlaTile);      // the table entry of the tile after the loaded one

        // The four partial S^T (this wave's 144 of the 576 columns each) meet: [wave][g4][lane] f32x4, the same lane of every
        // wave holding the same (key, row) elements.  One barrier per tile: the buffer written two tiles later is free because
        // every wave passed the barrier in between behind its reads of this one.
        {
            float* const xb = reinterpret_cast<float*>(smem + kMlaWaves * kMlaVimg + MLA_XB * kMlaXbuf);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<f32x4*>(xb + ((wave * 4 + g4) * 64 + lane) * 4) = f32x4{s[4 * g4], s[4 * g4 + 1], s[4 * g4 + 2], s[4 * g4 + 3]};
            __syncthreads();
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {      // wave order 0..3 in every wave: the same bits of S everywhere
                f32x4 v = *reinterpret_cast<const f32x4*>(xb + (g4 * 64 + lane) * 4);
#pragma unroll
                for (int w = 1; w < kMlaWaves; ++w) v += *reinterpret_cast<const f32x4*>(xb + ((w * 4 + g4) * 64 + lane) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[4 * g4 + e] = v[e];
            }
        }

        // fa2_decode_tile.inc's softmax: the row is the lane, its 16 keys the registers, masked P selected to 0
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] *= sc;
            mx = MLA_VISIBLE(e) ? fmaxf(mx, s[e]) : mx;
        }
        mx = half_max(mx);
        const float m_new = fmaxf(m, mx);
        const float m0 = m_new == -INFINITY ? 0.0f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m - m0);      // m = -inf: 0, and there is nothing to scale yet
        m = m_new;
        float ps = 0.0f;
        bf16x8 p[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float pe = MLA_VISIBLE(e) ? __builtin_amdgcn_exp2f(s[e] - m0) : 0.0f;
            ps += pe;
            p[e >> 3][e & 7] = (__bf16)pe;
        }
        l = l * alpha + ps;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[c][e] *= alpha;
        // O^T [128 w ..+128][32 rows] += V^T P^T.  Element j of half h of k-step ks is key 16 ks + 8 (j >> 2) + 4 h + (j & 3):
        // two transposed reads of four keys each
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 vt;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int row = 16 * ks + 8 * u + 4 * h + qq, col = 32 * c + c0 + 4 * pp;
                    const bf16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                        (mla_lds_bf16x4*)(vimg + lds_off<128>(row, col >> 3) + 8 * (pp & 1)));
#pragma unroll
                    for (int e = 0; e < 4; ++e) vt[4 * u + e] = x[e];
                }
                o[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, p[ks], o[c], 0, 0, 0);
            }
        }
#undef MLA_KB
#undef MLA_SL
#undef MLA_XB
