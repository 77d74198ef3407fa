// fa2_mla_decode_fp8_tile.inc -- the e4m3 data path of one 32-key tile (EB = 1), included by fa2_mla_decode_tile.inc in the place
// of the bf16 body's V-image writes and nine MFMAs: kf[MLA_SL][0..3] are the lane's four 16-byte loads of latent CODES, kf[MLA_SL][4]
// its rotary bf16; `s` arrives zeroed and leaves as the wave's partial S^T, descale x s_latent + s_rotary.
            // Load j, words 2 u ..+2: the eight codes of k-step 2 j + u, columns 128 w + 32 j + 16 h + 8 u ..+8 -- q[2 j + u]'s.
            // Widened once (exact: three mantissa bits, every e4m3 exponent a normal bf16 one), used by both products.
            bf16x8 kw[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) kw[t] = mla_e4m3x8_to_bf16(kf[MLA_SL][t / 2][2 * (t % 2)], kf[MLA_SL][t / 2][2 * (t % 2) + 1]);
            // this wave's 128 columns of V, in bf16 like the bf16 body's: k-step 2 j + u of half h is chunk 4 j + 2 h + u of row r.
            // A 16-lane group of one write has 16 consecutive rows and one chunk: 16 slots, no bank conflict (fa2_mla_decode.hip).
#pragma unroll
            for (int t = 0; t < 8; ++t) *reinterpret_cast<bf16x8*>(vimg + lds_off<128>(r, 4 * (t / 2) + 2 * h + t % 2)) = kw[t];
#pragma unroll
            for (int t = 0; t < 8; ++t) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kw[t], q[t], s, 0, 0, 0);
            // the rotary columns hold their own values: an accumulator of their own, joined behind the descale
            f32x16 sr;
#pragma unroll
            for (int e = 0; e < 16; ++e) sr[e] = 0.0f;
            sr = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[MLA_SL][4]), q[8], sr, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = fmaf(ds, s[e], sr[e]);
