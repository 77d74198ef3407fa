// fa2_extend_tile.inc -- one 32-key tile of a wave in extend_split_body (fa2_decode.hip): fa2_decode_tile.inc with RT row tiles,
// every K fragment and V fragment feeding the products of each.  Textually included where the loop
// over a wave's tiles stands: the tile's first key is DEC_KB and its K / V fragments wait in slot DEC_SL (kf[DEC_SL], vf[DEC_SL]),
// which -- behind the first product -- takes the loads of the tile PF rounds ahead.  Included text and not a lambda: called through
// a lambda, the bf16 kernels' loop came out of the compiler re-scheduled (tools/asm_identity.py against the parent).
        if constexpr (WIN) {      // the tile that straddles lo: its V rows below lo may hold anything, and 0 x NaN is NaN
            if (DEC_KB < lo) {
#pragma unroll
                for (int n = 0; n < NV; ++n)
                    if (DEC_KB + n * RPI + lane / CPR < lo) vf[DEC_SL][n] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            if constexpr (EB == 2) {
                *reinterpret_cast<u32x4*>(vimg + lds_off<D>(n * RPI + lane / CPR, lane % CPR)) = vf[DEC_SL][n];
            } else {      // the lane's 16 elements are two 16-byte chunks of the bf16 image
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    *reinterpret_cast<bf16x8*>(vimg + lds_off<D>(n * RPI + lane / CPR, 2 * (lane % CPR) + u)) =
                        e4m3x8_to_bf16(vf[DEC_SL][n][2 * u], vf[DEC_SL][n][2 * u + 1]);
            }
        }
        f32x16 s[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) s[i][e] = 0.0f;
#pragma unroll
        for (int t = 0; t < KS; ++t) {      // one K fragment, the product of every row tile
            bf16x8 kt;
            if constexpr (EB == 2)
                kt = __builtin_bit_cast(bf16x8, kf[DEC_SL][t]);
            else
                kt = e4m3x8_to_bf16(kf[DEC_SL][t / 2][2 * (t % 2)], kf[DEC_SL][t / 2][2 * (t % 2) + 1]);
#pragma unroll
            for (int i = 0; i < RT; ++i) s[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, q[i][t], s[i], 0, 0, 0);
        }
        load_tile(DEC_KB + PF * kDecodeKB, DEC_SL);
        if constexpr (PAGED) fetch_entry(DEC_KB + (PF + 1) * kDecodeKB);      // the table entry of the tile after the next one

        bf16x8 p[RT][2];
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            float mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[i][e] *= sc;
                if constexpr (WIN)
                    mx = DEC_KB + acc_row(e, h) < kmax[i] && DEC_KB + acc_row(e, h) >= kmin[i] ? fmaxf(mx, s[i][e]) : mx;
                else
                    mx = DEC_KB + acc_row(e, h) < kmax[i] ? fmaxf(mx, s[i][e]) : mx;
            }
            mx = half_max(mx);
            const float m_new = fmaxf(m[i], mx);
            const float m0 = m_new == -INFINITY ? 0.0f : m_new;
            const float alpha = __builtin_amdgcn_exp2f(m[i] - m0);      // m = -inf: 0, and there is nothing to scale yet
            m[i] = m_new;
            float ps = 0.0f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float pe;
                if constexpr (WIN)
                    pe = DEC_KB + acc_row(e, h) < kmax[i] && DEC_KB + acc_row(e, h) >= kmin[i] ? __builtin_amdgcn_exp2f(s[i][e] - m0) : 0.0f;
                else
                    pe = DEC_KB + acc_row(e, h) < kmax[i] ? __builtin_amdgcn_exp2f(s[i][e] - m0) : 0.0f;
                ps += pe;
                p[i][e >> 3][e & 7] = (__bf16)pe;
            }
            l[i] = l[i] * alpha + ps;
#pragma unroll
            for (int c = 0; c < DB; ++c)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[i][c][e] *= alpha;
        }
        // element j of half h of k-step ks is key 16 ks + 8 (j >> 2) + 4 h + (j & 3): two transposed reads of four keys each,
        // one V fragment for every row tile
#pragma unroll
        for (int c = 0; c < DB; ++c) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 vt;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int row = 16 * ks + 8 * u + 4 * h + qq, col = 32 * c + c0 + 4 * pp;
                    const bf16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                        (dec_lds_bf16x4*)(vimg + lds_off<D>(row, col >> 3) + 8 * (pp & 1)));
#pragma unroll
                    for (int e = 0; e < 4; ++e) vt[4 * u + e] = x[e];
                }
#pragma unroll
                for (int i = 0; i < RT; ++i) o[i][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt, p[i][ks], o[i][c], 0, 0, 0);
            }
        }
#undef DEC_KB
#undef DEC_SL
