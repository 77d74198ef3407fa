// fa2_decode_combine.inc -- one row piece of the combine kernels (fa2_decode.hip): the lane owns columns 4 c4 ..+4 of row `row`
// of the R rows of O, L and of every split's partials; DEC_NQ is the number of consecutive rows that share a head (the sink's
// index).  Included text and not a function: fa2_decode_combine_kernel came out of the compiler with other registers when its
// body was called through one (tools/asm_identity.py against the parent).
    // The partials of a row are loaded kCombineBatch at a time, all loads of a batch ahead of their use: the loop is a chain of
    // memory latencies, one per batch, and summing split after split behind its own load made it four times as long (the
    // summation order stays ascending s).  Indices past the last split are clamped and their terms selected away.
    const int last = a.n_splits - 1;
    float m = -INFINITY;
    for (int s0 = 0; s0 < a.n_splits; s0 += 2 * kCombineBatch) {
        float ls[2 * kCombineBatch];
#pragma unroll
        for (int i = 0; i < 2 * kCombineBatch; ++i) ls[i] = a.wsL[(size_t)min(s0 + i, last) * R + row];
#pragma unroll
        for (int i = 0; i < 2 * kCombineBatch; ++i) m = fmaxf(m, ls[i]);
    }
    const float m0 = m == -INFINITY ? 0.0f : m;
    float sum = 0.0f;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s0 = 0; s0 < a.n_splits; s0 += kCombineBatch) {
        float ls[kCombineBatch];
        f32x4 os[kCombineBatch];
#pragma unroll
        for (int i = 0; i < kCombineBatch; ++i) {
            const size_t at = (size_t)min(s0 + i, last) * R + row;
            ls[i] = a.wsL[at];
            os[i] = *reinterpret_cast<const f32x4*>(a.wsO + at * D + 4 * c4);
        }
#pragma unroll
        for (int i = 0; i < kCombineBatch; ++i) {
            const bool has = s0 + i <= last && ls[i] != -INFINITY;      // a select: an empty split's O_s is left out
            const float w = __builtin_amdgcn_exp2f((ls[i] - m0) * kLog2e);
            sum += has ? w : 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = has ? acc[e] + w * os[i][e] : acc[e];
        }
    }
    const bool none = m == -INFINITY;
    float Lrow = none ? -INFINITY : m + __builtin_amdgcn_logf(sum) * kDecLn2;
    const float inv = 1.0f / sum;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = none ? 0.0f : acc[e] * inv;
    float w = 1.0f;
    if (a.sink) w = decode_sink(a.sink[(row / DEC_NQ) % a.Hq], Lrow);
    *reinterpret_cast<bf16x4*>((__bf16*)a.O + row * D + 4 * c4) = to_bf16x4(acc, w);
    if (c4 == 0) a.L[row] = Lrow;
#undef DEC_NQ
