// fa2_rope_ragged_owner.h -- which sequence owns a packed token of a ragged append (fa2_rope_kv_append_ragged, _paged;
// include/fa2_rope_ragged_mi355x.h).  The whole ownership rule, host and device, with no HIP in it: fa2_rope_append_ragged.hip
// takes a token's owner from this one function and nothing else, and tests/test_rope_ragged_owner.py compiles it into a host
// program and enumerates it against the plan model of tests/extend_ragged_ref.py.
//
// seq_pairs is what stands behind the 8-int header of the plan fa2_extend_ragged_plan filled: B pairs (start_b, q_b), the starts
// non-decreasing, an empty sequence sharing its start with its successor.  Token t belongs to the LAST b with start_b <= t (the
// upper bound over the starts, minus one) if that pair is valid -- start >= 0, q > 0, q <= T - start, the ragged extend's test --
// and t < start_b + q_b; otherwise to no sequence.  The search makes exactly `iters` steps, iters = ceil(log2 B) from the host
// (ragged_owner_iters): no trip count comes from the array.  WHATEVER the array holds, only seq_pairs[0 .. 2 B - 1] is read and
// an answer other than "none" has 0 <= b < B, 0 <= i < q and q = seq_pairs[2 b + 1] <= T: an array that is no plan can give a
// token to a wrong sequence, never an index out of range.
#ifndef FA2_ROPE_RAGGED_OWNER_H
#define FA2_ROPE_RAGGED_OWNER_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_ROPE_HD __host__ __device__
#else
#define FA2_ROPE_HD
#endif

namespace fa2 {

struct RaggedOwner {
    int b;      // the owning sequence, or -1: none
    int i;      // t - start_b: the token is number i of the sequence's q newest
    int q;      // q_b
};

// The search's trip count for B sequences: the smallest n with 2^n >= B (0 for B <= 1).
FA2_ROPE_HD inline int ragged_owner_iters(int B)
{
    int n = 0;
    while (n < 31 && (1LL << n) < B) ++n;
    return n;
}

FA2_ROPE_HD inline RaggedOwner ragged_owner(const int* seq_pairs, int B, int iters, int T, int t)
{
    const RaggedOwner none = {-1, 0, 0};
    if (t < 0 || t >= T || B < 1) return none;
    // b is the last index found with start <= t, taken to be 0 until the check below; bit k of it is decided at step k, so it
    // reaches every index below 2^iters and the sum never passes INT_MAX (iters <= 31)
    int b = 0;
    for (int k = iters - 1; k >= 0; --k) {
        const long long m = (long long)b + (1LL << k);
        if (m < B && seq_pairs[2 * m] <= t) b = (int)m;
    }
    const int start = seq_pairs[2 * (long long)b], q = seq_pairs[2 * (long long)b + 1];
    if (start < 0 || q <= 0 || q > T - start) return none;
    if (t < start || t - start >= q) return none;
    const RaggedOwner own = {b, t - start, q};
    return own;
}

}  // namespace fa2

#endif  // FA2_ROPE_RAGGED_OWNER_H
