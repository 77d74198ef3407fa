// A host program around cuda_flashattention_amd/csrc/fa2_rope_ragged_owner.h, the ragged append's ownership rule
// (tests/test_rope_ragged_owner.py builds and drives it; no HIP call, no device).  Input: one problem after another,
//     B T  then the 2 B ints of the pair array (start_0 q_0 start_1 q_1 ...)
// The array is copied into a heap block of exactly 2 B ints, so a sanitiser build sees any read outside it.  Output per
// problem: a line "iters" and then, for every t in -1 .. T, a line "b i q" (b = -1: no owner).
#include <cstdio>
#include <vector>

#include "fa2_rope_ragged_owner.h"

int main()
{
    int B, T;
    while (std::scanf("%d %d", &B, &T) == 2) {
        std::vector<int> pairs(2 * (size_t)B);
        for (int& v : pairs)
            if (std::scanf("%d", &v) != 1) return 1;
        const int iters = fa2::ragged_owner_iters(B);
        std::printf("%d\n", iters);
        for (int t = -1; t <= T; ++t) {
            const fa2::RaggedOwner o = fa2::ragged_owner(pairs.data(), B, iters, T, t);
            std::printf("%d %d %d\n", o.b, o.i, o.q);
        }
    }
    return 0;
}
