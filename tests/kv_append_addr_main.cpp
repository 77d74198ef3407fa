// A host program around cuda_flashattention_amd/csrc/fa2_kv_append_addr.h, the append's position and address rule
// (tests/test_kv_append_addr.py builds and drives it; no HIP call, no device).  One query per input line:
//     len n_new t capacity  b h H_kv d  entry n_pages page_size
// and one answer per line: pos  contiguous_offset  table_index  paged_offset   (-1: dropped; table_index -1 when pos is).
#include <cstdio>

#include "fa2_kv_append_addr.h"

int main()
{
    int len, n_new, t, cap, b, h, H, d, entry, n_pages, P;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d", &len, &n_new, &t, &cap, &b, &h, &H, &d, &entry, &n_pages, &P) == 11) {
        const int pos = fa2::kv_append_pos(len, n_new, t, cap);
        const long long off = fa2::kv_append_offset(pos, b, h, H, cap, d);
        const int ti = pos >= 0 ? fa2::kv_append_table_index(pos, P) : -1;
        const long long offp = fa2::kv_append_offset_paged(pos, entry, n_pages, h, H, P, d);
        std::printf("%d %lld %d %lld\n", pos, off, ti, offp);
    }
    return 0;
}
