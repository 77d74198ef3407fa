// fa2_kv_append_addr.h -- where an appended token goes (fa2_kv_append, fa2_kv_append_paged; include/fa2_kvcache_mi355x.h).
// The whole position and address rule of the append, host and device, with no HIP in it: fa2_kv_append.hip forms every
// destination through these three functions and nothing else, and tests/test_kv_append_addr.py compiles them into a host
// program and enumerates them against the reference model of tests/kv_append_ref.py.
//
// seqlens_k[b] is the length AFTER the append: token t of n_new goes to logical row pos = len - n_new + t.  It is WRITTEN iff
// 0 <= pos < capacity; every other token is dropped (a write is never clamped into range).  Paged: row pos is row
// pos % page_size of page block_table[b][pos / page_size], and a token whose table entry lies outside [0, n_pages) is dropped
// too -- the decode clamps such an entry, a write through the clamped entry would land in another sequence's page.
#ifndef FA2_KV_APPEND_ADDR_H
#define FA2_KV_APPEND_ADDR_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FA2_KV_HD __host__ __device__
#else
#define FA2_KV_HD
#endif

namespace fa2 {

constexpr long long kKvAppendDropped = -1;      // what the offset functions return for a token that is not written

// The logical row of token t (0 <= t < n_new), or -1: dropped.  64-bit, so no int32 len (INT_MIN, INT_MAX) overflows.
FA2_KV_HD inline int kv_append_pos(int len, int n_new, int t, int capacity)
{
    const long long pos = (long long)len - n_new + t;
    return pos >= 0 && pos < capacity ? (int)pos : -1;
}

// Element offset of row pos of head h of sequence b in a cache [B][H_kv][capacity][d]; pos is kv_append_pos's.
FA2_KV_HD inline long long kv_append_offset(int pos, int b, int h, int H_kv, int capacity, int d)
{
    if (pos < 0 || pos >= capacity) return kKvAppendDropped;
    return (((long long)b * H_kv + h) * capacity + pos) * d;
}

// Which entry of sequence b's table row a written token reads: pos / page_size, below max_pages_per_seq because
// pos < capacity = max_pages_per_seq x page_size.  Only call with pos >= 0.
FA2_KV_HD inline int kv_append_table_index(int pos, int page_size) { return pos / page_size; }

// Element offset of row pos of head h in a pool [n_pages][H_kv][page_size][d], `entry` being block_table[b][pos / page_size].
// 64-bit: a pool may exceed 4 GiB.
FA2_KV_HD inline long long kv_append_offset_paged(int pos, int entry, int n_pages, int h, int H_kv, int page_size, int d)
{
    if (pos < 0 || entry < 0 || entry >= n_pages) return kKvAppendDropped;
    return (((long long)entry * H_kv + h) * page_size + pos % page_size) * d;
}

}  // namespace fa2

#endif  // FA2_KV_APPEND_ADDR_H
