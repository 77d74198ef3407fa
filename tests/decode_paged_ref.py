"""Paged decode attention (fa2_forward_decode_paged): page pools and block tables built from tests/decode_ref.py's cases, and the
page-edge batch (a helper module, no tests: tests/test_decode_paged_reference.py certifies what is here on the CPU,
tests/test_gpu_decode_paged.py runs the kernels on it).

THE PROBLEM (include/fa2_mi355x.h).  K and V live in pools [n_pages, H_kv, page_size, d]; logical key j of sequence b is row
j % page_size of page block_table[b, j // page_size]; the capacity is max_pages * page_size.  Everything else is decode_ref's.

WHAT build() MAKES, the worst a caller may legally hand over: a pool of B * max_pages + 5 pages pre-filled with NaN; a seeded
permutation that assigns pages to (sequence, logical page), so no sequence's pages are in order or adjacent; only rows < len_b
copied in, so the tail of each last page and every spare page stay NaN; a table whose unused entries alternate -1 and 0x7fffffff.
gather() is the inverse: the contiguous [B, H_kv, max_pages * page_size, d] cache the pool and the table stand for (zeros where
no page is in use), which is what flash_attention_2_decode and the float64 reference read.

PAGE_SIZES: 32 (the four waves of one 128-key round in four pages), 64 (two pages per round), 96 (not a power of two: pages
straddle the 128-key blocks unevenly), 128 (one page per round), 256 (two rounds per page)."""
import functools

import numpy as np
import torch

import decode_ref as dr
import decode_rows_ref as rows
import regimes
from sink_ref import ref_attention_sink

PAGE_SIZES = (32, 64, 96, 128, 256)
SPLITS = (0, 1, 2, 7, 64)
SPARE_PAGES = 5
UNUSED = (-1, 0x7FFFFFFF)
FILLS = {"nan": float("nan"), "3e38": 3e38, "zero": 0.0}


def _first(**want):
    return next(i for i, c in enumerate(dr.CASES) if all(c[k] == v for k, v in want.items()))


# the cases test_gpu_decode.py feeds garbage to (re-derived: the same three selections)
GARBAGE_CASES = (_first(hq=8, hkv=2, d=128, nq=4, causal=True, regime=None, seqlens=True),
                 _first(hq=8, hkv=1, d=64, nq=4, causal=False, regime=None, seqlens=True),
                 _first(hq=3, hkv=3, d=128, nq=1, causal=True, regime=None, seqlens=True))
M32_CASES = tuple(_first(hq=32, hkv=1, d=d) for d in (64, 128))                   # M = 32 from the heads alone
NOLENS_CASE = _first(seqlens=False, ncap=300)                                    # seqlens_k = None: every sequence has the capacity
REGIME_CASE = _first(regime="spikes", d=128)
BIT_CASES = GARBAGE_CASES + M32_CASES + (NOLENS_CASE, REGIME_CASE)


def pages_for(n, page_size):
    return -(-n // page_size)


def build(K, V, lens, page_size, seed, fill=float("nan"), unused=UNUSED, full=False):
    """(K_pages, V_pages, block_table int32 [B, max_pages]) of contiguous host caches K, V [B, hkv, ncap, d] of which sequence b uses
    lens[b] rows.  full: every sequence uses the whole capacity max_pages * page_size (seqlens_k = None); the rows past ncap are
    seeded random data."""
    B, hkv, ncap, d = K.shape
    max_pages = pages_for(ncap, page_size)
    cap = max_pages * page_size
    g = torch.Generator().manual_seed(seed)
    if full:
        pad = lambda t: torch.cat([t, (torch.rand(B, hkv, cap - ncap, d, generator=g) - 0.5).bfloat16()], dim=2)
        K, V, lens = pad(K), pad(V), [cap] * B
    n_pages = B * max_pages + SPARE_PAGES
    perm = torch.randperm(n_pages, generator=g)
    pools = [torch.full((n_pages, hkv, page_size, d), fill, dtype=torch.bfloat16) for _ in range(2)]
    table = torch.empty(B, max_pages, dtype=torch.int32)
    for b in range(B):
        n = int(lens[b])
        for p in range(max_pages):
            if p < pages_for(n, page_size):
                page = int(perm[b * max_pages + p])
                rows = min(page_size, n - p * page_size)
                for pool, t in zip(pools, (K, V)):
                    pool[page, :, :rows] = t[b, :, p * page_size:p * page_size + rows]
                table[b, p] = page
            else:
                table[b, p] = unused[(b * max_pages + p) % len(unused)]
    return pools[0], pools[1], table


def gather(pool, table, lens, page_size):
    """The contiguous cache [B, hkv, max_pages * page_size, d] a pool and a table stand for: the pages of the entries in use (those
    below ceil(len_b / page_size)), whole, zeros elsewhere.  Works on host and device tensors."""
    B, max_pages = table.shape
    out = torch.zeros(B, pool.shape[1], max_pages * page_size, pool.shape[3], dtype=pool.dtype, device=pool.device)
    host = table.cpu()
    for b in range(B):
        for p in range(pages_for(int(lens[b]), page_size)):
            out[b, :, p * page_size:(p + 1) * page_size] = pool[int(host[b, p])]
    return out


@functools.lru_cache(maxsize=None)
def paged_inputs(i, page_size, fill="nan", zero_unused=False):
    """CASES[i] of decode_ref as (K_pages, V_pages, table, lens list, capacity), made once and never written.  fill: a name in
    FILLS, what the pool holds where no key was copied; zero_unused: the table's unused entries are 0."""
    c = dr.CASES[i]
    _, K, V, _, _, _ = dr.inputs(i)
    Kp, Vp, table = build(K, V, c["lens"], page_size, 91000 + 17 * i + page_size, fill=FILLS[fill],
                          unused=(0, 0) if zero_unused else UNUSED, full=not c["seqlens"])
    cap = table.shape[1] * page_size
    return Kp, Vp, table, ([cap] * len(c["lens"]) if not c["seqlens"] else list(c["lens"])), cap


def reference64(Q, K, V, lens, scale, causal, sink):
    """float64 O [B, hq, nq, d] and L [B, hq, nq] on contiguous host caches: decode_ref.reference's rule for any batch, with the
    row gate's .quad beside them (decode_rows_ref.Ref)."""
    G = Q.shape[1] // K.shape[1]
    O, L = np.zeros(tuple(Q.shape)), np.zeros(tuple(Q.shape[:3]))
    for b, n in enumerate(lens):
        q = regimes.f64(Q[b])
        k, v = (np.repeat(regimes.f64(t[b, :, :n]), G, axis=0) for t in (K, V))
        if sink is None:
            O[b], L[b] = regimes.ref_attention(q, k, v, np.zeros_like(q), scale, causal)[:2]
        else:
            O[b], L[b] = ref_attention_sink(q, k, v, np.zeros_like(q), scale, causal, sink.double().numpy())[:2]
    return rows.Ref(O, L, rows.quad64(Q, K, V, lens, scale, causal, sink))


@functools.lru_cache(maxsize=None)
def paged_reference(i, page_size):
    """The float64 reference of CASES[i] behind pages: decode_ref's own where the lengths are the case's; with seqlens_k = None the
    sequences have the capacity, which depends on the page size."""
    c = dr.CASES[i]
    if c["seqlens"]:
        return dr.reference(i)
    Q, _, _, scale, _, sink = dr.inputs(i)
    Kp, Vp, table, lens, _ = paged_inputs(i, page_size)
    return reference64(Q, gather(Kp, table, lens, page_size), gather(Vp, table, lens, page_size), lens, scale, c["causal"], sink)


# ---- the page-edge batch: one per page size P, lengths at every edge of a page, 8 heads on 2, N_q = 4, causal
EDGE_NCAP = 2560


def edge_lens(P):
    return (2500, P - 1, P, P + 1, 2 * P - 1, 2 * P + 1, 0, 1, 3 * P)


def edge_case(P, d):
    """A case record in decode_ref's form (ncap is the paged capacity)."""
    return dict(hq=8, hkv=2, d=d, nq=4, causal=True, lens=edge_lens(P), ncap=pages_for(EDGE_NCAP, P) * P, sink=d == 64, regime=None,
                splits=SPLITS, seqlens=True)


@functools.lru_cache(maxsize=None)
def edge_inputs(P, d):
    """(Q, K_pages, V_pages, table, scale, lens int32, sink) of the edge batch, host tensors made once."""
    c = edge_case(P, d)
    B = len(c["lens"])
    g = torch.Generator().manual_seed(64000 + 13 * P + d)
    mk = lambda h, n: (torch.rand(B, h, n, d, generator=g) - 0.5).bfloat16()
    Q, K, V = mk(c["hq"], c["nq"]), mk(c["hkv"], EDGE_NCAP), mk(c["hkv"], EDGE_NCAP)
    Kp, Vp, table = build(K, V, c["lens"], P, 65000 + 13 * P + d)
    sink = dr.sink_of(c["hq"], 300 + P) if c["sink"] else None
    return Q, Kp, Vp, table, 1.0 / d ** 0.5, torch.tensor(c["lens"], dtype=torch.int32), sink


@functools.lru_cache(maxsize=None)
def edge_gathered(P, d):
    _, Kp, Vp, table, _, lens, _ = edge_inputs(P, d)
    return gather(Kp, table, lens.tolist(), P), gather(Vp, table, lens.tolist(), P)


@functools.lru_cache(maxsize=None)
def edge_reference(P, d):
    Q, _, _, _, scale, lens, sink = edge_inputs(P, d)
    K, V = edge_gathered(P, d)
    return reference64(Q, K, V, lens.tolist(), scale, True, sink)
