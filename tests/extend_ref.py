"""Extend attention (fa2_forward_extend, fa2_forward_extend_paged; include/fa2_extend_mi355x.h): the cases, their inputs, the float64
reference and a model of the kernels' row blocks in Python integers (a helper module, no tests: tests/test_extend_reference.py
certifies what is here on the CPU, tests/test_gpu_extend.py runs the kernels on it).

THE PROBLEM.  decode_ref's (decode_window_ref's under a window) with any M = (H_q / H_kv) N_q.  The rows of a K/V head are the
slab [G][N_q]: row rho is head rho // N_q of the group and token rho % N_q; a workgroup takes 64 of them.

CASES.  SHAPES are the smallest at which the new code can go wrong (M = 33: one row in the second tile, MQA at N_q 1; 40; 64: one
full block; 65: a second block of one row; 68: head boundaries inside tiles; 96: a last block of one tile; G = 1 with 70 tokens;
160), each at d = 64 and 128 over ONE batch of the lengths 0, 1, N_q - 1, N_q, 127, 128, 129, 300, 1100, 2500 in a cache of 2560;
two more have seqlens_k = None.  A case is run under VARIANTS: the causal mask, no mask, and the causal mask with each window of
WINDOWS; the sink alternates over (case, variant).  Sequences 8 and 9 share their first 192 keys, so their first pages can be
SHARED in a pool (shared_pages).

REFERENCE (reference64): decode_paged_ref.reference64 -- regimes.ref_attention, sink_ref.ref_attention_sink per sequence -- without
a window, decode_window_ref.reference64 with one; e4m3 caches through decode_fp8kv_ref's quantise / dequantise.
GATES: decode_ref.errors / within_gates, unchanged, for bf16 and e4m3 caches alike (as tests/test_gpu_decode_window.py uses them),
and the row gate of O of tests/decode_rows_ref.py (the references carry its term)."""
import functools

import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_window_ref as wr

KB, TILE, WAVES = dr.KB, dr.TILE, dr.WAVES
ROWS = 64                 # kExtendRows: the rows of one workgroup, two 32-row tiles per wave
N_CAP = 2560
SHAPES = ((33, 1, 1), (8, 1, 5), (16, 2, 8), (13, 1, 5), (8, 2, 17), (8, 2, 24), (4, 4, 70), (8, 2, 40))      # (H_q, H_kv, N_q)
SPLITS = (0, 1, 2, 7, 64)
WINDOWS = (0, 1, 31, 127, 128, 200, N_CAP - 1)
PAGE_SIZES = (32, 96)
SHARED_KEYS = 192         # a whole number of pages of either size
VARIANTS = (("causal", None), ("full", None)) + tuple(("causal", w) for w in WINDOWS)      # (mask, window_left)


def lens_of(nq):
    return (0, 1, nq - 1, nq, KB - 1, KB, KB + 1, 300, 1100, 2500)


def _cases():
    out = [dr._case(hq, hkv, d, nq, True, lens_of(nq), N_CAP, sink=False, splits=SPLITS) for (hq, hkv, nq) in SHAPES for d in (64, 128)]
    for (hq, hkv, nq), d in (((8, 1, 5), 64), ((8, 2, 24), 128)):      # seqlens_k = None: every sequence has the capacity
        out.append(dr._case(hq, hkv, d, nq, True, (300, 300), 300, sink=False, splits=SPLITS, seqlens=False))
    return tuple(out)


CASES = _cases()
SLICED = tuple(i for i, c in enumerate(CASES) if c["nq"] <= dr.MAX_ROWS)      # a group member's rows are a call of the shipped kernels


def rows_of(c):
    return c["hq"] // c["hkv"] * c["nq"]


def case_id(c):
    return f"{c['hq']}-{c['hkv']}-q{c['nq']}-d{c['d']}" + ("" if c["seqlens"] else "-nolens")


def variant_id(v):
    return v[0] if v[1] is None else f"w{v[1]}"


IDS = [case_id(c) for c in CASES]
RUNS = tuple((i, k) for i in range(len(CASES)) for k in range(len(VARIANTS)))
RUN_IDS = [f"{IDS[i]}-{variant_id(VARIANTS[k])}" for i, k in RUNS]


def has_sink(i, k):
    return (i + k) % 2 == 1


@functools.lru_cache(maxsize=4)
def inputs(i):
    """Host tensors of CASES[i] (made once, never written), decode_ref's recipe: (Q, K, V, scale, lens int32, sink [hq])."""
    c = CASES[i]
    B, d, ncap = len(c["lens"]), c["d"], c["ncap"]
    g = torch.Generator().manual_seed(97000 + 31 * i)
    mk = lambda h, n, s: ((torch.rand(B, h, n, d, generator=g) - 0.5) * s).bfloat16()
    Q, K, V = mk(c["hq"], c["nq"], 1.0), mk(c["hkv"], ncap, 8.0), mk(c["hkv"], ncap, 8.0)      # the caches start as garbage
    for b, n in enumerate(c["lens"]):
        K[b, :, :n] /= 8.0
        V[b, :, :n] /= 8.0
    if c["seqlens"]:
        K[9, :, :SHARED_KEYS], V[9, :, :SHARED_KEYS] = K[8, :, :SHARED_KEYS], V[8, :, :SHARED_KEYS]
    return Q, K, V, 1.0 / d ** 0.5, torch.tensor(c["lens"], dtype=torch.int32), dr.sink_of(c["hq"], 277 + i)


@functools.lru_cache(maxsize=4)
def inputs_fp8(i):
    """inputs(i) with the caches quantised to e4m3, a distinct descale per head that is no power of two (decode_window_ref's):
    (Q, K8, V8, k_descale, v_descale, scale, lens, sink)."""
    Q, K, V, scale, lens, sink = inputs(i)
    K8, kd = fr.quantise(K, headroom=0.25)
    V8, vd = fr.quantise(V, headroom=0.375)
    return Q, K8, V8, kd * 1.0625, vd * 1.1875, scale, lens, sink


@functools.lru_cache(maxsize=4)
def dequantised(i):
    _, K8, V8, kd, vd, _, _, _ = inputs_fp8(i)
    return fr.dequantise(K8, kd), fr.dequantise(V8, vd)


def reference64(Q, K, V, lens, scale, causal, sink, wl):
    """float64 O [B, hq, nq, d] and L [B, hq, nq] on contiguous host caches; wl = None: no window."""
    if wl is None:
        return pr.reference64(Q, K, V, [int(n) for n in lens], scale, causal, sink)
    assert causal
    return wr.reference64(Q, K, V, lens, scale, sink, wl)


@functools.lru_cache(maxsize=8)
def reference(i, k, fp8=False):
    """The float64 reference of CASES[i] under VARIANTS[k] (fp8: on the dequantised caches), computed once and never written."""
    c = CASES[i]
    mask, wl = VARIANTS[k]
    Q, K, V, scale, _, sink = inputs(i)
    if fp8:
        K, V = dequantised(i)
    return reference64(Q, K, V, c["lens"], scale, mask == "causal", sink if has_sink(i, k) else None, wl)


@functools.lru_cache(maxsize=4)
def paged_inputs(i, P, fp8=False):
    """CASES[i] behind pages of P keys (decode_paged_ref.build: permuted pages, NaN where no key was copied, unused entries -1 and
    INT_MAX) with the first SHARED_KEYS / P pages of sequence 9 SHARED with sequence 8: (K_pages, V_pages, table, capacity)."""
    c = CASES[i]
    full = not c["seqlens"]
    if fp8:
        _, K8, V8 = inputs_fp8(i)[:3]
        Kp, Vp, table, _ = fr.pools(K8, V8, c["lens"], P, 98000 + 17 * i + P, full=full)
    else:
        _, K, V = inputs(i)[:3]
        Kp, Vp, table = pr.build(K, V, c["lens"], P, 98000 + 17 * i + P, full=full)
    shared_pages(c, table, P)
    return Kp, Vp, table, table.shape[1] * P


def shared_pages(c, table, P):
    """Sequence 9 reads its first SHARED_KEYS keys through sequence 8's pages (in place; the cases with lengths only)."""
    if c["seqlens"]:
        table[9, :SHARED_KEYS // P] = table[8, :SHARED_KEYS // P]
    return table


def lens_under(c, cap):
    """The lengths the kernels see: the case's, or the capacity where seqlens_k is None."""
    return list(c["lens"]) if c["seqlens"] else [cap] * len(c["lens"])


# ---- the kernels' row blocks and their clip, in Python integers (extend_split_body, csrc/fa2_decode.hip)
def split_range(n, nq, wl, n_splits, s):
    """Keys [begin, end) of split s: the siblings' rule (decode_ref.split_range, decode_window_ref.window_range)."""
    return dr.split_range(n, n_splits, s) if wl is None else wr.window_range(n, nq, wl, n_splits, s)


def row_window(rho, nq, n, causal, wl):
    """Keys [kmin, kmax) row rho of a group sees in a sequence of n keys (kmax <= kmin: none)."""
    pos = rho % nq + n - nq
    return (max(pos - wl, 0) if wl is not None else 0), (min(pos + 1, n) if causal else n)


def block_tiles(M, nq, n, causal, wl, n_splits, s, j):
    """{wave: [first key of each 32-key tile it processes]} of row block j (rows 64 j ..+64 of M) in split s of a sequence of n
    keys, or None where the block takes the empty-split exit.  The waves take a split's tiles round-robin counted from the
    split's first key; the block stops at the largest kmax of its rows and, under a window, every wave starts at the first of
    its tiles at or behind the tile that holds the smallest kmin of its rows."""
    begin, end = split_range(n, nq, wl, n_splits, s)
    r0, r1 = ROWS * j, min(ROWS * (j + 1), M) - 1
    wrap = r0 // nq != r1 // nq
    tlo, thi = (0, nq - 1) if wrap else (r0 % nq, r1 % nq)
    if causal:
        end = min(end, thi + n - nq + 1)
    cstart = 0
    if wl is not None:
        cstart = max(tlo + n - nq - wl, 0) // TILE * TILE
    if begin >= end or (wl is not None and cstart >= end):
        return None
    out = {}
    for w in range(WAVES):
        kb = begin + TILE * w
        if wl is not None and cstart > kb:
            kb += -(-(cstart - kb) // KB) * KB
        out[w] = list(range(kb, end, KB))
    return out


def resolved_splits(c, wl, n_splits, ncap=None):
    """What n_splits = 0 stands for (fa2_extend_num_splits): the siblings' rule with B H_kv ceil(M / 64) workgroups above 32 rows."""
    if n_splits:
        return n_splits
    ncap = ncap or c["ncap"]
    M = rows_of(c)
    keys = ncap if wl is None or wl >= ncap - 1 else min(ncap, wl + c["nq"] + KB - 1)
    groups = len(c["lens"]) * c["hkv"] * (1 if M <= dr.MAX_ROWS else -(-M // ROWS))
    return min(-(-256 // groups), max(1, keys // dr.MIN_SPLIT_KEYS), 256)
