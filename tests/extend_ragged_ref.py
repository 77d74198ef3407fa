"""Ragged extend attention (fa2_forward_extend_ragged, _paged; include/fa2_extend_ragged_mi355x.h): the cases, their inputs, the
float64 reference, and Python-integer models of the plan kernel and of a workgroup's clip (a helper module, no tests:
tests/test_extend_ragged_reference.py certifies what is here on the CPU, tests/test_gpu_extend_ragged.py runs the kernels on it).

THE PROBLEM.  extend_ref's with a q_len per sequence: sequence b owns tokens cu[b] .. cu[b + 1] - 1 of the T packed ones, Q and O
are [T, H_q, d], L is [T, H_q]; everything extend_ref defines with N_q uses q_b.

CASES, the smallest batches at which the new code can go wrong, each at d = 64 and 128 in a capacity of 2560:
  mixed   (8, 2)   q_b = 0 1 8 9 16 17 1 40 3 0   M_b = 0 4 32 36 64 68 4 160 12 0: empty sequences first, last and in the middle,
                   exactly one tile, one row in the second tile, exactly one block, a second block, head boundaries inside tiles
  mqa     (33, 1)  1 1 2 0 1                      a wide MQA group
  g1      (4, 4)   70 1 64 65 33                  one head per K/V head
  decode  (16, 2)  ten times 1                    a pure decode batch
  nolens  (8, 1)   5 24                           seqlens_k = None at a capacity of 300
The lengths come from {0, 1, q_b - 1, q_b, 127, 128, 129, 300, 1100, 2500}; every case with lengths has a sequence with
len_b < q_b, one with len_b = q_b, and one on each side of a 128-key boundary.  A case is run under extend_ref.VARIANTS (the
causal mask, no mask, the causal mask with each window); the sink alternates over (case, variant).  SHARE: two sequences that share
their first 192 keys, so their first pages can be shared in a pool.

REFERENCE: per sequence, extend_ref.reference64 (decode_paged_ref.reference64 / decode_window_ref.reference64) on the transposed
slice [1, H_q, q_b, d].  GATES: decode_ref.errors / within_gates, unchanged, over all T H_q rows at once, and the row gate of O of
tests/decode_rows_ref.py on each of them."""
import functools

import numpy as np
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows
import extend_ref as er

ROWS, KB, TILE, WAVES = er.ROWS, er.KB, er.TILE, er.WAVES
N_CAP = er.N_CAP
SPLITS = (0, 1, 2, 7, 64)
PAGE_SIZES = (32, 96)
SHARED_KEYS = er.SHARED_KEYS
VARIANTS = er.VARIANTS
HEADER = 8                # kRaggedPlanHeader
INT_MAX = 2 ** 31 - 1

# name, (H_q, H_kv), q_b, len_b, the pair of sequences that share their first SHARED_KEYS keys (or None)
BATCHES = (
    ("mixed", (8, 2), (0, 1, 8, 9, 16, 17, 1, 40, 3, 0), (300, 0, 8, 8, 128, 129, 127, 2500, 1100, 1), (7, 8)),
    ("mqa", (33, 1), (1, 1, 2, 0, 1), (127, 129, 1, 128, 1), None),
    ("g1", (4, 4), (70, 1, 64, 65, 33), (1100, 0, 64, 129, 127), None),
    ("decode", (16, 2), (1,) * 10, (0, 1, 127, 128, 129, 300, 1100, 2500, 1, 0), (6, 7)),
)


def _case(name, heads, qs, lens, share, d, ncap=N_CAP, seqlens=True):
    return dict(name=name, hq=heads[0], hkv=heads[1], qs=tuple(qs), lens=tuple(lens), share=share, d=d, ncap=ncap, seqlens=seqlens,
                splits=SPLITS)


def _cases():
    out = [_case(*b, d) for b in BATCHES for d in (64, 128)]
    out += [_case("nolens", (8, 1), (5, 24), (300, 300), None, d, ncap=300, seqlens=False) for d in (64, 128)]
    return tuple(out)


CASES = _cases()
IDS = [f"{c['name']}-d{c['d']}" for c in CASES]
RUNS = tuple((i, k) for i in range(len(CASES)) for k in range(len(VARIANTS)))
RUN_IDS = [f"{IDS[i]}-{er.variant_id(VARIANTS[k])}" for i, k in RUNS]


def has_sink(i, k):
    return (i + k) % 2 == 1


def cu_of(qs):
    out = [0]
    for q in qs:
        out.append(out[-1] + q)
    return out


def total_q(c):
    return sum(c["qs"])


@functools.lru_cache(maxsize=4)
def inputs(i):
    """Host tensors of CASES[i] (made once, never written), extend_ref's recipe: (Q [T, hq, d], K, V [B, hkv, ncap, d], scale,
    lens int32, sink [hq], cu int32 [B + 1])."""
    c = CASES[i]
    B, d, ncap, T = len(c["lens"]), c["d"], c["ncap"], total_q(c)
    g = torch.Generator().manual_seed(99000 + 31 * i)
    Q = (torch.rand(T, c["hq"], d, generator=g) - 0.5).bfloat16()
    mk = lambda: ((torch.rand(B, c["hkv"], ncap, d, generator=g) - 0.5) * 8.0).bfloat16()      # the caches start as garbage
    K, V = mk(), mk()
    for b, n in enumerate(c["lens"]):
        K[b, :, :n] /= 8.0
        V[b, :, :n] /= 8.0
    if c["share"]:
        s, t = c["share"]
        K[t, :, :SHARED_KEYS], V[t, :, :SHARED_KEYS] = K[s, :, :SHARED_KEYS], V[s, :, :SHARED_KEYS]
    return (Q, K, V, 1.0 / d ** 0.5, torch.tensor(c["lens"], dtype=torch.int32), dr.sink_of(c["hq"], 311 + i),
            torch.tensor(cu_of(c["qs"]), dtype=torch.int32))


@functools.lru_cache(maxsize=4)
def inputs_fp8(i):
    """inputs(i) with the caches quantised to e4m3, a distinct descale per head that is no power of two (extend_ref's):
    (Q, K8, V8, k_descale, v_descale, scale, lens, sink, cu)."""
    Q, K, V, scale, lens, sink, cu = inputs(i)
    K8, kd = fr.quantise(K, headroom=0.25)
    V8, vd = fr.quantise(V, headroom=0.375)
    return Q, K8, V8, kd * 1.0625, vd * 1.1875, scale, lens, sink, cu


@functools.lru_cache(maxsize=4)
def dequantised(i):
    _, K8, V8, kd, vd = inputs_fp8(i)[:5]
    return fr.dequantise(K8, kd), fr.dequantise(V8, vd)


def reference64(Q, K, V, qs, lens, scale, causal, sink, wl):
    """float64 O [T, hq, d] and L [T, hq] of a packed batch on contiguous host caches: extend_ref.reference64 per sequence on the
    transposed slice; tokens past the last sequence (T > sum q_b) stay NaN -- no sequence owns them.  The row gate's .quad [T, hq]
    comes with them (decode_rows_ref.Ref)."""
    T, hq, d = Q.shape
    O, L, quad = np.full((T, hq, d), np.nan), np.full((T, hq), np.nan), np.full((T, hq), np.nan)
    t = 0
    for b, q in enumerate(qs):
        if q:
            Qb = Q[t:t + q].transpose(0, 1)[None]
            rb = er.reference64(Qb, K[b:b + 1], V[b:b + 1], [int(lens[b])], scale, causal, sink, wl)
            O[t:t + q], L[t:t + q], quad[t:t + q] = (np.swapaxes(x[0], 0, 1) for x in (*rb, rb.quad))
        t += q
    return rows.Ref(O, L, quad)


@functools.lru_cache(maxsize=8)
def reference(i, k, fp8=False):
    """The float64 reference of CASES[i] under VARIANTS[k] (fp8: on the dequantised caches), computed once and never written."""
    c = CASES[i]
    mask, wl = VARIANTS[k]
    Q, K, V, scale, _, sink, _ = inputs(i)
    if fp8:
        K, V = dequantised(i)
    return reference64(Q, K, V, c["qs"], c["lens"], scale, mask == "causal", sink if has_sink(i, k) else None, wl)


def shared_pages(c, table, P):
    """The second sequence of SHARE reads its first SHARED_KEYS keys through the first one's pages (in place)."""
    if c["share"]:
        s, t = c["share"]
        table[t, :SHARED_KEYS // P] = table[s, :SHARED_KEYS // P]
    return table


@functools.lru_cache(maxsize=4)
def paged_inputs(i, P, fp8=False):
    """CASES[i] behind pages of P keys (decode_paged_ref.build: permuted pages, NaN where no key was copied, unused entries -1 and
    INT_MAX) with SHARE's pages shared: (K_pages, V_pages, table, capacity)."""
    c = CASES[i]
    full = not c["seqlens"]
    if fp8:
        _, K8, V8 = inputs_fp8(i)[:3]
        Kp, Vp, table, _ = fr.pools(K8, V8, c["lens"], P, 99500 + 17 * i + P, full=full)
    else:
        _, K, V = inputs(i)[:3]
        Kp, Vp, table = pr.build(K, V, c["lens"], P, 99500 + 17 * i + P, full=full)
    shared_pages(c, table, P)
    return Kp, Vp, table, table.shape[1] * P


def lens_under(c, cap):
    """The lengths the kernels see: the case's, or the capacity where seqlens_k is None."""
    return list(c["lens"]) if c["seqlens"] else [cap] * len(c["lens"])


# ---- the host formulas, restated (include/fa2_extend_ragged_mi355x.h)
def max_blocks(B, hq, hkv, T):
    return (hq // hkv) * T // ROWS + min(B, T)


def plan_ints(B, hq, hkv, T):
    return HEADER + 2 * B + 2 * max_blocks(B, hq, hkv, T)


def plan_bytes(B, hq, hkv, T):
    return (plan_ints(B, hq, hkv, T) * 4 + 15) // 16 * 16


def num_splits(B, hq, hkv, T, cap, wl):
    """What n_splits = 0 stands for: the siblings' rule on H_kv max(min(B, T), ceil(G T / 64)) workgroups."""
    keys = cap if wl is None or wl < 0 or wl >= cap - 1 else min(cap, wl + T + KB - 1)
    groups = hkv * max(min(B, T), -(-(hq // hkv) * T // ROWS))
    return min(-(-256 // groups), max(1, keys // dr.MIN_SPLIT_KEYS), 256)


def workspace_bytes(hq, T, d, n):
    return 0 if n == 1 else (n * T * hq * (d + 1) * 4 + 255) // 256 * 256


# ---- the plan kernel in Python integers (fa2_extend_ragged_plan_kernel, csrc/fa2_decode.hip)
def sanitised(cu, T):
    """[(start_b, q_b)] of ANY list of B + 1 ints: the running maximum clamped to [0, T]."""
    c, run = [], -2 ** 31
    for v in cu:
        run = max(run, int(v))
        c.append(min(max(run, 0), T))
    return [(c[b], c[b + 1] - c[b]) for b in range(len(cu) - 1)]


def plan_model(cu, G, T):
    """The plan's ints, header | seq | items, exactly as the kernel stores them."""
    B = len(cu) - 1
    seq = sanitised(cu, T)
    mb = G * T // ROWS + min(B, T)
    items = [(b, j) for b, (_, q) in enumerate(seq) for j in range(-(-G * q // ROWS))]
    assert len(items) <= mb
    first, last = min(max(int(cu[0]), 0), T), min(max(max(int(v) for v in cu), 0), T)
    out = [B, G, T, len(items), first, last, 0, 0]
    for s in seq:
        out += list(s)
    for it in items + [(-1, 0)] * (mb - len(items)):
        out += list(it)
    return out


def plan_rows(plan, G):
    """{(token, head of the group): work item} of a plan's ints as a workgroup of K/V head 0 decodes them -- every live row of
    every item; raises where two items claim a row."""
    B, T, n_items = plan[0], plan[2], plan[3]
    seq = [(plan[HEADER + 2 * b], plan[HEADER + 2 * b + 1]) for b in range(B)]
    base = HEADER + 2 * B
    out = {}
    for it in range((len(plan) - base) // 2):
        b, j = plan[base + 2 * it], plan[base + 2 * it + 1]
        if b < 0:
            assert it >= n_items
            continue
        assert it < n_items and 0 <= b < B and j >= 0
        start, q = seq[b]
        assert 0 <= start and q > 0 and start + q <= T and ROWS * j < G * q
        for rho in range(ROWS * j, min(ROWS * (j + 1), G * q)):
            key = (start + rho % q, rho // q)
            assert key not in out, key
            out[key] = it
    return out
