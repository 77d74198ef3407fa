"""Decode attention with a sliding window (fa2_forward_decode_window, fa2_forward_decode_paged_window): the cases, their inputs, the
float64 reference with the window mask, the kernels' key range and split rule in Python integers and a CPU emulation of the data
flow (a helper module, no tests: tests/test_decode_window_reference.py certifies what is here on the CPU,
tests/test_gpu_decode_window.py runs the kernels on it).

THE PROBLEM (include/fa2_mi355x.h).  decode_ref's, under the causal mask, with one more bound: with pos_i = i + len_b - N_q key j
is visible to query i iff pos_i - window_left <= j <= pos_i.  lo_b = max(0, len_b - N_q - window_left) is the lowest key any row
of sequence b sees; the splits share [base_b, len_b), base_b = rounddown(lo_b, 128) (window_range).  A row with pos_i < 0 has no
key: O = 0, L = -inf (L = sink[h] with a sink).

CASES: a record is decode_ref's (_case) plus `wl`; the inputs are made by decode_ref's recipe (seeded uniform bf16, the cache rows
past a length finite garbage eight times as large) and the rows BELOW lo_b are real data like the rest -- the tests that put
garbage there overwrite them.  Every case is one batch whose lengths sit beside each other (lens_of).

EMULATION (emulate): decode_ref.emulate with window_range in place of split_range and a split's partial computed by
split_partial, which is decode_ref._split_partial with the lower bound kmin beside kmax in the two selects (and, like the kernel,
V rows below lo_b zeroed: it never multiplies what lies there).  With kmin = 0 it IS decode_ref._split_partial, bit for bit
(tests/test_decode_window_reference.py asserts it), and the combine and the sink step are decode_ref's own code paths, copied
where they are not functions.

GATES: decode_ref.errors / within_gates, unchanged, and the row gate of O of tests/decode_rows_ref.py (reference64 carries its term)."""
import functools
import itertools

import numpy as np
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows
import regimes

KB, TILE, WAVES = dr.KB, dr.TILE, dr.WAVES
INT_MAX = 2 ** 31 - 1

N_CAP = 1024
HEADS = ((8, 2), (3, 3))
WINDOWS = (0, 1, 31, 127, 128, 200)
SPLITS = (0, 1, 2, 5)
PAGE_SIZES = (32, 96)


def lo_of(n, nq, wl):
    """The lowest key any row of a sequence of n keys sees."""
    return max(0, n - nq - wl)


def lens_of(nq, wl):
    """One batch: no key, one key, fewer keys than queries, the window just not reached / reached / exceeded, lo_b exactly 256
    (a multiple of the key block) and 257, and the full cache."""
    return (0, 1, nq - 1, wl, wl + 1, wl + 2, 256 + nq + wl, 257 + nq + wl, N_CAP)


def _cases():
    out = []
    for n, ((hq, hkv), d, nq, wl) in enumerate(itertools.product(HEADS, (64, 128), (1, 4), WINDOWS)):
        c = dr._case(hq, hkv, d, nq, True, lens_of(nq, wl), N_CAP, sink=n % 3 == 1, splits=SPLITS)
        c["wl"] = wl
        out.append(c)
    return tuple(out)


CASES = _cases()
GPT_OSS = next(i for i, c in enumerate(CASES) if (c["hq"], c["hkv"], c["d"], c["nq"], c["wl"]) == (8, 2, 64, 1, 127))


def case_id(c):
    return f"{c['hq']}-{c['hkv']}-d{c['d']}-q{c['nq']}-w{c['wl']}" + ("-sink" if c["sink"] else "")


IDS = [case_id(c) for c in CASES]


@functools.lru_cache(maxsize=8)
def inputs(i):
    """Host tensors of CASES[i] (made once, never written): decode_ref.inputs' recipe."""
    c = CASES[i]
    B, d, ncap = len(c["lens"]), c["d"], c["ncap"]
    g = torch.Generator().manual_seed(83000 + 31 * i)
    mk = lambda h, n, s: ((torch.rand(B, h, n, d, generator=g) - 0.5) * s).bfloat16()
    Q, K, V = mk(c["hq"], c["nq"], 1.0), mk(c["hkv"], ncap, 8.0), mk(c["hkv"], ncap, 8.0)      # the caches start as garbage
    for b, n in enumerate(c["lens"]):
        K[b, :, :n] /= 8.0
        V[b, :, :n] /= 8.0
    sink = dr.sink_of(c["hq"], 177 + i) if c["sink"] else None
    return Q, K, V, 1.0 / d ** 0.5, torch.tensor(c["lens"], dtype=torch.int32), sink


@functools.lru_cache(maxsize=8)
def inputs_fp8(i):
    """inputs(i) with the caches quantised to e4m3, a distinct descale per head that is no power of two:
    (Q, K8, V8, k_descale, v_descale, scale, lens, sink)."""
    Q, K, V, scale, lens, sink = inputs(i)
    K8, kd = fr.quantise(K, headroom=0.25)
    V8, vd = fr.quantise(V, headroom=0.375)
    kd, vd = kd * 1.0625, vd * 1.1875      # (head 0 too: amax / 448 alone may be a power of two)
    return Q, K8, V8, kd, vd, scale, lens, sink


@functools.lru_cache(maxsize=8)
def dequantised(i):
    _, K8, V8, kd, vd, _, _, _ = inputs_fp8(i)
    return fr.dequantise(K8, kd), fr.dequantise(V8, vd)


def reference64(Q, K, V, lens, scale, sink, wl):
    """float64 O [B, hq, nq, d] and L [B, hq, nq] on contiguous host caches under the causal mask with the window; wl = None: no
    window.  Written out here, not through regimes.ref_attention: that function has no lower bound.  With the row gate's .quad
    (decode_rows_ref.Ref)."""
    B, hq, nq, d = Q.shape
    G = hq // K.shape[1]
    O, L = np.zeros((B, hq, nq, d)), np.zeros((B, hq, nq))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b, n in enumerate(lens):
            n = int(n)
            q = regimes.f64(Q[b])
            k, v = (np.repeat(regimes.f64(t[b, :, :n]), G, axis=0) for t in (K, V))
            s = scale * (q @ np.swapaxes(k, -1, -2))
            pos, j = (np.arange(nq) + n - nq)[:, None], np.arange(n)[None, :]
            vis = j <= pos
            if wl is not None:
                vis &= j >= pos - wl
            s = np.where(vis, s, -np.inf)
            m = s.max(axis=-1, initial=-np.inf)
            seen = np.isfinite(m)
            p = np.exp(s - np.where(seen, m, 0.0)[..., None])
            l = p.sum(axis=-1)
            Lb = np.where(seen, m + np.log(np.where(seen, l, 1.0)), -np.inf)
            Ob = np.where(seen[..., None], (p @ v) / np.where(seen, l, 1.0)[..., None], 0.0)
            if sink is not None:
                sk = np.broadcast_to(sink.double().numpy()[:, None], Lb.shape)
                Ln = np.where(np.isneginf(sk), Lb, np.where(seen, np.logaddexp(Lb, sk), sk))
                Ob = Ob * np.where(np.isneginf(sk), 1.0, np.where(seen, np.exp(Lb - Ln), 0.0))[..., None]
                Lb = Ln
            O[b], L[b] = Ob, Lb
    return rows.Ref(O, L, rows.quad64(Q, K, V, lens, scale, True, sink, wl))


@functools.lru_cache(maxsize=None)
def reference(i, fp8=False):
    """float64 O and L of CASES[i] (fp8: on the dequantised caches)."""
    c = CASES[i]
    Q, K, V, scale, _, sink = inputs(i)
    if fp8:
        K, V = dequantised(i)
    return reference64(Q, K, V, c["lens"], scale, sink, c["wl"])


def window_range(n, nq, wl, n_splits, s):
    """Keys [begin, end) of split s of a sequence of n keys under window wl: the kernel's rule, in Python integers."""
    base = lo_of(n, nq, wl) // KB * KB
    chunk = -(-(-(-(n - base) // n_splits)) // KB) * KB
    return base + s * chunk, min(base + (s + 1) * chunk, n)


def resolved_splits(c, n_splits, ncap=None):
    """What n_splits = 0 stands for with a window: decode_ref's rule on min(capacity, window_left + N_q + 127) keys; the plain
    rule where the window excludes no key of a full cache."""
    if n_splits:
        return n_splits
    ncap = ncap or c["ncap"]
    keys = ncap if c["wl"] is None or c["wl"] >= ncap - 1 else min(ncap, c["wl"] + c["nq"] + KB - 1)
    groups = len(c["lens"]) * c["hkv"]
    return min(-(-256 // groups), max(1, keys // dr.MIN_SPLIT_KEYS), 256)


_f32 = np.float32


def split_partial(q, k, v, kmin, kmax, begin, end, sc):
    """decode_ref._split_partial with keys [kmin, kmax) visible per row: q [hkv, M, d] fp32, k, v [hkv, ncap, d] fp32, kmin, kmax [M]."""
    hkv, M, d = q.shape
    ms, ls, os_ = [], [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for w in range(WAVES):
            m, l, o = np.full((hkv, M), -np.inf, _f32), np.zeros((hkv, M), _f32), np.zeros((hkv, M, d), _f32)
            for kb in range(begin + TILE * w, end, KB):
                ke = min(kb + TILE, end)
                S = (q @ np.swapaxes(k[:, kb:ke], 1, 2)).astype(_f32) * sc
                j = np.arange(kb, ke)[None, :]
                vis = ((j < kmax[:, None]) & (j >= kmin[:, None]))[None]
                mx = np.where(vis, S, -np.inf).max(axis=-1).astype(_f32)
                m_new = np.maximum(m, mx)
                m0 = np.where(np.isneginf(m_new), _f32(0.0), m_new)
                alpha = np.exp2(m - m0, dtype=_f32)
                p = np.where(vis, np.exp2(S - m0[..., None], dtype=_f32), _f32(0.0))
                l = l * alpha + p.sum(axis=-1, dtype=_f32)
                o = o * alpha[..., None] + (dr._bf16(p) @ v[:, kb:ke]).astype(_f32)
                m = m_new
            ms.append(m), ls.append(l), os_.append(o)
        mt = np.maximum.reduce(ms)
        mt0 = np.where(np.isneginf(mt), _f32(0.0), mt)
        lt, acc = np.zeros_like(ls[0]), np.zeros_like(os_[0])
        for m, l, o in zip(ms, ls, os_):
            f = np.exp2(m - mt0, dtype=_f32)
            lt, acc = lt + l * f, acc + o * f[..., None]
        has = lt > 0
        Os = np.where(has[..., None], acc / np.where(has, lt, _f32(1.0))[..., None], _f32(0.0)).astype(_f32)
        Ls = np.where(has, (mt + np.log2(np.where(has, lt, _f32(1.0)), dtype=_f32)) * dr._LN2, -np.inf).astype(_f32)
    return Os, Ls


def emulate(Q, K, V, lens, scale, sink, wl, n_splits):
    """The windowed kernels' data flow on the CPU for an explicit n_splits >= 1: O (bf16 values as fp32) and L fp32.  K and V are
    fp32-representable host tensors (bf16, or dequantised e4m3); rows below lo_b are never multiplied: K's by the select, V's
    because the emulation zeroes them as the kernel does."""
    B, hq, nq, d = Q.shape
    hkv, ncap = K.shape[1], K.shape[2]
    M = hq // hkv * nq
    sc = _f32(scale) * dr._LOG2E
    O, L = np.zeros((B, hq, nq, d), _f32), np.zeros((B, hq, nq), _f32)
    for b in range(B):
        n = min(max(int(lens[b]), 0), ncap)
        lo = lo_of(n, nq, wl)
        q = Q[b].float().numpy().reshape(hkv, M, d)
        k, v = K[b].float().numpy(), V[b].float().numpy().copy()
        v[:, :lo] = 0.0
        pos = np.arange(M) % nq + n - nq
        kmax_all, kmin = pos + 1, np.maximum(pos - wl, 0)
        parts = []
        for s in range(n_splits):
            begin, end = window_range(n, nq, wl, n_splits, s)
            if begin >= end:
                parts.append((np.zeros((hkv, M, d), _f32), np.full((hkv, M), -np.inf, _f32)))
            else:
                parts.append(split_partial(q, k, v, kmin, np.minimum(kmax_all, end), begin, end, sc))
        if n_splits == 1:
            Ob, Lb = parts[0]
        else:      # (decode_ref.emulate's combine)
            with np.errstate(invalid="ignore", divide="ignore"):
                m = np.maximum.reduce([p[1] for p in parts])
                m0 = np.where(np.isneginf(m), _f32(0.0), m)
                tot, acc = np.zeros_like(m), np.zeros((hkv, M, d), _f32)
                for Os, Ls in parts:
                    has = ~np.isneginf(Ls)
                    w = np.where(has, np.exp2((Ls - m0) * dr._LOG2E, dtype=_f32), _f32(0.0))
                    tot, acc = tot + w, acc + w[..., None] * Os
                none = np.isneginf(m)
                Lb = np.where(none, -np.inf, m + np.log2(np.where(none, _f32(1.0), tot), dtype=_f32) * dr._LN2).astype(_f32)
                Ob = np.where(none[..., None], _f32(0.0), acc / np.where(none, _f32(1.0), tot)[..., None]).astype(_f32)
        Ob, Lb = Ob.reshape(hq, nq, d), Lb.reshape(hq, nq)
        if sink is not None:
            Lb, w = dr._sink32(Lb, np.broadcast_to(sink.numpy()[:, None], Lb.shape))
            Ob = Ob * w[..., None]
        O[b], L[b] = dr._bf16(Ob), Lb
    return O, L


# ---- what lies before the window
def below_window(shape, lens, nq, wl):
    """bool [B, H_kv, N_cap, d]: the rows of a contiguous cache below each sequence's lo_b."""
    out = torch.zeros(shape, dtype=torch.bool)
    for b, n in enumerate(lens):
        out[b, :, :lo_of(int(n), nq, wl)] = True
    return out


def pages_below(lens, nq, wl, P):
    """[(b, logical page)] of the pages that lie wholly below lo_b: their table entries are never read."""
    return [(b, p) for b, n in enumerate(lens) for p in range(lo_of(int(n), nq, wl) // P)]


@functools.lru_cache(maxsize=8)
def paged_inputs(i, P, fp8=False):
    """CASES[i] behind pages of P keys (decode_paged_ref.build: permuted pages, NaN where no key was copied, unused entries -1 and
    INT_MAX): (K_pages, V_pages, table, capacity)."""
    c = CASES[i]
    if fp8:
        _, K8, V8 = inputs_fp8(i)[:3]
        Kp, Vp, table, _ = fr.pools(K8, V8, c["lens"], P, 87000 + 17 * i + P)
    else:
        _, K, V = inputs(i)[:3]
        Kp, Vp, table = pr.build(K, V, c["lens"], P, 87000 + 17 * i + P)
    return Kp, Vp, table, table.shape[1] * P
