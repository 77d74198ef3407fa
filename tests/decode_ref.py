"""Decode attention over a KV cache with per-sequence lengths (fa2_forward_decode): the cases, their inputs, the float64 reference
and a CPU emulation of the kernels' data flow (a helper module, no tests: tests/test_decode_reference.py certifies what is here
on the CPU, tests/test_gpu_decode.py runs the kernels on it).

THE PROBLEM (include/fa2_mi355x.h).  Q [B, H_q, N_q, d] against caches [B, H_kv, N_cap, d]; sequence b attends keys [0, len_b) of
its cache rows; the N_q queries are its last tokens: under the causal mask key j is visible to query i iff j <= i + len_b - N_q.
A row without a visible key has O = 0 and L = -inf (L = sink[h] with a sink).

REFERENCE.  Per sequence, regimes.ref_attention (sink_ref.ref_attention_sink with a sink) on K[b, :, :len_b] and V[b, :, :len_b]
repeated per group, in float64 on the bf16 inputs; the rules for rows without a key are those functions'.

EMULATION (emulate): what the kernels do to the numbers, in NumPy fp32 -- a split's keys go to four waves in 32-key tiles taken
round-robin; per tile fp32 scores in log2 units, the running maximum, P = exp2(S - m) with masked entries selected to 0, the row
sum from the fp32 P, P rounded to bf16 for the second product, fp32 accumulation; the waves meet at their common maximum; a split
leaves a normalised fp32 O_s and L_s; the combine folds them in ascending order in fp32, applies the sink and rounds to bf16 once.
It follows the kernels' order of operations, not their bits (a NumPy fp32 product sums in another order than an MFMA).

GATES: the project's bf16 ones (tests/test_gpu_qk.py): O rel-L2 <= 5e-3 over the whole tensor; max |dL| <= 1e-4 over rows with a
finite reference L of magnitude <= 25, <= 1e-3 above; the rows with L = -inf are exactly the reference's and O is exactly 0 there.
The tensor gate alone lets a fault on the long sequences' P V side pass (they hold 0.1 % of the norm): O is also gated PER ROW by
tests/decode_rows_ref.py, whose quadrature term reference() carries beside (O, L)."""
import functools
import itertools

import numpy as np
import torch

import decode_rows_ref as rows
import regimes
from sink_ref import ref_attention_sink

KB = 128              # kDecodeKB: a split's first key is a multiple of it (one round of the four waves)
TILE = 32             # kDecodeTile: keys of one MFMA tile, a wave's step
WAVES = KB // TILE
MAX_ROWS = 32         # kDecodeMaxRows: (H_q / H_kv) N_q
BF16_REL = 5e-3
L_ABS, L_ABS_LARGE, L_LARGE = 1e-4, 1e-3, 25.0

SPLITS = (0, 1, 2, 7, 64)
N_CAP = 2560
LENS = (0, 1, 2, KB - 1, KB, KB + 1, 300, 1100, 2500)                       # one batch: every length beside the others
LENS_TILE = (2500, TILE + 1, 0, TILE - 1, 3, TILE, 2 * KB + TILE + 1, 1100, 2 * KB)      # the wave tile's edges, the longest first
HEADS = ((3, 3), (8, 2), (8, 1))


def _case(hq, hkv, d, nq, causal, lens, ncap, sink, regime=None, splits=SPLITS, seqlens=True):
    return dict(hq=hq, hkv=hkv, d=d, nq=nq, causal=causal, lens=tuple(lens), ncap=ncap, sink=sink, regime=regime, splits=tuple(splits),
                seqlens=seqlens)


def _cases():
    out = []
    for n, ((hq, hkv), d, nq, causal) in enumerate(itertools.product(HEADS, (64, 128), (1, 4), (True, False))):
        lens = LENS if n % 2 == 0 else LENS_TILE
        out.append(_case(hq, hkv, d, nq, causal, lens, N_CAP if n % 4 < 2 else max(lens), sink=n % 3 == 1))
    for d in (64, 128):                                       # M = 32 from the heads alone
        out.append(_case(32, 1, d, 1, True, LENS, N_CAP, sink=d == 64))
    for nq, causal in ((1, True), (4, True), (4, False)):     # seqlens_k = None: every sequence has N_cap keys
        for ncap in (3, KB + 1, 300):                         # (3 < N_q = 4 under the mask: a row without a key)
            out.append(_case(8, 2, 128 if ncap != 300 else 64, nq, causal, (ncap, ncap), ncap, sink=ncap == 3, seqlens=False))
    for regime, d in itertools.product(("peaked", "spikes", "scale-one", "low-level"), (64, 128)):
        out.append(_case(8, 2, d, 4, True, (300, 1100), 1100, sink=regime != "low-level" and d == 128, regime=regime, splits=(0, 1, 7)))
    return tuple(out)


CASES = _cases()


def case_id(c):
    return (f"{c['hq']}-{c['hkv']}-d{c['d']}-q{c['nq']}-{'causal' if c['causal'] else 'full'}-cap{c['ncap']}-len{c['lens'][0]}"
            + ("-sink" if c["sink"] else "") + ("" if c["seqlens"] else "-nolens") + (f"-{c['regime']}" if c["regime"] else ""))


def sink_of(hq, seed):
    """Finite logits about the size of a row's L, two heads without a sink."""
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(hq, generator=g) * 6.0 + 1.0).float()
    s[0] = -np.inf
    s[hq // 2] = -np.inf
    return s


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Host tensors of CASES[i] (made once, never written): bf16 Q [B, hq, nq, d], K and V caches [B, hkv, ncap, d] whose rows past
    a sequence's length hold finite garbage, the softmax scale, int32 lengths, the fp32 sink or None."""
    c = CASES[i]
    B, d, ncap = len(c["lens"]), c["d"], c["ncap"]
    g = torch.Generator().manual_seed(52000 + 31 * i)
    mk = lambda h, n, s: ((torch.rand(B, h, n, d, generator=g) - 0.5) * s).bfloat16()
    Q, K, V = mk(c["hq"], c["nq"], 1.0), mk(c["hkv"], ncap, 8.0), mk(c["hkv"], ncap, 8.0)      # the caches start as garbage
    scale = 1.0 / d ** 0.5
    for b, n in enumerate(c["lens"]):
        if c["regime"]:
            q, k, v, _, scale = regimes.sequence(c["regime"], c["hq"], c["hkv"], c["nq"], n, d)
            Q[b], K[b, :, :n], V[b, :, :n] = q, k, v
        else:
            K[b, :, :n] /= 8.0
            V[b, :, :n] /= 8.0
    sink = sink_of(c["hq"], 77 + i) if c["sink"] else None
    return Q, K, V, float(scale), torch.tensor(c["lens"], dtype=torch.int32), sink


@functools.lru_cache(maxsize=None)
def reference(i):
    """float64 O [B, hq, nq, d] and L [B, hq, nq] of CASES[i], with the row gate's .quad beside them (decode_rows_ref.Ref)."""
    c = CASES[i]
    Q, K, V, scale, lens, sink = inputs(i)
    G = c["hq"] // c["hkv"]
    O, L = np.zeros(tuple(Q.shape)), np.zeros(tuple(Q.shape[:3]))
    for b, n in enumerate(c["lens"]):
        q = regimes.f64(Q[b])
        k, v = (np.repeat(regimes.f64(t[b, :, :n]), G, axis=0) for t in (K, V))
        if sink is None:
            O[b], L[b] = regimes.ref_attention(q, k, v, np.zeros_like(q), scale, c["causal"])[:2]
        else:
            O[b], L[b] = ref_attention_sink(q, k, v, np.zeros_like(q), scale, c["causal"], sink.double().numpy())[:2]
    return rows.Ref(O, L, rows.quad64(Q, K, V, c["lens"], scale, c["causal"], sink))


def split_range(n, n_splits, s):
    """Keys [begin, end) of split s of a sequence of n keys: the kernel's rule."""
    chunk = -(-(-(-n // n_splits)) // KB) * KB
    return s * chunk, min((s + 1) * chunk, n)


_f32 = np.float32
_LOG2E, _LN2 = _f32(1.4426950408889634), _f32(0.6931471805599453)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def _sink32(L, sink_rows):
    """(L', w) of the kernels' sink step in fp32: L' = logaddexp(L, s), w = exp(L - L'); s = -inf: nothing changes; L = -inf: L' = s, w = 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        none, keyless = np.isneginf(sink_rows), np.isneginf(L)
        e = np.exp2(-np.abs(L - sink_rows) * _LOG2E, dtype=_f32)
        Ln = np.maximum(L, sink_rows) + np.log2(_f32(1.0) + e, dtype=_f32) * _LN2
        w = np.exp2((L - Ln) * _LOG2E, dtype=_f32)
    return (np.where(none, L, np.where(keyless, sink_rows, Ln)).astype(_f32),
            np.where(none, _f32(1.0), np.where(keyless, _f32(0.0), w)).astype(_f32))


def _split_partial(q, k, v, kmax, begin, end, sc):
    """One split's normalised fp32 O_s [hkv, M, d] and L_s [hkv, M]: q [hkv, M, d] fp32, k, v [hkv, ncap, d] fp32, kmax [M]."""
    hkv, M, d = q.shape
    ms, ls, os_ = [], [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for w in range(WAVES):
            m, l, o = np.full((hkv, M), -np.inf, _f32), np.zeros((hkv, M), _f32), np.zeros((hkv, M, d), _f32)
            for kb in range(begin + TILE * w, end, KB):
                ke = min(kb + TILE, end)
                S = (q @ np.swapaxes(k[:, kb:ke], 1, 2)).astype(_f32) * sc
                vis = (np.arange(kb, ke)[None, :] < kmax[:, None])[None]
                mx = np.where(vis, S, -np.inf).max(axis=-1).astype(_f32)
                m_new = np.maximum(m, mx)
                m0 = np.where(np.isneginf(m_new), _f32(0.0), m_new)
                alpha = np.exp2(m - m0, dtype=_f32)
                p = np.where(vis, np.exp2(S - m0[..., None], dtype=_f32), _f32(0.0))
                l = l * alpha + p.sum(axis=-1, dtype=_f32)
                o = o * alpha[..., None] + (_bf16(p) @ v[:, kb:ke]).astype(_f32)
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
        Ls = np.where(has, (mt + np.log2(np.where(has, lt, _f32(1.0)), dtype=_f32)) * _LN2, -np.inf).astype(_f32)
    return Os, Ls


def emulate(Q, K, V, lens, scale, causal, sink, n_splits):
    """The kernels' data flow on the CPU: O (bf16 values as fp32) [B, hq, nq, d] and L fp32 [B, hq, nq] for an explicit n_splits >= 1."""
    B, hq, nq, d = Q.shape
    hkv, ncap = K.shape[1], K.shape[2]
    G = hq // hkv
    M = G * nq
    sc = _f32(scale) * _LOG2E
    O, L = np.zeros((B, hq, nq, d), _f32), np.zeros((B, hq, nq), _f32)
    for b in range(B):
        n = min(max(int(lens[b]), 0), ncap)
        q = Q[b].float().numpy().reshape(hkv, M, d)              # row m of a K/V head: query head m // nq of its group, query m % nq
        k, v = K[b].float().numpy(), V[b].float().numpy()
        kmax_all = (np.arange(M) % nq + n - nq + 1) if causal else np.full(M, n)
        parts = []
        for s in range(n_splits):
            begin, end = split_range(n, n_splits, s)
            if begin >= end:
                parts.append((np.zeros((hkv, M, d), _f32), np.full((hkv, M), -np.inf, _f32)))
            else:
                parts.append(_split_partial(q, k, v, np.minimum(kmax_all, end), begin, end, sc))
        if n_splits == 1:
            Ob, Lb = parts[0]
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                m = np.maximum.reduce([p[1] for p in parts])
                m0 = np.where(np.isneginf(m), _f32(0.0), m)
                tot, acc = np.zeros_like(m), np.zeros((hkv, M, d), _f32)
                for Os, Ls in parts:
                    has = ~np.isneginf(Ls)
                    w = np.where(has, np.exp2((Ls - m0) * _LOG2E, dtype=_f32), _f32(0.0))
                    tot, acc = tot + w, acc + w[..., None] * Os
                none = np.isneginf(m)
                Lb = np.where(none, -np.inf, m + np.log2(np.where(none, _f32(1.0), tot), dtype=_f32) * _LN2).astype(_f32)
                Ob = np.where(none[..., None], _f32(0.0), acc / np.where(none, _f32(1.0), tot)[..., None]).astype(_f32)
        Ob, Lb = Ob.reshape(hq, nq, d), Lb.reshape(hq, nq)
        if sink is not None:
            Lb, w = _sink32(Lb, np.broadcast_to(sink.numpy()[:, None], Lb.shape))
            Ob = Ob * w[..., None]
        O[b], L[b] = _bf16(Ob), Lb
    return O, L


def resolved_splits(c, n_splits):
    """What n_splits = 0 stands for: the smallest s with B H_kv s >= 256 that leaves a split of a full cache MIN_SPLIT_KEYS keys."""
    if n_splits:
        return n_splits
    groups = len(c["lens"]) * c["hkv"]
    return min(-(-256 // groups), max(1, c["ncap"] // MIN_SPLIT_KEYS), 256)


MIN_SPLIT_KEYS = 256      # kDecodeMinSplitKeys


def errors(O, L, ref):
    """(O rel-L2, max |dL| where |L_ref| <= 25, max |dL| above, whether the -inf rows are the reference's and O is 0 on them)."""
    rO, rL = ref[:2]
    O, L = np.asarray(O, dtype=np.float64), np.asarray(L, dtype=np.float64)
    none = np.isneginf(rL)
    same = bool(np.array_equal(np.isneginf(L), none) and np.isfinite(L[~none]).all() and np.isfinite(O).all() and (O[none] == 0).all())
    small = ~none & (np.abs(rL) <= L_LARGE)
    dl = np.abs(np.where(none, 0.0, L) - np.where(none, 0.0, rL))
    return (regimes.rel(O, rO), float(dl[small].max(initial=0.0)), float(dl[~none & ~small].max(initial=0.0)), same)


def within_gates(e):
    return e[0] <= BF16_REL and e[1] <= L_ABS and e[2] <= L_ABS_LARGE and e[3]
