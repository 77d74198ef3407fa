"""What the row gate of tests/decode_rows_ref.py is certified on and what tests/test_gpu_decode_rows.py runs (a helper module, no
tests): the regime runs on every body of the family, the CPU emulation of any call of the family, the subset of the extend and
ragged cases the certificate takes, and the mutants that pin the gap the tensor gate left.

THE REGIME RUNS.  `peaked`, `spikes`, `scale-one` and `low-level` of tests/regimes.py, through regimes.sequence as
decode_ref.inputs uses it, on the smallest shape that reaches each body, 8 query heads on 2, causal, at d = 64 and 128:
    decode   N_q = 4                       lengths (300, 1100)
    extend   N_q = 17: M = 68 rows, a spiked head (1 and 7) in each of the two row tiles of the first block and a second block
    ragged   q_b = (17, 1, 4)              lengths (1100, 300, 1100)
in caches of 1120 rows (35 pages of 32; the rows past a length hold finite garbage), over bf16 and e4m3 caches
(decode_fp8kv_ref.quantise with a descale that is no power of two, as extend_ref.inputs_fp8), contiguous and behind pages of 32,
no window and window_left 127 and 200, 1, 7 and 0 splits; the sink alternates over (cache kind, window) except under `low-level`
(a sink of 1 .. 7 beside keys at -115 leaves O below bf16's normal range: decode_ref.CASES keeps that regime without one too).
The spike keys fall where they fall: at 300 keys under window 200 the 28-unit key (84) lies in a tile wholly below lo; at 1100
keys the 28-unit key (308) is hidden by either window and the 130-unit one (902) is visible.

THE MUTANTS, built from the emulation on the bf16 inputs:
    m1  the second product of the longest sequence misses its last full 32-key tile (V's rows zeroed: L untouched)
    m2  O of the longest sequence x 1.02
    m3  two query rows of the longest sequence exchanged
    m4  for a G > 1 extend shape, two heads' rows of the longest sequence exchanged
    m5  O of the longest sequence taken with the next K/V head's V (a wrong head stride on the V side alone)."""
import functools

import numpy as np
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows
import decode_window_ref as wr
import extend_ragged_ref as rr
import extend_ref as er
import regimes

BODIES = ("decode", "extend", "ragged")
REGIMES = ("peaked", "spikes", "scale-one", "low-level")
HEAD_DIMS = (64, 128)
HQ, HKV = 8, 2
N_CAP, PAGE = 1120, 32
NQ = {"decode": 4, "extend": 17}
LENS = (300, 1100)
RAGGED_QS, RAGGED_LENS = (17, 1, 4), (1100, 300, 1100)
KINDS = ("bf16", "e4m3")
WINDOWS = (None, 127, 200)
SPLITS = (1, 7, 0)
RUNS = tuple((body, d, regime) for body in BODIES for d in HEAD_DIMS for regime in REGIMES)
RUN_IDS = [f"{body}-d{d}-{regime}" for body, d, regime in RUNS]


def has_sink(regime, kind, wi):
    return regime != "low-level" and (KINDS.index(kind) + wi) % 2 == 1


def shape_of(body):
    """(q_b per sequence, len_b per sequence)."""
    return (RAGGED_QS, RAGGED_LENS) if body == "ragged" else ((NQ[body],) * len(LENS), LENS)


@functools.lru_cache(maxsize=4)
def inputs(body, d, regime):
    """Host tensors (made once, never written): Q ([B, hq, nq, d]; ragged: [T, hq, d]), bf16 K, V [B, hkv, N_CAP, d], the scale,
    the lengths int32, the sink fp32 [hq], cu int32 [B + 1] (ragged, else None)."""
    qs, lens = shape_of(body)
    B = len(lens)
    g = torch.Generator().manual_seed(104000 + 97 * BODIES.index(body) + 13 * REGIMES.index(regime) + d)
    K, V = (((torch.rand(B, HKV, N_CAP, d, generator=g) - 0.5) * 8.0).bfloat16() for _ in range(2))      # the caches start as garbage
    Qs = []
    for b, (nq, n) in enumerate(zip(qs, lens)):
        q, k, v, _, scale = regimes.sequence(regime, HQ, HKV, nq, n, d)
        Qs.append(q)
        K[b, :, :n], V[b, :, :n] = k, v
    Q = torch.cat([q.transpose(0, 1) for q in Qs]).contiguous() if body == "ragged" else torch.stack(Qs)
    cu = torch.tensor(rr.cu_of(qs), dtype=torch.int32) if body == "ragged" else None
    return Q, K, V, float(scale), torch.tensor(lens, dtype=torch.int32), dr.sink_of(HQ, 411 + d), cu


@functools.lru_cache(maxsize=4)
def inputs_fp8(body, d, regime):
    """(K8, V8, k_descale, v_descale) of inputs(...): one descale per head, no power of two (extend_ref.inputs_fp8's)."""
    _, K, V = inputs(body, d, regime)[:3]
    K8, kd = fr.quantise(K, headroom=0.25)
    V8, vd = fr.quantise(V, headroom=0.375)
    return K8, V8, kd * 1.0625, vd * 1.1875


@functools.lru_cache(maxsize=4)
def caches(body, d, regime, kind):
    """The values the caches hold, as the reference and the emulation read them (e4m3: dequantised fp32)."""
    if kind == "bf16":
        return inputs(body, d, regime)[1:3]
    K8, V8, kd, vd = inputs_fp8(body, d, regime)
    return fr.dequantise(K8, kd), fr.dequantise(V8, vd)


@functools.lru_cache(maxsize=4)
def paged_inputs(body, d, regime, kind):
    """(K_pages, V_pages, table) behind pages of PAGE keys (decode_paged_ref.build: permuted pages, NaN where no key was copied)."""
    _, lens = shape_of(body)
    seed = 105000 + 97 * BODIES.index(body) + 13 * REGIMES.index(regime) + d
    if kind == "e4m3":
        K8, V8 = inputs_fp8(body, d, regime)[:2]
        return fr.pools(K8, V8, lens, PAGE, seed)[:3]
    return pr.build(*inputs(body, d, regime)[1:3], lens, PAGE, seed)


@functools.lru_cache(maxsize=16)
def reference(body, d, regime, kind, wi):
    """The float64 reference (a decode_rows_ref.Ref) under WINDOWS[wi] on the `kind` caches."""
    Q, _, _, scale, lens, sink, _ = inputs(body, d, regime)
    K, V = caches(body, d, regime, kind)
    sink = sink if has_sink(regime, kind, wi) else None
    if body == "ragged":
        return rr.reference64(Q, K, V, RAGGED_QS, lens.tolist(), scale, True, sink, WINDOWS[wi])
    return er.reference64(Q, K, V, lens.tolist(), scale, True, sink, WINDOWS[wi])


# ------------------------------------------------------------------------------------------------ the emulation of any call
def emulate(Q, K, V, lens, scale, causal, sink, wl, n_splits):
    """decode_ref.emulate without a window, decode_window_ref.emulate with one: neither has a row limit, so they serve extend too."""
    if wl is None:
        return dr.emulate(Q, K, V, lens, scale, causal, sink, n_splits)
    assert causal
    return wr.emulate(Q, K, V, lens, scale, sink, wl, n_splits)


def emulate_ragged(Q, K, V, qs, lens, scale, causal, sink, wl, n_splits):
    """emulate per sequence on the transposed slice [1, hq, q_b, d]: token-major O [T, hq, d] and L [T, hq]."""
    T, hq, d = Q.shape
    O, L = np.full((T, hq, d), np.nan, np.float32), np.full((T, hq), np.nan, np.float32)
    t = 0
    for b, q in enumerate(qs):
        if q:
            Ob, Lb = emulate(Q[t:t + q].transpose(0, 1)[None], K[b:b + 1], V[b:b + 1], [int(lens[b])], scale, causal, sink, wl, n_splits)
            O[t:t + q], L[t:t + q] = np.swapaxes(Ob[0], 0, 1), np.swapaxes(Lb[0], 0, 1)
        t += q
    return O, L


def emulate_run(body, d, regime, kind, wi, n_splits):
    Q, _, _, scale, lens, sink, _ = inputs(body, d, regime)
    K, V = caches(body, d, regime, kind)
    sink = sink if has_sink(regime, kind, wi) else None
    if body == "ragged":
        return emulate_ragged(Q, K, V, RAGGED_QS, lens.tolist(), scale, True, sink, WINDOWS[wi], n_splits)
    return emulate(Q, K, V, lens.tolist(), scale, True, sink, WINDOWS[wi], n_splits)


# ------------------------------------------------------------------------------------------------ the certificate's subset
CERT_VARIANTS = (0, 1, 4, 7)      # extend_ref.VARIANTS: causal, full, w31, w200
CERT_SPLITS = (1, 7)


def cert_subset(n_cases):
    """[(case, variant, fp8)]: every case twice -- once on bf16 and once on e4m3 caches, under two of the four variants, rotating
    so that every variant meets both cache kinds and both head dims (the cases alternate d = 64, 128)."""
    out = []
    for i in range(n_cases):
        out += [(i, CERT_VARIANTS[(i // 2) % 4], False), (i, CERT_VARIANTS[(i // 2 + 1 + i % 2) % 4], True)]
    return out


# ------------------------------------------------------------------------------------------------ the mutants
def longest(lens):
    return int(np.argmax(lens))


def last_full_tile(n):
    """The first key of the last full 32-key tile of a sequence of n keys."""
    return (n // dr.TILE - 1) * dr.TILE


def m1_last_tile_missing_from_pv(Q, K, V, lens, scale, causal, sink, wl, n_splits):
    """(m1) -> (O, L, b): the emulation with V's rows of the longest sequence's last full tile zeroed -- K is whole, so L is untouched."""
    b = longest(lens)
    V = V.clone()
    t0 = last_full_tile(int(lens[b]))
    V[b, :, t0:t0 + dr.TILE] = 0.0
    return emulate(Q, K, V, lens, scale, causal, sink, wl, n_splits) + (b,)


def m2_scaled(O, lens, factor=1.02):
    """(m2) -> (O, b): O of the longest sequence x factor, rounded to bf16 again."""
    b = longest(lens)
    O = O.copy()
    O[b] = dr._bf16(O[b] * np.float32(factor))
    return O, b


def m3_rows_exchanged(O, lens, i, j):
    """(m3) -> (O, b): query rows i and j of the longest sequence exchanged, in every head."""
    b = longest(lens)
    O = O.copy()
    O[b][:, [i, j]] = O[b][:, [j, i]]
    return O, b


def m4_heads_exchanged(O, lens, g, h):
    """(m4) -> (O, b): the rows of heads g and h of the longest sequence exchanged."""
    b = longest(lens)
    O = O.copy()
    O[b][[g, h]] = O[b][[h, g]]
    return O, b


def m5_next_heads_v(Q, K, V, lens, scale, causal, sink, wl, n_splits):
    """(m5) -> (O, L, b): the longest sequence's second product reads the K/V heads' V rotated by one; L untouched."""
    b = longest(lens)
    V = V.clone()
    V[b] = torch.roll(V[b], 1, dims=0)
    return emulate(Q, K, V, lens, scale, causal, sink, wl, n_splits) + (b,)
