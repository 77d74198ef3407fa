"""Cases and mutants for the row gates of attention sinks and of a gradient for L (a helper module, no tests:
tests/test_sink_rows_reference.py certifies what is here on the CPU, tests/test_gpu_sink_rows.py runs the kernels on it).
Everything numeric is bf16_rows_ref.Case with its optional `sink` and `dL`; this module only says WHICH
problems run and what a specific fault would write.

SINKS.  Eight per (8, 2) problem, one per query head: -inf (no sink), -30 (a sink that vanishes), log N_k - 1, log N_k,
log N_k + 1, log N_k + 3 (the head keeps about 0.05 of a plain head's |O|), log N_k + 6 and log N_k + 20 (about 2e-9 of it).
Three per (3, 3) problem: -inf, log N_k + 3 and log N_k + 20 -- no sink beside the two heads a tensor norm cannot see.  `spikes`
and `lift` put a sink of 26 on the spiked heads, as tests/test_gpu_sink.py does.
dL.  Normal noise times the standard deviation of D = rowsum(dO o bf16(O_ref)) over the problem, and 100 x that (the row
constant D' = D - dL is then dL to two digits), on `scale-one`, with the eight sinks and without any.

THE MUTANTS (k1 .. k7), each what one fault would write, built from the emulation like m1 .. m10 of bf16_rows_ref:
  (k1) the sink factor f applied twice on the second row block of a causal pair (the plain causal launch gives a workgroup row
       blocks nrb - 1 - i and i; the second is i);  (k2) every row of the log N_k + 20 head has O = 0;  (k3) the log N_k + 3
  head's O is x 1.05;  (k4) one 32-row group's mask shifted by one key in the backward of a sinked head;  (k5) one row takes its
  neighbour's dL;  (k6) dL ignored on one 32-row group;  (k7) dL multiplied in, not selected, on an L = -inf row holding Inf:
  0 x Inf = NaN in that row's dS, which reaches dQ of the row and dK of every key block the row's tile meets."""
import functools
import math

import numpy as np
import torch

import bf16_rows_ref as B
import lse_ref as LR
import regimes as R

HEADS = ((8, 2), (3, 3))
SINK_SHAPES = ((300, 300), (600, 600), (1024, 1024), (1025, 1025), (257, 64), (300, 1100), (1100, 300))
SINK_REGIMES = ("scale-one", "peaked")
SPIKED_SHAPES, SPIKED_REGIMES, SPIKE_SINK = ((1100, 1100), (300, 1100)), ("spikes", "lift"), 26.0
DL_SHAPES = (((300, 300), B.MASKS), ((1024, 1024), B.MASKS), ((70, 300), B.MASKS), ((300, 70), (True,)))
DL_SCALES, DL_REGIME = (1.0, 100.0), "scale-one"
PACKED, PACKED_REGIME = R.PACKED_TWO, "scale-one"
OFFSETS8 = (None, -30.0, -1.0, 0.0, 1.0, 3.0, 6.0, 20.0)       # None: -inf; a number x: log N_k + x, but -30 itself
PLUS3, PLUS20 = {8: 5, 3: 1}, {8: 7, 3: 2}                     # the heads with log N_k + 3 and log N_k + 20


def sinks(regime, hq, nq, nk):
    """fp32 [hq]: the module's sinks for a problem."""
    base = math.log(max(nk, 1))
    vals = [-math.inf, -30.0] + [base + x for x in OFFSETS8[2:]]
    if hq == 3:
        vals = [vals[0], vals[5], vals[7]]
    assert len(vals) == hq
    sink = torch.tensor(vals, dtype=torch.float32)
    if regime in R.SPIKED:
        for h in sorted({h for h, *_ in R.spike_rows(nq, nk, hq, False)}):
            sink[h] = SPIKE_SINK
    return sink


def _dl(regime, Q, K, V, dO, s, shift, sink, scale, seed):
    O, _ = LR.forward(Q, K, V, s, shift, sink)
    size = float((B.f64(dO) * B._bf16(O)).sum(axis=-1).std())
    noise = torch.randn(Q.shape[:2], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (noise * (size * scale)).float()


def _one(regime, hq, hkv, nq, nk, d, causal, with_sink, dl_scale):
    Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
    sink = sinks(regime, hq, nq, nk) if with_sink else None
    dL = None
    if dl_scale:                                              # (a packed sequence without rows or keys: D = 0, and so is its dL)
        dL = _dl(regime, Q, K, V, dO, s, nk - nq if causal else None, sink, dl_scale, R.seed_of(regime, nq, nk, d) + 5) if nq and nk else torch.zeros(hq, nq)
    return B.Case(regime, Q, K, V, dO, s, causal, sink, dL)


@functools.lru_cache(maxsize=6)
@B.one_thread
def case(regime, hq, hkv, nq, nk, d, causal, with_sink=True, dl_scale=0.0):
    return _one(regime, hq, hkv, nq, nk, d, causal, with_sink, dl_scale)


@functools.lru_cache(maxsize=2)
@B.one_thread
def packed(d, causal):
    """The two-sided packed batch of regimes.PACKED_TWO with the eight sinks and a dL of the size of D."""
    hq, hkv = R.HEADS_GQA
    sink = sinks(PACKED_REGIME, hq, 0, max(nk for _, nk in PACKED))      # one sink per head for the whole batch: the longest sequence's
    parts = []
    for nq, nk in PACKED:
        Q, K, V, dO, s = R.sequence(PACKED_REGIME, hq, hkv, nq, nk, d)
        dL = _dl(PACKED_REGIME, Q, K, V, dO, s, nk - nq if causal else None, sink, 1.0, R.seed_of(PACKED_REGIME, nq, nk, d) + 5) if nq and nk else torch.zeros(hq, nq)
        parts.append(B.Case(PACKED_REGIME, Q, K, V, dO, s, causal, sink, dL))
    return B.Packed(parts)


def cpu_cases():
    """Every (label, builder, arguments) tests/test_gpu_sink_rows.py hands a kernel."""
    out = []
    for d in B.HEAD_DIMS:
        for causal in B.MASKS:
            for hq, hkv in HEADS:
                out += [(f"sink {r} H{hq}/{hkv} {nq}x{nk}", case, (r, hq, hkv, nq, nk, d, causal)) for r in SINK_REGIMES for nq, nk in SINK_SHAPES]
            out += [(f"sink {r} H8/2 {nq}x{nk}", case, (r,) + R.HEADS_GQA + (nq, nk, d, causal)) for r in SPIKED_REGIMES for nq, nk in SPIKED_SHAPES]
            for (nq, nk), masks in DL_SHAPES:
                if causal in masks:
                    out += [(f"dL x{sc:g} {'sinks' if ws else 'plain'} {nq}x{nk}", case, (DL_REGIME,) + R.HEADS_GQA + (nq, nk, d, causal, ws, sc))
                            for sc in DL_SCALES for ws in (False, True)]
            out.append(("packed sinks dL", packed, (d, causal)))
    mask = lambda build, args: args[1] if build is packed else args[6]
    dim = lambda build, args: args[0] if build is packed else args[5]
    return [(f"{label} d{dim(build, args)} {'causal' if mask(build, args) else 'full'}", build, args) for label, build, args in out]


def runs_partials(c):
    """Whether phases 7 and 8 | 1 of this case sum bf16 per-head partials (grouped heads on the single kernel)."""
    return c.G > 1 and not isinstance(c, B.Packed) and c.nq == c.nk and B.single_kernel(c.nq, c.d)


# ------------------------------------------------------------------------------------------------ the suite's tensor gates
def tensor_gates(got, c):
    """What tests/test_gpu_sink.py and part 1 of tests/test_gpu_lse.py would say of `got` ({tensor: array}, any subset): rel-L2 <=
    5e-3 per tensor, max |dL| <= 1e-4 over the finite rows (1e-3 where |L_ref| > 25), every value finite, O and dQ exactly 0 on
    the rows without a key.  -> ({tensor: figure}, passes)."""
    figs, ok = {}, True
    for n, x in got.items():
        x = B.f64(x)
        if n == "L":
            fin = np.isfinite(c.ref["L"])
            with np.errstate(invalid="ignore"):
                e = np.abs(x - c.ref["L"])[fin]
            near = np.abs(c.ref["L"][fin]) <= B.L_NEAR
            figs[n] = float(e.max(initial=0.0))
            ok = ok and bool((e[near] <= B.L_ABS).all() and (e[~near] <= B.L_ABS_FAR).all()) and np.array_equal(np.isneginf(x), np.isneginf(c.ref["L"]))
            continue
        figs[n] = R.rel(x, c.ref[n]) if np.isfinite(x).all() else math.inf
        ok = ok and figs[n] <= B.BF16_REL
        if n in ("O", "dQ"):
            ok = ok and bool((x[c.keyless] == 0).all())
    return figs, ok


# ------------------------------------------------------------------------------------------------ the mutants
def _sunk_rows(c, offset, head, rows, times):
    out = c.emulate_forward(offset)
    new = B.forward_flow(c.scores()[head, rows], c.v[head // c.G], offset, sink=B.f64(c.sink)[head], sink_times=times)
    for n in out:
        out[n][head, rows] = new[n]
    return out


def k1_sink_factor_twice(c, offset, head):
    """(k1) -> (outputs, rows): f applied twice to O on the second row block of the first causal pair (row block 0)."""
    assert c.causal and c.nq > 256 and np.isfinite(float(c.sink[head]))
    rows = slice(0, 256)
    out = _sunk_rows(c, offset, head, rows, 2)
    out["L"] = c.emulate_forward(offset)["L"]                 # L' is stored once: it is O's scale that is applied again
    return out, rows


def k2_head_is_zero(c, offset):
    head = PLUS20[c.hq]
    out = c.emulate_forward(offset)
    out["O"][head] = 0.0
    return out, head


def k3_head_is_scaled(c, offset, factor=1.05):
    head = PLUS3[c.hq]
    out = c.emulate_forward(offset)
    out["O"][head] = B._bf16(out["O"][head] * factor)
    return out, head


def k4_mask_shifted_backward(c, head, group):
    assert c.dL is None and np.isfinite(float(c.sink[head]))
    return B.m3_mask_shifted_backward(c, head, group)


@B.one_thread
def _backward_with_dl(c, dL):
    return {n: B._bf16(x) for n, x in zip(B.GRADS, LR.flow(*c.t, dL, c.s, c.shift, c.O16, c.L32, c.sink, kernel_formats=True))}


def k5_neighbours_dl(c, head, row):
    dL = c.dL.clone()
    dL[head, row] = c.dL[head, row + 1]
    return _backward_with_dl(c, dL)


def k6_dl_ignored(c, head, group):
    dL = c.dL.clone()
    dL[head, 32 * group:32 * group + 32] = 0.0
    return _backward_with_dl(c, dL)


def k7_dl_multiplied_in(c, head, row):
    """(k7) the row has L = -inf and dL = Inf: P = 0 times Inf is NaN in every dS of the row -- dQ of the row and dK of the head's
    K/V head over the keys of the row's tiles (here: all of them, the problem is shorter than a key block)."""
    assert np.isneginf(c.ref["L"][head, row])
    out = c.emulate_backward()
    out["dQ"][head, row] = np.nan
    out["dK"][head // c.G] = np.nan
    return out
