"""GPU: attention sinks and a gradient for L, row by row.

tests/test_gpu_sink.py and part 1 of tests/test_gpu_lse.py judge O, dQ, dK and dV by one rel-L2 per tensor.  A head whose sink is
log N_k + 3 holds 0.05 of a plain head's |O|, one with log N_k + 20 about 2e-9 of it: whatever happens to their rows is rounding
noise in that norm (tests/test_sink_rows_reference.py: a head of zeros, a head scaled by 1.05 and a shifted mask in a sinked head's
backward all pass it).  Here every row has the gate of bf16_rows_ref.Case with its `sink` and `dL` -- P = exp(S - L) with the
sink-inclusive L, D' = D - dL, e_ij with phi P_ij |dL_i| -- certified on the CPU for every case below; the Dense driver, the
checker, the order of the checks and the report line are tests/test_gpu_bf16_rows.py's.  The forward is judged against
lse_ref.forward, the backward is handed bf16(O_ref), fp32(L_ref), the sink and dL and judged against lse_ref.flow fed the same.
Routes: phases 7; 1 then 6; 8 | 1 where the plan says 1 (grouped heads there: the dK / dV gates include the bf16 partials).
A row without a visible key: O = 0 and dQ = 0 exactly, L = its head's sink bit for bit.  dsink keeps its bound of
tests/test_gpu_lse.py (the isolating one, against the float64 value on the arrays the kernel is fed) and gets no row gate.

  (a) sinks: the eight of sink_rows_ref on (8, 2), three on (3, 3); 300^2, 600^2 (causal: the second row block of a pair),
      1024^2 and 1025^2 (the single kernel and its padded length), (257, 64) and (1100, 300) (causal: rows without a key),
      (300, 1100); `scale-one` and `peaked`; `spikes` and `lift` at 1100^2 and (300, 1100) with a sink of 26 on the spiked heads;
  (b) dL of the size of D and 100 x that, with the eight sinks and without, at 300^2, 1024^2, (70, 300) and (300, 70) causal --
      there the rows with L = -inf hold NaN and Inf in dL, and every output is finite and bit-equal to the run with zeros there;
  (c) one two-sided packed batch with sinks and dL through the varlen calls."""
import itertools

import numpy as np
import pytest
import torch

import bf16_rows_ref as B
import regimes as R
import sink_rows_ref as SR
from test_gpu_bf16_rows import Dense, _fa, _mask, _merge, _nan

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def _dsink_gate(label, got, case):
    """dsink: finite, 0 for a head without a sink, and within the isolating bound of tests/test_gpu_lse.py of case.dsink."""
    sk = case.sink.double().numpy()
    has = np.isfinite(sk)
    ds = got.double().cpu().numpy()
    assert np.isfinite(ds).all() and (ds[~has] == 0).all(), (label, "dsink", ds)
    L = case.ref["L"]
    live = has[:, None] & np.isfinite(L)      # (a row without a key has L = s: P_sink = 1, D = 0, and its dL is a term like any other)
    gap = np.where(live, np.abs(sk[:, None] - np.where(np.isfinite(L), L, 0.0)), 0.0)
    terms = (np.abs(B.f64(case.t[3])) * np.abs(B.f64(case.O16))).sum(axis=-1) + (0.0 if case.dL is None else np.abs(B.f64(case.dL)))
    M = (np.where(live, np.exp(-gap), 0.0) * terms).sum(axis=1)
    bound = ((case.d + 1 + case.nq) * U24 + (4 + gap.max(axis=1)) * 4 * U24) * M
    err = np.abs(ds - case.dsink)
    assert (err[has] <= bound[has]).all(), (label, "dsink", err, bound)
    return float((err[has] / np.maximum(bound[has], 1e-300)).max(initial=0.0))


def _run(label, case):
    dev = Dense(case)
    report = B.check(f"{label} forward", dev.forward(), case)
    for phases, single in dev.routes():
        _merge(report, B.check(f"{label} phases {phases}", dev.backward(phases), case, partials=single and case.G > 1))
        if case.sink is not None:
            _merge(report, {"dsink / bound": _dsink_gate(f"{label} phases {phases}", dev.dsink, case)})
    print(B.report_line(label, {n: v for n, v in report.items() if n != "dsink / bound"}) + (f"  dsink/bound {report['dsink / bound']:.3f}" if "dsink / bound" in report else ""))
    return dev


# ---- (a)
@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("heads", SR.HEADS, ids=lambda h: f"H{h[0]}-{h[1]}")
@pytest.mark.parametrize("regime", SR.SINK_REGIMES)
@pytest.mark.parametrize("nq,nk", SR.SINK_SHAPES)
def test_sinks(nq, nk, regime, heads, d, causal):
    _run(f"sink {regime} H{heads[0]}/{heads[1]} {nq}x{nk} d{d} {_mask(causal)}", SR.case(regime, *heads, nq, nk, d, causal))


@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("regime", SR.SPIKED_REGIMES)
@pytest.mark.parametrize("nq,nk", SR.SPIKED_SHAPES)
def test_restart_and_lift_under_a_sink(nq, nk, regime, d, causal):
    """The sink is applied once, to what the row ends with: after the restart with maxima (`spikes`) and after a lift (`lift`)."""
    hq, hkv = R.HEADS_GQA
    case = SR.case(regime, hq, hkv, nq, nk, d, causal)
    for h, r, j, i in R.spike_rows(nq, nk, hq, causal, R.SPIKED[regime]):
        assert case.ref["L"][h, r] > max(R.SPIKE_L[i], SR.SPIKE_SINK), "the reference row does not see its spike"
    _run(f"sink {regime} H{hq}/{hkv} {nq}x{nk} d{d} {_mask(causal)}", case)


# ---- (b)
@pytest.mark.parametrize("with_sink", [False, True], ids=["plain", "sinks"])
@pytest.mark.parametrize("scale", SR.DL_SCALES, ids=lambda s: f"x{s:g}")
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("shape,causal", [(s, c) for s, masks in SR.DL_SHAPES for c in masks], ids=lambda x: _mask(x) if isinstance(x, bool) else f"{x[0]}x{x[1]}")
def test_a_gradient_for_l(shape, causal, d, scale, with_sink):
    nq, nk = shape
    hq, hkv = R.HEADS_GQA
    case = SR.case(SR.DL_REGIME, hq, hkv, nq, nk, d, causal, with_sink, scale)
    label = f"dL x{scale:g} {'sinks' if with_sink else 'plain'} {nq}x{nk} d{d} {_mask(causal)}"
    dev = _run(label, case)
    none = np.isneginf(case.ref["L"])
    if (nq, nk, causal) == (300, 70, True) and not with_sink:
        assert none[:, :230].all() and not none[:, 230:].any()
    if not none.any():
        return
    # the rows with L = -inf ignore their dL, whatever it holds: zeros, NaN and Inf there give the same finite bits
    mask = torch.from_numpy(none)[None].cuda()
    clean = dev.dL.clone()
    runs = []
    for poison in (0.0, float("nan"), float("inf")):
        dev.dL = torch.where(mask, torch.full_like(clean, poison), clean)
        runs.append((dev.backward((7,)), None if dev.dsink is None else dev.dsink.clone()))
    dev.dL = clean
    for (got, ds), poison in zip(runs[1:], ("NaN", "Inf")):
        for n in B.GRADS:
            assert torch.isfinite(got[n].float()).all(), (label, n, poison)
            assert torch.equal(got[n], runs[0][0][n]), (label, n, f"dL = {poison} on the rows with L = -inf")
        assert ds is None or torch.equal(ds, runs[0][1]), (label, "dsink", poison)
    B.check(f"{label} dL = 0 on the rows with L = -inf", runs[0][0], case)


# ---- (c)
@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
def test_a_packed_batch_with_sinks_and_dl(d, causal):
    fa = _fa()
    case = SR.packed(d, causal)
    cq, ck = ([0] + list(itertools.accumulate(x)) for x in zip(*SR.PACKED))
    plan = fa.VarlenPlan(cq, ck)
    assert plan.two_sided
    Q, K, V, dO, O16, L32, sink, dL = (t.contiguous().cuda() for t in case.t + (case.O16, case.L32, case.sink, case.dL))
    O, L = _nan(Q.shape, torch.bfloat16), _nan(Q.shape[:2], torch.float32)
    dQ, dK, dV = _nan(Q.shape, torch.bfloat16), _nan(K.shape, torch.bfloat16), _nan(V.shape, torch.bfloat16)
    dsink = _nan((case.hq,), torch.float32)
    fa.flash_attention_2_varlen_forward(Q, K, V, plan, case.s, causal=causal, O=O, L=L, sink=sink)
    fa.flash_attention_2_varlen_backward(Q, K, V, O16, L32, dO, plan, case.s, causal=causal, dQ=dQ, dK=dK, dV=dV, sink=sink, dsink=dsink, dL=dL)
    torch.cuda.synchronize()
    label = f"packed sinks dL d{d} {_mask(causal)}"
    report = B.check(f"{label} forward", {"O": O, "L": L}, case)
    _merge(report, B.check(f"{label} backward", {"dQ": dQ, "dK": dK, "dV": dV}, case))
    print(B.report_line(label, report) + f"  dsink/bound {_dsink_gate(label, dsink, case):.3f}")
