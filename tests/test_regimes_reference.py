"""CPU: the inputs and references of tests/regimes.py, certified before a kernel sees them.

For every (regime, sequence shape, head_dim, causal) that tests/test_gpu_regimes.py hands a kernel:
  * the inputs are what they claim -- bf16 tensors of the stated shapes, scaled scores of the stated spread, the means of V and
    dO, L below -88 throughout the low-level regime, L of 11 to 22 in the peaked one at 1100 keys, the spikes above 25 and 120
    wherever the mask lets their rows see them (and nothing above 45 in the lift regime), and head 0 of the 3-head spikes problem untouched by them;
  * the kernels' data flow itself leaves room under the project's 5e-3 gate: emulate() (D in fp32, P and dS in bf16) stays within
    2.5e-3 rel-L2 -- half the gate -- of ref_flow() fed the same bf16 O and fp32 L, on dQ, dK and dV.  dQ of the low-level regime
    is exempt: K is nearly constant there, the rows of dS sum to zero and dQ = dS K cancels to ~1e-4 of its terms (measured
    3.4e-2 at d = 128, up to 7.2e-2 at d = 64; the GPU file gives it the gate of test_ragged_lengths_run_the_single_kernel).
    Measured (rel-L2, worst over dQ, dK, dV and every case here): scale-one 1.8e-3, scale-small 1.8e-3, peaked 1.9e-3, spikes
    2.1e-3 (dQ, 1024 x 1024, d = 128, causal), offsets 1.8e-3, low-level 2.0e-3 on dK / dV, lift 1.9e-3.
The reference is pinned: ref_flow fed the exact float64 O and L is ref_attention's backward to 1e-12 relative.  The scale is what
is applied: folding s into Q and passing scale 1 gives the same reference."""
import itertools

import numpy as np
import pytest
import torch

import regimes as R

EMU_GATE = 2.5e-3                         # half the bf16 gate of 5e-3
CASES = tuple(itertools.product(R.problems(), (64, 128), (False, True)))


def _id(case):
    (hq, hkv, nq, nk), d, causal = case
    return f"{hq}-{hkv}-{nq}x{nk}-d{d}-{'causal' if causal else 'full'}"


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_inputs_are_what_they_claim_and_leave_the_kernels_room(case):
    (hq, hkv, nq, nk), d, causal = case
    for regime in R.REGIMES:
        where = f"{regime} {_id(case)}"
        Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
        assert s == R.scale_of(regime, d)
        for t, shape in ((Q, (hq, nq, d)), (K, (hkv, nk, d)), (V, (hkv, nk, d)), (dO, (hq, nq, d))):
            assert t.dtype == torch.bfloat16 and tuple(t.shape) == shape and not t.is_cuda
            assert torch.equal(t.double().bfloat16(), t) and torch.isfinite(t.float()).all()         # float64 holds them exactly
        again = R.sequence(regime, hq, hkv, nq, nk, d)
        assert all(torch.equal(a, b) for a, b in zip(again[:4], (Q, K, V, dO)))                      # the same data every time
        vbar, gbar = R._TABLE[regime][2:]
        assert abs(float(V.double().mean()) - vbar) < 0.02 and abs(float(dO.double().mean()) - gbar) < 0.008, where      # 5 sigma at (40, 40)
        O, L, dQ, dK, dV = ref = R.ref_grouped(Q, K, V, dO, s, causal)
        seen = np.isfinite(L)
        assert (np.isneginf(L) == ~seen).all() and (seen.all() or (causal and nq > nk)), where
        if causal and nq > nk:
            assert not seen[:, :nq - nk].any() and seen[:, nq - nk:].all(), where                    # the rows without a key
        scores = s * (R.f64(Q)[0] @ R.f64(K)[0].T)
        sigma = R._TABLE[regime][1]
        if regime == "low-level":
            assert L[seen].max() < R.LOW_LEVEL_L and -125.0 < scores.min() and scores.max() < -105.0, (where, L[seen].max())
        elif regime in R.SPIKED:
            which = R.SPIKED[regime]
            for h, r, j, i in R.spike_rows(nq, nk, hq, causal, which):
                assert L[h, r] > R.SPIKE_L[i], (where, h, r, L[h, r])
            if nk >= 57:                                   # every spike visible to its row under the bottom-right mask
                assert len(R.spike_rows(nq, nk, hq, causal, which)) == 2 * len(which), where
            if hq == hkv:                                  # head 0 shares no K/V head with a spike: flat softmax
                assert np.abs(L[0][seen[0]]).max() < 25.0, where
            if regime == "spikes":
                assert L[seen].max() > 120.0 or nk < 34 or not R.spike_rows(nq, nk, hq, causal), where
            else:                                          # no row sum near 2^80 = e^55 above a reference: nothing restarts
                assert L[seen].max() < 45.0, (where, L[seen].max())
        else:
            assert 0.9 * sigma < scores.std() < 1.1 * sigma, (where, scores.std())
            if regime == "peaked" and nk == 1100 and not causal:
                print(where, f"L {L.min():.2f} .. {L.max():.2f}")
                assert 9.0 < L.min() and L.max() < 25.0 and 12.0 < np.median(L) < 17.0, (where, L.min(), L.max())
        O16, L32 = R.kernel_feed(O, L)
        flow = R.ref_flow(Q, K, V, dO, s, causal, O16, L32)
        emu = R.emulate(Q, K, V, dO, s, causal, O16, L32)
        errs = {n: _rel(e, f) for n, e, f in zip(("dQ", "dK", "dV"), emu, flow)}
        drift = {n: _rel(f, r) for n, f, r in zip(("dQ", "dK", "dV"), flow, ref[2:])}
        print(where, "emulate vs ref_flow", " ".join(f"{n} {e:.2e}" for n, e in errs.items()),
              "| ref_flow vs exact", " ".join(f"{n} {e:.2e}" for n, e in drift.items()))
        for n, e in errs.items():
            assert all(np.isfinite(x).all() for x in emu + flow), where
            if regime == "low-level" and n == "dQ":
                continue
            assert e <= EMU_GATE, (where, n, e)


@pytest.mark.parametrize("d,causal", [(64, False), (64, True), (128, False), (128, True)])
def test_ref_flow_fed_the_exact_o_and_l_is_the_reference_backward(d, causal):
    hq, hkv = R.HEADS_GQA
    for regime, (nq, nk) in itertools.product(R.REGIMES, R.QK_SHAPES):
        Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
        O, L, *grads = R.ref_grouped(Q, K, V, dO, s, causal)
        for n, a, b in zip(("dQ", "dK", "dV"), R.ref_flow(Q, K, V, dO, s, causal, O, L), grads):
            assert a.shape == b.shape and _rel(a, b) <= 1e-12, (regime, nq, nk, n, _rel(a, b))
        if causal and nq > nk:
            assert (grads[0][:, :nq - nk] == 0).all()


@pytest.mark.parametrize("d,causal", [(64, True), (128, False)])
def test_the_scale_is_what_is_applied(d, causal):
    """scale-one and scale-small: Q' = s Q under scale 1 is the same problem (s is a power of two: Q' is exact), with dQ' = dQ / s;
    and the scale matters -- the default d^-1/2 on the same tensors gives another L."""
    hq, hkv = R.HEADS_GQA
    nq, nk = R.QK_SHAPES[0]
    for regime in ("scale-one", "scale-small"):
        Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
        want = R.ref_grouped(Q, K, V, dO, s, causal)
        got = R.ref_grouped(R.f64(Q) * s, K, V, dO, 1.0, causal)
        for n, a, b in zip("O L dQ dK dV".split(), got, want):
            assert _rel(a * (s if n == "dQ" else 1.0), b) <= 1e-12, (regime, n)
        other = R.ref_grouped(Q, K, V, dO, d ** -0.5, causal)
        assert np.abs(other[1] - want[1]).max() > 1.0, regime
