"""CPU: what the row gate of the cache-side attention family rests on (tests/decode_rows_ref.py, tests/decode_rows_cases.py).

(i) THE CERTIFICATE.  The CPU emulations of the kernels' data flow use at most ROOM = 0.75 of the O row gate, of the L gates and
of the tensor gate on every row of: every decode_ref case on bf16 and e4m3 caches at 1 and 7 splits; every decode_window_ref case
on both cache kinds at 1 and 5 splits; the subset decode_rows_cases.cert_subset of the extend and ragged (case, variant, cache
kind) triples at 1 and 7 splits (printed by test_the_subset_covers_what_it_must); every regime run of tests/test_gpu_decode_rows.py
on both cache kinds under its three windows at 1 and 7 splits.  test_kappa_is_the_smallest prints the largest ratio per family
(DESIGN.md section 6d quotes them) and asserts that KAPPA - 0.5 would not do.
(ii) THE REGIMES, from the reference alone: on the bf16 caches a row that sees a spike has L above regimes.SPIKE_L, and every
finite `low-level` L lies below -88 (both cache kinds).
(iii) THE GAP, PINNED.  Mutants m1 .. m5 of decode_rows_cases on the emulation: the row gate fails on every row a mutant touches
and holds on every other; on decode_ref.CASES[2], [5] and [9] the tensor gate PASSES m1 and m2 -- why the row gate exists.
(iv) THE FORMULA on a case checked by hand: one visible key gives P = 1, O = v, gate (KAPPA + 1) u |v|; a keyless row has gate 0."""
import numpy as np
import pytest
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_cases as rc
import decode_rows_ref as rows
import decode_window_ref as wr
import extend_ragged_ref as rr
import extend_ref as er
import regimes

FAMILIES = ("decode", "e4m3 decode", "windowed", "extend", "ragged extend", "regime runs")
SEEN = {f: [] for f in FAMILIES}      # family -> [(label, row errors, u quad, u |O_ref|)] of what ran
RAN = {f: 0 for f in FAMILIES}
EXPECTED = {"decode": len(dr.CASES), "e4m3 decode": len(dr.CASES), "windowed": len(wr.CASES), "extend": 2 * len(er.CASES),
            "ragged extend": 2 * len(rr.CASES), "regime runs": len(rc.RUNS)}


def _certify(family, label, O, L, ref):
    e = dr.errors(O, L, ref)
    r = rows.ratios(O, ref)
    top = float(r.max(initial=0.0))
    print(f"ROWS-CPU {family} {label}: row ratio {top:.3f}  O rel-L2 {e[0]:.2e}  dL {e[1]:.2e}  dL(|L| > 25) {e[2]:.2e}")
    assert top <= rows.ROOM, (family, label, top)
    assert e[0] <= rows.ROOM * dr.BF16_REL and e[1] <= rows.ROOM * dr.L_ABS and e[2] <= rows.ROOM * dr.L_ABS_LARGE and e[3], (family, label, e)
    SEEN[family].append((label, rows.row_errors(O, ref).ravel(), rows.U * np.nan_to_num(ref.quad).ravel(),
                         rows.U * np.nan_to_num(np.linalg.norm(ref[0], axis=-1)).ravel()))


# ------------------------------------------------------------------------------------------------ (i)
@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=[dr.case_id(c) for c in dr.CASES])
def test_certificate_decode(i):
    c = dr.CASES[i]
    Q, K, V, scale, lens, sink = dr.inputs(i)
    for n_splits in (1, 7):
        _certify("decode", f"{dr.case_id(c)} splits {n_splits}", *dr.emulate(Q, K, V, lens, scale, c["causal"], sink, n_splits), dr.reference(i))
        _certify("e4m3 decode", f"{dr.case_id(c)} splits {n_splits}", *fr.emulate(i, n_splits), fr.reference(i))
    RAN["decode"] += 1
    RAN["e4m3 decode"] += 1


@pytest.mark.parametrize("i", range(len(wr.CASES)), ids=wr.IDS)
def test_certificate_windowed(i):
    c = wr.CASES[i]
    Q, K, V, scale, lens, sink = wr.inputs(i)
    for fp8 in (False, True):
        Kc, Vc = wr.dequantised(i) if fp8 else (K, V)
        for n_splits in (1, 5):
            _certify("windowed", f"{wr.IDS[i]} {'e4m3' if fp8 else 'bf16'} splits {n_splits}",
                     *wr.emulate(Q, Kc, Vc, lens, scale, sink, c["wl"], n_splits), wr.reference(i, fp8))
    RAN["windowed"] += 1


EXTEND_SUBSET, RAGGED_SUBSET = rc.cert_subset(len(er.CASES)), rc.cert_subset(len(rr.CASES))
_sub_id = lambda ids: (lambda t: f"{ids[t[0]]}-{er.variant_id(er.VARIANTS[t[1]])}-{'e4m3' if t[2] else 'bf16'}")


@pytest.mark.parametrize("run", EXTEND_SUBSET, ids=_sub_id(er.IDS))
def test_certificate_extend(run):
    i, k, fp8 = run
    c = er.CASES[i]
    mask, wl = er.VARIANTS[k]
    Q, K, V, scale, _, sink = er.inputs(i)
    if fp8:
        K, V = er.dequantised(i)
    sink = sink if er.has_sink(i, k) else None
    for n_splits in rc.CERT_SPLITS:
        O, L = rc.emulate(Q, K, V, list(c["lens"]), scale, mask == "causal", sink, wl, n_splits)
        _certify("extend", f"{_sub_id(er.IDS)(run)} splits {n_splits}", O, L, er.reference(i, k, fp8))
    RAN["extend"] += 1


@pytest.mark.parametrize("run", RAGGED_SUBSET, ids=_sub_id(rr.IDS))
def test_certificate_ragged(run):
    i, k, fp8 = run
    c = rr.CASES[i]
    mask, wl = rr.VARIANTS[k]
    Q, K, V, scale, _, sink, _ = rr.inputs(i)
    if fp8:
        K, V = rr.dequantised(i)
    sink = sink if rr.has_sink(i, k) else None
    for n_splits in rc.CERT_SPLITS:
        O, L = rc.emulate_ragged(Q, K, V, c["qs"], c["lens"], scale, mask == "causal", sink, wl, n_splits)
        _certify("ragged extend", f"{_sub_id(rr.IDS)(run)} splits {n_splits}", O, L, rr.reference(i, k, fp8))
    RAN["ragged extend"] += 1


def test_the_subset_covers_what_it_must():
    """Every shape at both head dims, both cache kinds, and causal, full, w31 and w200 each on both cache kinds and head dims."""
    for name, subset, cases, ids in (("extend", EXTEND_SUBSET, er.CASES, er.IDS), ("ragged", RAGGED_SUBSET, rr.CASES, rr.IDS)):
        print(f"{name} certificate subset:", " ".join(_sub_id(ids)(t) for t in subset))
        assert {i for i, _, fp8 in subset if fp8} == {i for i, _, fp8 in subset if not fp8} == set(range(len(cases)))
        for fp8 in (False, True):
            for d in rc.HEAD_DIMS:
                assert {k for i, k, f in subset if f == fp8 and cases[i]["d"] == d} == set(rc.CERT_VARIANTS), (name, fp8, d)
    assert [er.VARIANTS[k] for k in rc.CERT_VARIANTS] == [("causal", None), ("full", None), ("causal", 31), ("causal", 200)]


def _spike_rows(body, wl):
    """[(row index into the reference's L, i)] of the rows that see spike i under the causal mask and the window."""
    qs, lens = rc.shape_of(body)
    cu = rr.cu_of(qs)
    out = []
    for b, (nq, n) in enumerate(zip(qs, lens)):
        for h, r, j, i in regimes.spike_rows(nq, n, rc.HQ, True):
            if wl is None or j >= r + n - nq - wl:
                out.append(((cu[b] + r, h) if body == "ragged" else (b, h, r), i))
    return out


@pytest.mark.parametrize("run", rc.RUNS, ids=rc.RUN_IDS)
def test_certificate_regime_runs(run):
    body, d, regime = run
    for kind in rc.KINDS:
        for wi, wl in enumerate(rc.WINDOWS):
            ref = rc.reference(body, d, regime, kind, wi)
            for n_splits in rc.CERT_SPLITS:
                O, L = rc.emulate_run(body, d, regime, kind, wi, n_splits)
                _certify("regime runs", f"{rc.RUN_IDS[rc.RUNS.index(run)]} {kind} w{wl} splits {n_splits}", O, L, ref)
            # (ii) the regimes, from the reference alone
            rL = ref[1]
            if regime == "spikes" and kind == "bf16":
                seen = _spike_rows(body, wl)
                assert seen, (run, wl)
                for index, i in seen:
                    assert rL[index] > regimes.SPIKE_L[i], (run, wl, index, rL[index])
                if wl is None:
                    assert {i for _, i in seen} == {0, 1}
            if regime == "low-level":
                assert np.isfinite(rL).all() and (rL < regimes.LOW_LEVEL_L).all(), (run, kind, wl, rL.max())
    RAN["regime runs"] += 1


def _worst(kappa, entries):
    top = 0.0
    for _, e, quad, rest in entries:
        with np.errstate(divide="ignore", invalid="ignore"):
            top = max(top, float(np.where(e == 0.0, 0.0, e / (kappa * quad + rest)).max(initial=0.0)))
    return top


def test_kappa_is_the_smallest():
    """Over what ran before this test (the whole file: every family): the largest ratio per family at KAPPA and at the multiples
    of 0.5 around it, and -- when everything ran -- that KAPPA - 0.5 leaves some row above ROOM."""
    for kappa in (rows.KAPPA - 0.5, rows.KAPPA, rows.KAPPA + 0.5, rows.KAPPA + 1.0):
        print(f"KAPPA {kappa}: " + "  ".join(f"{f} {_worst(kappa, SEEN[f]):.3f}" for f in FAMILIES))
    assert rows.KAPPA <= rows.KAPPA_BOUND and rows.KAPPA % 0.5 == 0.0
    assert all(_worst(rows.KAPPA, SEEN[f]) <= rows.ROOM for f in FAMILIES)
    if RAN == EXPECTED:
        assert rows.KAPPA == 0.5 or max(_worst(rows.KAPPA - 0.5, SEEN[f]) for f in FAMILIES) > rows.ROOM


# ------------------------------------------------------------------------------------------------ (iii)
def _fails_exactly(label, O, L, ref, touched, tensor_gate_passes=None):
    """The row gate fails on every touched row and on no other; L stays inside its gates."""
    r = rows.ratios(O, ref)
    print(f"ROWS-MUTANT {label}: touched rows {r[touched].min():.2f} .. {r[touched].max():.2f} x gate, the others at most "
          f"{r[~touched].max(initial=0.0):.2f}; tensor rel-L2 {dr.errors(O, L, ref)[0]:.2e}")
    assert (r[touched] > 1.0).all(), (label, float(r[touched].min()))
    assert (r[~touched] <= rows.ROOM).all(), label
    e = dr.errors(O, L, ref)
    assert e[1] <= dr.L_ABS and e[2] <= dr.L_ABS_LARGE and e[3], (label, e)
    if tensor_gate_passes is not None:
        assert dr.within_gates(e) == tensor_gate_passes, (label, e)


def _touched(shape, b, rows_=None, heads=None):
    t = np.zeros(shape, dtype=bool)
    t[b, slice(None) if heads is None else heads, slice(None) if rows_ is None else rows_] = True
    return t


@pytest.mark.parametrize("n_splits", [1, 7])
@pytest.mark.parametrize("i", [2, 5, 9])
def test_m1_m2_pass_the_tensor_gate_and_fail_the_row_gate(i, n_splits):
    c = dr.CASES[i]
    Q, K, V, scale, lens, sink = dr.inputs(i)
    ref = dr.reference(i)
    args = (Q, K, V, lens.tolist(), scale, c["causal"], sink, None, n_splits)
    assert max(c["lens"]) == 2500 and c["regime"] is None
    O, L, b = rc.m1_last_tile_missing_from_pv(*args)
    _fails_exactly(f"m1 CASES[{i}] splits {n_splits}", O, L, ref, _touched(L.shape, b), tensor_gate_passes=True)
    O0, L0 = rc.emulate(*args)
    assert np.array_equal(L, L0)      # the second product alone
    O, b = rc.m2_scaled(O0, c["lens"])
    _fails_exactly(f"m2 CASES[{i}] splits {n_splits}", O, L0, ref, _touched(L.shape, b), tensor_gate_passes=True)


def test_m3_m5_on_the_decode():
    i = 2
    c = dr.CASES[i]
    assert (c["hq"], c["hkv"], c["nq"]) == (3, 3, 4)
    Q, K, V, scale, lens, sink = dr.inputs(i)
    ref = dr.reference(i)
    args = (Q, K, V, lens.tolist(), scale, c["causal"], sink, None, 7)
    O0, L0 = rc.emulate(*args)
    O, b = rc.m3_rows_exchanged(O0, c["lens"], 1, 2)
    _fails_exactly("m3 CASES[2]", O, L0, ref, _touched(L0.shape, b, rows_=[1, 2]))
    O, L, b = rc.m5_next_heads_v(*args)
    assert np.array_equal(L, L0)
    _fails_exactly("m5 CASES[2]", O, L, ref, _touched(L0.shape, b))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_m1_to_m4_on_an_extend_shape(fp8):
    """(8, 2), N_q = 17 at d = 64 under window 200: heads 0 and 1 share a K/V head and lie in one row tile."""
    i, k = er.IDS.index("8-2-q17-d64"), 7
    c = er.CASES[i]
    mask, wl = er.VARIANTS[k]
    assert wl == 200 and c["hq"] // c["hkv"] > 1
    Q, K, V, scale, _, sink = er.inputs(i)
    if fp8:
        K, V = er.dequantised(i)
    ref = er.reference(i, k, fp8)
    args = (Q, K, V, list(c["lens"]), scale, True, sink if er.has_sink(i, k) else None, wl, 7)
    O0, L0 = rc.emulate(*args)
    O, L, b = rc.m1_last_tile_missing_from_pv(*args)
    assert np.array_equal(L, L0) and c["lens"][b] == 2500      # (keys 2464 .. 2495: inside every row's window, the last 201 keys)
    _fails_exactly("m1 extend", O, L, ref, _touched(L0.shape, b))
    O, b = rc.m2_scaled(O0, c["lens"])
    _fails_exactly("m2 extend", O, L0, ref, _touched(L0.shape, b))
    O, b = rc.m3_rows_exchanged(O0, c["lens"], 15, 16)
    _fails_exactly("m3 extend", O, L0, ref, _touched(L0.shape, b, rows_=[15, 16]))
    O, b = rc.m4_heads_exchanged(O0, c["lens"], 0, 1)
    _fails_exactly("m4 extend", O, L0, ref, _touched(L0.shape, b, heads=[0, 1]))


def test_m3_on_a_ragged_batch():
    """Two tokens of the longest sequence of `mixed` (q_b = 40 against 2500 keys) exchanged in the token-major O."""
    i, k = rr.IDS.index("mixed-d128"), 0
    c = rr.CASES[i]
    Q, K, V, scale, _, sink, _ = rr.inputs(i)
    ref = rr.reference(i, k, False)
    O, L = rc.emulate_ragged(Q, K, V, c["qs"], c["lens"], scale, True, sink if rr.has_sink(i, k) else None, None, 7)
    b = rc.longest(c["lens"])
    t = rr.cu_of(c["qs"])[b]
    O = O.copy()
    O[[t + 38, t + 39]] = O[[t + 39, t + 38]]
    touched = np.zeros(L.shape, dtype=bool)
    touched[[t + 38, t + 39]] = True
    _fails_exactly("m3 ragged", O, L, ref, touched)


# ------------------------------------------------------------------------------------------------ (iv)
def test_the_formula_by_hand():
    d = 64
    g = torch.Generator().manual_seed(7)
    Q, K, V = ((torch.rand(2, 1, n, d, generator=g) - 0.5).bfloat16() for n in (1, 4, 4))
    ref = pr.reference64(Q, K, V, [1, 0], 0.125, True, None)
    v = np.linalg.norm(V[0, 0, 0].double().numpy())
    np.testing.assert_array_equal(ref[0][0, 0, 0], V[0, 0, 0].double().numpy())                  # one visible key: P = 1, O = v
    np.testing.assert_allclose(rows.gate(ref)[0, 0, 0], (rows.KAPPA + 1.0) * 2.0 ** -9 * v, rtol=1e-14)
    assert rows.gate(ref)[1, 0, 0] == 0.0 and np.isneginf(ref[1][1, 0, 0])                       # no key: gate 0, O exactly 0
    O = ref[0].copy()
    assert rows.ratios(O, ref).max() == 0.0
    O[1, 0, 0, 5] = 1e-30
    assert np.isinf(rows.ratios(O, ref)[1, 0, 0])
    with pytest.raises(AssertionError, match=r"sequence 1, head 0, token 0"):
        rows.check("by hand", O, ref)
    # a sink beside the one key: P = w = 1 / (1 + exp(sink - s)), O = w v, gate (KAPPA + 1) u w |v|; alone: L = sink, gate 0
    sink = torch.tensor([0.75])
    ref = pr.reference64(Q, K, V, [1, 0], 0.125, True, sink)
    s = 0.125 * float(Q[0, 0, 0].double() @ K[0, 0, 0].double())
    w = 1.0 / (1.0 + np.exp(0.75 - s))
    np.testing.assert_allclose(rows.gate(ref)[0, 0, 0], (rows.KAPPA + 1.0) * 2.0 ** -9 * w * v, rtol=1e-12)
    assert rows.gate(ref)[1, 0, 0] == 0.0 and ref[1][1, 0, 0] == 0.75
    # the window's reference and the ragged one carry the same gate
    np.testing.assert_allclose(wr.reference64(Q, K, V, [1, 0], 0.125, sink, 3).quad, ref.quad, rtol=1e-14)
    rag = rr.reference64(Q[:, 0], K, V, (1, 1), [1, 0], 0.125, True, sink, None)
    np.testing.assert_allclose(rag.quad, ref.quad[:, :, 0], rtol=1e-14)
    # two bf16 partials merged: u (w_a |O_a| + w_b |O_b|) on top
    a, b_ = (np.ones((1, 1, 1, d)), np.array([[[0.0]]])), (2.0 * np.ones((1, 1, 1, d)), np.array([[[-np.inf]]]))
    np.testing.assert_allclose(rows.merged_extra([a, b_], np.array([[[0.0]]])), 2.0 ** -9 * 8.0)
