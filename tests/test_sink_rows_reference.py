"""CPU: the row gates of bf16_rows_ref.Case with a sink and with a gradient for L, certified before a kernel sees them
(DESIGN.md section 6e).  KAPPA, PHI, ROOM and the L figures are bf16_rows_ref's; nothing here comes from a kernel.

ROOM.  On every case tests/test_gpu_sink_rows.py hands a kernel (sink_rows_ref.cpu_cases()) the emulation -- the forward at both
references followed by the sink epilogue, the backward as lse_ref.flow(kernel_formats=True) with bf16 outputs, and with bf16
per-head partials where grouped heads run the single kernel -- uses at most ROOM = 0.75 of every row gate and stays inside the L
gates.  Every case prints its ratios (pytest -s); DESIGN.md section 6e keeps the largest per regime and tensor.
BY HAND.  A 2-row, 3-key problem with a sink and a dL, every term of the O and dQ gates written out.
TEETH.  Every mutant of sink_rows_ref (k1 .. k7) fails the row gate on the rows it touches and on no others; the tensor gates of
tests/test_gpu_sink.py and tests/test_gpu_lse.py are computed on the same arrays, printed, and asserted to PASS where they do
(PASSED_BY_THE_TENSOR_GATES): that is the gap the row gates close."""
import math

import numpy as np
import pytest
import torch

import bf16_rows_ref as B
import sink_rows_ref as SR

CASES = {label: (build, args) for label, build, args in SR.cpu_cases()}
BITE = 1.5
PASSED_BY_THE_TENSOR_GATES = {"k2", "k3", "k4"}      # (k5, k6: a dL of the size of D on 300 rows is no m8 -- rel-L2 6e-3 .. 3e-2)


def _largest(rat):
    return {n: float(r.max(initial=0.0)) for n, r in rat.items()}


@pytest.mark.parametrize("label", list(CASES))
def test_every_gpu_case_leaves_the_kernels_room(label):
    build, args = CASES[label]
    case = build(*args)
    worst = {}
    runs = [(f"forward -{off:g}", False, case.emulate_forward(off)) for off in B.FWD_OFFSETS] + [("backward", False, case.emulate_backward())]
    if SR.runs_partials(case):
        runs.append(("backward, bf16 partials", True, case.emulate_backward(True)))
    for name in ("O",) + B.GRADS:
        gate = case.gate(name)
        has = ~case.keyless if name in ("O", "dQ") else case.key_seen
        assert np.isfinite(gate).all() and (gate[has] > 0).all(), (label, name, "a zero or infinite gate")
    for what, partials, got in runs:
        for name, m in _largest(B.ratios(got, case, partials)).items():
            assert m <= (1e-6 if name == "L" else B.ROOM), (label, what, name, m)
            worst[name] = max(worst.get(name, 0.0), m)
    print(f"ROOM {label} ({case.regime}): " + " ".join(f"{n} {m:.3f}" for n, m in worst.items() if n != "L"))


def test_without_a_sink_and_dl_a_case_is_what_it_was():
    """sink = None and dL = None take the old path; a sink of -inf everywhere and a zero dL give the same references and gates to
    rounding of the float64 formulas (the arrays are not the same bits: lse_ref sums in another order)."""
    import regimes as R
    t = R.sequence("scale-one", 3, 3, 257, 64, 64)
    old = B.Case("scale-one", *t, True)
    new = B.Case("scale-one", *t, True, torch.full((3,), -math.inf), torch.zeros(3, 257))
    assert old.sink is None and old.dL is None and old.dsink is None
    for n in B.OUTPUTS:
        assert np.allclose(old.ref[n], new.ref[n], rtol=1e-9, atol=1e-12, equal_nan=True), n
    for n in ("O",) + B.GRADS:
        assert np.allclose(old.gate(n), new.gate(n), rtol=1e-9, atol=1e-15), n
    assert np.array_equal(old.keyless, np.isneginf(old.ref["L"])) and old.keyless[:, :193].all() and not old.keyless[:, 193:].any()


def test_the_gate_by_hand_with_a_sink_and_a_dl():
    """2 rows, 3 keys, d = 2, one head, scale 1, no mask, sink = 0.5, dL = (0.25, -2): every term of the O and dQ gates."""
    bf = lambda x: torch.tensor(x, dtype=torch.float64).bfloat16()[None]
    Q, K = bf([[1.0, 0.0], [0.5, 0.5]]), bf([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    V, dO = bf([[1.0, 2.0], [-1.0, 0.5], [0.25, 0.0]]), bf([[0.5, -0.25], [0.125, 1.0]])
    sink, dL = torch.tensor([0.5]), torch.tensor([[0.25, -2.0]])
    c = B.Case("scale-one", Q, K, V, dO, 1.0, False, sink, dL)
    q, k, v, g = (x[0] for x in (c.q, c.k, c.v, c.g))
    S = q @ k.T
    L = np.log(np.exp(S).sum(axis=1) + math.exp(0.5))
    assert np.allclose(c.ref["L"][0], L, rtol=1e-14)
    L32 = L.astype(np.float32).astype(np.float64)
    P = np.exp(S - L32[:, None])
    assert (P.sum(axis=1) < 1).all() and np.allclose(1 - P.sum(axis=1), np.exp(0.5 - L32), rtol=1e-6)      # the rest stays with the sink
    O = np.exp(S - L[:, None]) @ v
    assert np.allclose(c.ref["O"][0], O, rtol=1e-13)
    O16 = B._bf16(O)
    vn, kn = np.linalg.norm(v, axis=1), np.linalg.norm(k, axis=1)
    for i in range(2):
        gate_o = B.KAPPA * B.U * math.sqrt(sum(P[i, j] ** 2 * vn[j] ** 2 for j in range(3))) + B.U * np.linalg.norm(O[i])
        assert math.isclose(c.gate("O")[0, i], gate_o, rel_tol=1e-12)
        Dp = float(g[i] @ O16[i]) - float(dL[0, i])
        dS = [P[i, j] * (float(g[i] @ v[j]) - Dp) for j in range(3)]
        e = [B.PHI * P[i, j] * (float(np.abs(g[i]) @ np.abs(v[j])) + float(np.abs(g[i]) @ np.abs(O16[i])) + abs(float(dL[0, i]))) for j in range(3)]
        dQ = sum(dS[j] * k[j] for j in range(3))
        assert np.allclose(c.ref["dQ"][0, i], dQ, rtol=1e-12)
        gate_q = B.KAPPA * B.U * math.sqrt(sum(dS[j] ** 2 * kn[j] ** 2 for j in range(3))) + sum(e[j] * kn[j] for j in range(3)) + B.U * np.linalg.norm(dQ)
        assert math.isclose(c.gate("dQ")[0, i], gate_q, rel_tol=1e-12)
    ds = -sum(math.exp(0.5 - L32[i]) * (float(g[i] @ O16[i]) - float(dL[0, i])) for i in range(2))
    assert math.isclose(c.dsink[0], ds, rel_tol=1e-12)


def test_a_row_without_a_key_is_gated_exactly_under_a_sink():
    """(1100, 300) causal: rows 0 .. 799 see no key -- O = 0, dQ = 0, L = the head's sink bit for bit (-inf on the head without)."""
    case = SR.case("scale-one", 8, 2, 1100, 300, 64, True)
    sink = case.sink.double().numpy()
    assert case.keyless[:, :800].all() and not case.keyless[:, 800:].any()
    assert (case.ref["L"][:, :800] == sink[:, None]).all() and np.isneginf(case.ref["L"][0, :800]).all()
    assert (case.ref["O"][:, :800] == 0).all() and (case.ref["dQ"][:, :800] == 0).all()
    got = dict(case.emulate_forward(0.0), **case.emulate_backward())
    assert max(_largest(B.ratios(got, case)).values()) <= B.ROOM
    for name, value in (("O", 1e-30), ("dQ", 1e-30), ("L", float(np.nextafter(np.float32(sink[3]), np.float32(9))))):
        bad = {n: x.copy() for n, x in got.items()}
        bad[name][3, 17] = value
        assert np.isinf(B.ratios(bad, case)[name][3, 17])
        with pytest.raises(AssertionError, match=rf"{name} row gate missed at \(h 3, row 17\)"):
            B.check("empty rows", bad, case)
    drop = B.Case("scale-one", *case.t, case.s, True, None, torch.full((8, 1100), 3.0))
    assert (drop.ref["dQ"][:, :800] == 0).all() and np.isneginf(drop.ref["L"][:, :800]).all()      # dL dropped where L = -inf


# ------------------------------------------------------------------------------------------------ teeth
def _bites(what, case, got, name, head, rows, also=None):
    """The mutant fails `name` on rows `rows` of `head` (by at least BITE) and no row fails any gate outside the rows it touches
    (also: {tensor: (head, rows)} -- the key rows a faulty query row reaches in dK and dV)."""
    rat = B.ratios(got, case, SR.runs_partials(case))
    hit = float(rat[name][head, rows].max())
    touched = dict(also or {}, **{name: (head, rows)})
    for n, r in rat.items():
        r = r.copy()
        if n in touched:
            r[touched[n]] = 0.0
        assert r.max(initial=0.0) <= 1.0, (what, n, "a row outside the fault fails")
    assert hit >= BITE, (what, name, hit)
    with pytest.raises(AssertionError, match=f"{name} row gate missed"):
        B.check(what, got, case)
    figs, ok = SR.tensor_gates(got, case)
    print(f"TEETH {what}: {name} {hit:.1f} x the row gate; the tensor gates " + ("PASS" if ok else "fail") + " it: " +
          " ".join(f"{n} {v:.2e}" for n, v in figs.items()))
    assert ok == (what.split()[0] in PASSED_BY_THE_TENSOR_GATES), (what, figs)
    return hit


@pytest.mark.parametrize("off", B.FWD_OFFSETS)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
def test_sink_mutants_of_the_forward_break_a_row_gate(d, off):
    case = SR.case("scale-one", 8, 2, 600, 600, d, True)
    got, rows = SR.k1_sink_factor_twice(case, off, 4)
    _bites(f"k1 d{d} -{off:g}", case, got, "O", 4, rows)
    got, head = SR.k2_head_is_zero(case, off)
    _bites(f"k2 d{d} -{off:g}", case, got, "O", head, slice(None))
    got, head = SR.k3_head_is_scaled(case, off)
    _bites(f"k3 d{d} -{off:g}", case, got, "O", head, slice(None))


@pytest.mark.parametrize("d", B.HEAD_DIMS)
def test_a_shifted_mask_in_the_backward_of_a_sinked_head_breaks_a_row_gate(d):
    """(3, 3): the mutants of bf16_rows_ref splice one head's blocks, which needs ungrouped heads.  Head 1 has log N_k + 3."""
    case = SR.case("scale-one", 3, 3, 600, 600, d, True)
    keys = (1, slice(0, 417))                                               # what rows 384 .. 415 reach with the mask one key further
    _bites(f"k4 d{d}", case, SR.k4_mask_shifted_backward(case, 1, 12), "dQ", 1, slice(384, 416), {"dK": keys, "dV": keys})


@pytest.mark.parametrize("with_sink", [False, True])
@pytest.mark.parametrize("scale", SR.DL_SCALES)
def test_dl_mutants_break_a_row_gate(scale, with_sink):
    case = SR.case(SR.DL_REGIME, 8, 2, 300, 300, 128, True, with_sink, scale)
    tag = f"x{scale:g} {'sinks' if with_sink else 'plain'}"
    got = SR.k5_neighbours_dl(case, 3, 200)                                 # (query head 3 attends K/V head 0)
    _bites(f"k5 {tag}", case, got, "dQ", 3, slice(200, 201), {"dK": (0, slice(0, 201))})
    assert B.ratios(got, case)["dV"].max() <= B.ROOM                        # dV = P^T dO does not see dL
    _bites(f"k6 {tag}", case, SR.k6_dl_ignored(case, 3, 6), "dQ", 3, slice(192, 224), {"dK": (0, slice(0, 224))})


def test_a_nan_from_a_multiplied_in_dl_is_refused():
    case = SR.case(SR.DL_REGIME, 8, 2, 300, 70, 64, True, False, 1.0)
    got = SR.k7_dl_multiplied_in(case, 0, 5)
    with pytest.raises(AssertionError, match="NaN left in dQ"):
        B.check("k7", got, case)
    with pytest.raises(AssertionError, match="NaN left in dK"):
        B.check("k7", {"dK": got["dK"]}, case)
    figs, ok = SR.tensor_gates(got, case)
    print("TEETH k7: NaN in dQ and dK; the tensor gates " + ("PASS" if ok else "fail") + " it (tests/test_gpu_lse.py asserts every output finite)")
    assert not ok
