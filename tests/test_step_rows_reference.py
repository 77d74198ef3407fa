"""CPU: the reference, the gates, the emulation and the mutants of tests/step_rows_ref.py, certified before the resumable forward
step sees them.  KAPPA, ROOM and the L figures are bf16_rows_ref's; nothing here comes from a kernel.

ROOM.  On every problem tests/test_gpu_step_rows.py runs -- three sets of cuts in every shard order, the strided row range under
both shifts, the two zig-zag ranks; both head dims; at both forward references -- the emulated O uses at most 0.75 of every row
gate and L stays within 1e-6, after the last step and, through the two state invariants, after every step before it.
`low-level`, `spikes` and `lift` need no exemption here: O is row-gated in every regime that runs.
INPUTS.  From the reference alone: every row that sees a spike has L above regimes.SPIKE_L, every `low-level` L lies below -88,
and the cuts put the spike keys where the GPU file's docstring says (the tile and round arithmetic of fa2_fwd1_bf16.hip).
TEETH.  s1 .. s6 fail the row gate on the rows they touch and on no others; the tensor gate of
test_forward_step_meets_the_gates_on_both_shard_orders (rel-L2 <= 5e-3 on O, the L figures) is computed on the same arrays,
printed, and asserted to PASS where it does (PASSED_BY_THE_TENSOR_GATE)."""
import itertools

import numpy as np
import pytest

import bf16_rows_ref as B
import regimes as R
import step_rows_ref as T

BITE = 1.5
PASSED_BY_THE_TENSOR_GATE = set()      # (s4 keeps O within 3e-3 rel-L2, but the old test gates L per row: 4e-3 against 1e-4)


def _room(label, step, order):
    """The emulation of one order at both references against the final reference, and every intermediate state against the
    reference over the keys seen so far; -> the largest O ratio."""
    worst = 0.0
    for off in B.FWD_OFFSETS:
        fin, states, _ = step.emulate(order, off)
        checks = [(fin, step.rows_of(order))] + [(st, step.rows_of(order[:n + 1])) for n, st in enumerate(states)]
        for got, ref in checks:
            for name, r in B.ratios(got, ref).items():
                m = float(r.max(initial=0.0))
                assert m <= (1e-6 if name == "L" else B.ROOM), (label, order, off, name, m)
                worst = max(worst, m if name == "O" else 0.0)
    return worst


@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("cuts", list(T.CUTS))
@pytest.mark.parametrize("regime", T.STEP_REGIMES)
def test_every_dense_step_order_leaves_the_kernel_room(regime, cuts, d):
    step = T.dense_step(regime, d, cuts)
    whole = step.rows()
    assert np.allclose(whole.gate("O"), step.case.gate("O"), rtol=1e-12) and np.allclose(whole.ref["O"], step.case.ref["O"], rtol=1e-9, atol=1e-13)
    worst = max(_room(f"{regime} {cuts} d{d}", step, order) for order in itertools.permutations(range(len(step.shards))))
    print(f"ROOM step {regime} {cuts} d{d}: O {worst:.3f}")


@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("shift", T.STRIDED_SHIFTS + (T.KLEN,))
def test_the_strided_steps_leave_the_kernel_room(shift, d):
    for regime in ("scale-one", "spikes"):
        step = T.strided_step(regime, d, shift)
        print(f"ROOM strided {regime} shift {shift} d{d}: O {_room('strided', step, (0, 1)):.3f}")
    if shift < 0:                                                            # rows that see no key in the second step
        assert not step.visible(step.shards[1])[T.R0:T.R0 - shift].any() and step.visible(step.shards[1])[T.R0 - shift].any()
    if shift >= T.KLEN:
        assert step.visible(step.shards[1])[T.R0:T.R0 + T.QLEN, T.STRIDED_CUT:T.K0 + T.KLEN].all()


@pytest.mark.parametrize("d", B.HEAD_DIMS)
def test_the_zigzag_steps_are_the_causal_problem(d):
    for label, step, whole, rows in T.zigzag_steps(d):
        ref = step.rows()
        assert np.allclose(ref.ref["O"], whole.ref["O"][:, rows], rtol=1e-9, atol=1e-13) and np.allclose(ref.ref["L"], whole.ref["L"][:, rows], rtol=1e-12)
        assert np.allclose(ref.gate("O"), whole.gate("O")[:, rows], rtol=1e-9)
        for order in ((0, 1), (1, 0)):
            print(f"ROOM zigzag {label} order {order} d{d}: O {_room(label, step, order):.3f}")


def test_the_inputs_do_what_the_gpu_file_says():
    for d in B.HEAD_DIMS:
        tile = 64 if d == 128 else 128
        ref = T.dense_step("spikes", d, "two").rows()
        for h, r, j, i in R.spike_rows(T.STEP_N, T.STEP_N, T.STEP_H, False):
            assert ref.ref["L"][h, r] > R.SPIKE_L[i]
            local = j - 40                                                   # its place in the long shard of `two` and `three`
            assert local // tile >= 1 and (local // (4 * tile) + 2) * 4 * tile <= 1036 or i == 1      # a round start behind the 28-unit key
            assert i == 0 or 1 <= local // tile < (1036 // (4 * tile)) * 4      # the 130-unit key: a whole round, not its first tile
        lift = T.dense_step("lift", d, "two").rows().ref["L"]
        assert lift.max() < 45 and all(lift[h, r] > R.SPIKE_L[0] for h, r, j, i in R.spike_rows(T.STEP_N, T.STEP_N, T.STEP_H, False, (0,)))
        assert (T.dense_step("low-level", d, "two").rows().ref["L"] < R.LOW_LEVEL_L).all()
        for n in range(1, 3):                                                # and over the keys seen so far, whichever they are
            assert (T.dense_step("low-level", d, "thirds").rows_of({n}).ref["L"] < R.LOW_LEVEL_L).all()
    assert 40 < 64 and 1100 - 1076 < 64 and 1060 % 64 and 1060 % 128         # a shard shorter than a tile; a ragged tail


# ------------------------------------------------------------------------------------------------ teeth
def _tensor_gate(got, ref):
    fin = np.isfinite(ref.ref["L"])
    with np.errstate(invalid="ignore"):
        e = np.abs(got["L"] - ref.ref["L"])
    near = np.abs(ref.ref["L"]) <= B.L_NEAR
    rel = R.rel(got["O"], ref.ref["O"]) if np.isfinite(got["O"]).all() else np.inf
    ok = rel <= B.BF16_REL and bool((e[fin & near] <= B.L_ABS).all() and (e[fin & ~near] <= B.L_ABS_FAR).all()) and np.array_equal(np.isfinite(got["L"]), fin)
    return rel, float(np.nan_to_num(e[fin], nan=np.inf).max(initial=0.0)), ok


def _bites(what, step, order, fault, off):
    got, _, touched = step.emulate(order, off, fault)
    ref = step.rows_of(order)
    assert touched.any(), what
    rat = B.ratios(got, ref)
    worst = np.maximum(np.nan_to_num(rat["O"], nan=np.inf), np.nan_to_num(rat["L"], nan=np.inf))
    assert worst[~touched].max(initial=0.0) <= 1.0, (what, "a row outside the fault fails")
    assert worst[touched].max() >= BITE, (what, float(worst[touched].max()))
    with pytest.raises(AssertionError):
        B.check(what, got, ref)
    rel, dl, ok = _tensor_gate(got, ref)
    print(f"TEETH {what} -{off:g}: {worst[touched].max():.3g} x the row gate on {int(touched.sum())} rows; the tensor gate " +
          ("PASSES" if ok else "fails") + f" it: O {rel:.2e} max|dL| {min(dl, 1e30):.2e}")
    assert ok == (what.split()[0] in PASSED_BY_THE_TENSOR_GATE), (what, rel, dl)


@pytest.mark.parametrize("off", B.FWD_OFFSETS)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
def test_step_mutants_break_a_row_gate(d, off):
    dense = T.dense_step("scale-one", d, "thirds")
    _bites(f"s1 d{d}", dense, (0, 1, 2), ("s1", 1), off)
    _bites(f"s2 d{d}", dense, (0, 1, 2), ("s2", 1, 2), off)
    _bites(f"s6 d{d}", dense, (0, 1, 2), ("s6", 1, 20, 800), off)
    strided = T.strided_step("scale-one", d, T.STRIDED_SHIFTS[0])
    _bites(f"s3 d{d}", strided, (0, 1), ("s3",), off)
    _bites(f"s5 d{d}", strided, (0, 1), ("s5",), off)
    _bites(f"s4 d{d}", T.strided_step("scale-one", d, T.STRIDED_SHIFTS[1]), (0, 1), ("s4", 1, 10), off)
