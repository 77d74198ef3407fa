"""CPU: the row gates, the emulation and the mutants of tests/bf16_rows_ref.py, certified before a bf16 kernel sees them.

KAPPA = 2.5 (bf16_rows_ref.KAPPA; the bound is 4).
ROOM.  On every case tests/test_gpu_bf16_rows.py hands a kernel (bf16_rows_ref.cpu_cases()), the emulation -- the forward at
the references 0 and 6 below the row maximum, the backward as regimes.emulate with bf16 outputs, and with bf16 per-head
partials where a grouped problem runs the single kernel -- uses at most ROOM = 0.75 of every row gate, and its L is the
reference's.  KAPPA is the smallest multiple of 0.5 at which that holds: at 2.0 `scale-one` dV reaches 0.86 (N = 1025, d = 64,
causal: test_kappa_is_the_smallest_that_leaves_room).  Largest ratios at KAPPA, O / dQ / dK / dV:
    scale-one 0.52 / 0.64 / 0.64 / 0.74    scale-small 0.50 / 0.63 / 0.62 / 0.64    peaked 0.53 / 0.66 / 0.69 / 0.69
    spikes 0.52 / 0.65 / 0.56 / 0.50       lift 0.52 / 0.67 / 0.51 / 0.50           low-level 0.48 / -- / -- / 0.55
    offsets -- / 0.61 / 0.59 / --
NOT ROW-GATED, and why (bf16_rows_ref.TENSOR_GATED; they keep the suite's tensor gates):
  * `low-level` dQ and dK: Q and K are nearly collinear, so the summed rounding error of dS K is a scalar with Gaussian tails and not
    a 2-norm over d: 1.50 (dQ; N = 1100, d = 128, full) and 1.55 (dK; N = 1024, d = 64, full) of the gate at kappa = 2.5, 0.95 and
    0.98 at kappa = 4.
  * `offsets` O and dV: every component of O is about 0.5 (the mean of V) and of dV about 0.1 sum_i P_ij -- just above a power of
    two, where bf16's spacing is widest relative to the value.  The output rounding alone is 2^-8 / sqrt(12) per component, about
    0.9 u |O_i| with u = 2^-9, and it does not shrink with kappa: 0.97 (O) and 0.91 (dV) of the gate at kappa = 2.5, 0.89 and
    0.81 at kappa = 4 (N = 1024 and 1100, d = 64, full).  The gate is not widened for it; the regime stays row-gated on L, dQ and dK.
TEETH.  Every mutant m1 .. m10 breaks a row gate by at least 1.5 on at least one row on every case it is run on (the figures are
printed; DESIGN.md section 6c keeps them).  A mutant is run where the tensor it touches is row-gated.
THE TENSOR GATE MISSES THEM.  m3 stays under rel-L2 5e-3 (`low-level` dQ: 0.15) on dQ, dK and dV on the four cases of the
issue's table; m8 on the row before a spike row of `spikes` at 1100 keys (it takes the spike row's D) stays
under it on dQ and dK, 282 times the dQ row gate.
NO ZERO GATES.  Every gate is positive and finite on every row with a visible key (asserted with ROOM)."""
import numpy as np
import pytest

import bf16_rows_ref as B
import regimes as R

CASES = {label: (build, args) for label, build, args in B.cpu_cases()}


def _case(label):
    build, args = CASES[label]
    return build(*args)


def _largest(rat):
    return {n: float(r.max(initial=0.0)) for n, r in rat.items()}


def _runs_partials(case):
    return case.G > 1 and not isinstance(case, B.Packed) and case.nq == case.nk and B.single_kernel(case.nq, case.d)


def _emulations(case):
    """(what, partials, outputs) of every emulated route of a case."""
    out = [(f"forward -{off:g}", False, case.emulate_forward(off)) for off in B.FWD_OFFSETS]
    out.append(("backward", False, case.emulate_backward()))
    if _runs_partials(case):
        out.append(("backward, bf16 partials", True, case.emulate_backward(True)))
    return out


# ------------------------------------------------------------------------------------------------ room, and no zero gates
def test_kappa_and_phi_are_within_their_bounds():
    assert B.KAPPA <= 4.0 and B.KAPPA % 0.5 == 0.0 and B.PHI <= 2.0 ** -18 and B.U == 2.0 ** -9 and B.ROOM == 0.75


@pytest.mark.parametrize("label", list(CASES))
def test_every_gpu_case_leaves_the_kernels_room(label):
    case = _case(label)
    none, worst = np.isneginf(case.ref["L"]), {}
    for name in ("O",) + B.GRADS:
        for partials in (False, True):
            gate = case.gate(name, partials)
            has_key = ~none if name in ("O", "dQ") else case.key_seen
            assert np.isfinite(gate).all() and (gate[has_key] > 0).all(), (label, name, "a zero or infinite gate")
    for what, partials, got in _emulations(case):
        for name, m in _largest(B.ratios(got, case, partials)).items():
            assert m <= (1e-6 if name == "L" else B.ROOM), (label, what, name, m)
            worst[name] = max(worst.get(name, 0.0), m)
    print(f"ROOM {label} ({case.regime}): " + " ".join(f"{n} {m:.3f}" for n, m in worst.items() if n != "L"))


def test_kappa_is_the_smallest_that_leaves_room():
    """One step lower the emulation passes 0.75 of a gate: KAPPA is the smallest multiple of 0.5 that leaves room."""
    case = _case("edges scale-one N1025 d64 causal")
    at = lambda kappa: float(B.ratios(case.emulate_backward(), case, kappa=kappa)["dV"].max())
    assert at(B.KAPPA - 0.5) > B.ROOM >= at(B.KAPPA)


def test_what_is_not_row_gated_and_why():
    """The two exemptions miss 0.75 at kappa = 4 as well: no admissible kappa would have kept them."""
    for label, names in (("regimes low-level N1100 d128 full", ("dQ",)), ("regimes offsets N1024 d64 full", ("O", "dV"))):
        case = _case(label)
        assert set(names) <= set(B.TENSOR_GATED[case.regime])
        got = dict(case.emulate_forward(0.0), **case.emulate_backward())
        for name in names:
            gate = case.gate(name, kappa=4.0)
            r = float((B.row_errors(got, case)[name] / gate).max())
            print(f"EXEMPT {label} {name}: {r:.2f} of the gate at kappa = 4")
            assert r > B.ROOM, (label, name, r)


def test_rows_and_keys_without_a_partner_are_gated_exactly():
    """(1100, 300) causal: rows 0 .. 799 see no key -- O = 0, L = -inf, dQ = 0 or an infinite error; the packed batch's
    sequence without queries: dK = dV = 0 or an infinite error."""
    case = B.dense_case("scale-one", 8, 2, 1100, 300, 64, True)
    assert np.isneginf(case.ref["L"][:, :800]).all() and np.isfinite(case.ref["L"][:, 800:]).all()
    got = dict(case.emulate_forward(0.0), **case.emulate_backward())
    assert max(_largest(B.ratios(got, case)).values()) <= B.ROOM
    for name, value in (("O", 1e-30), ("dQ", 1e-30), ("L", -1e30)):
        bad = {n: x.copy() for n, x in got.items()}
        bad[name][3, 17] = value
        assert np.isinf(B.ratios(bad, case)[name][3, 17])
        with pytest.raises(AssertionError, match=rf"{name} row gate missed at \(h 3, row 17\)"):
            B.check("empty rows", bad, case)
    packed = B.packed_case("scale-one", B.PACKED, 64, False)
    assert not packed.key_seen[:, -40:].any() and packed.key_seen[:, :-40].all()
    got = packed.emulate_backward()
    assert (got["dK"][:, -40:] == 0).all() and max(_largest(B.ratios(got, packed)).values()) <= B.ROOM
    got["dV"][1, -1, 5] = 1e-30
    assert np.isinf(B.ratios(got, packed)["dV"][1, -1])


def test_grouped_partials_widen_dk_and_dv_only():
    case = _case("gqa scale-one N1100 d128 full")
    assert _runs_partials(case) and not _runs_partials(_case("gqa scale-one N1100 d64 full"))
    for name in ("dK", "dV"):
        extra = case.gate(name, True) - case.gate(name)
        assert (extra > 0).all() and (extra < 8 * B.U * np.linalg.norm(case.ref[name], axis=-1).max() * 8).all()
    assert all(np.array_equal(case.gate(n, True), case.gate(n)) for n in ("O", "dQ", "L"))


# ------------------------------------------------------------------------------------------------ teeth
#          label                       regime       d    N     32-row group, 256-key block, row of m8
TEETH = {"scale-one-128-1100": ("scale-one", 128, 1100, 20, 1, 700), "offsets-64-600": ("offsets", 64, 600, 12, 0, 400),
         "spikes-128-1100": ("spikes", 128, 1100, 20, 1, 1058), "low-level-128-600": ("low-level", 128, 600, 12, 0, 400)}
HEAD, TEETH_H, BITE = 1, 3, 1.5


def _teeth(label, causal=True):
    regime, d, n, group, block, row = TEETH[label]
    return B.dense_case(regime, TEETH_H, TEETH_H, n, n, d, causal), group, block, row


def _bites(what, label, case, got, where=None):
    """The mutant's largest ratio per row-gated tensor; asserts one of at least BITE (where = (tensor, head, rows): there)."""
    rat = B.ratios(got, case)
    best = max(rat, key=lambda n: rat[n].max())
    print(f"TEETH {what} {label}: " + " ".join(f"{n} {r.max():.1f}" for n, r in rat.items()))
    assert rat[best].max() >= BITE, (what, label, _largest(rat))
    if where is not None:
        name, head, rows = where
        assert rat[name][head, rows].max() >= BITE, (what, label, name, float(rat[name][head, rows].max()))
        others = rat[name].copy()
        others[head, rows] = 0.0
        assert others.max() <= 1.0, (what, label, name, "a row outside the fault fails")
    with pytest.raises(AssertionError):                                      # the GPU file's verdict on the same arrays
        B.check(f"{what} {label}", got, case)
    return _largest(rat)


def _applies(case, *names):
    return all(B.row_gated(case, n) for n in names)


@pytest.mark.parametrize("off", B.FWD_OFFSETS)
@pytest.mark.parametrize("label", list(TEETH))
def test_forward_mutants_break_a_row_gate(label, off):
    case, group, block, _ = _teeth(label)
    rows = slice(32 * group, 32 * group + 32)
    if _applies(case, "O"):                                                  # m1 moves O alone
        got = B.m1_key_block_missing_from_pv(case, off, HEAD, group, 64)
        assert _bites("m1", label, case, got, ("O", HEAD, rows))["L"] <= 1e-6
    _bites("m2", label, case, B.m2_mask_shifted_forward(case, off, HEAD, group), ("L", HEAD, rows))


@pytest.mark.parametrize("label", list(TEETH))
def test_backward_mutants_break_a_row_gate(label):
    case, group, block, row = _teeth(label)
    rows, keys = slice(32 * group, 32 * group + 32), slice(256 * block, 256 * block + 256)
    _bites("m3", label, case, B.m3_mask_shifted_backward(case, HEAD, group))
    if _applies(case, "dQ"):
        _bites("m6", label, case, B.m6_handoff_lost(case, HEAD, group, block), ("dQ", HEAD, rows))
        if case.d == 64:
            _bites("m10", label, case, B.m10_key_half_left_out(case, HEAD, group, 128), ("dQ", HEAD, rows))
    _bites("m7", label, case, B.m7_subtile_missing_from_dkdv(case, HEAD, group, block),
           ("dK" if _applies(case, "dK") else "dV", HEAD, keys))
    if _applies(case, "dQ"):
        _bites("m8", label, case, B.m8_neighbours_d(case, HEAD, row), ("dQ", HEAD, slice(row, row + 1)))


@pytest.mark.parametrize("causal", B.MASKS)
@pytest.mark.parametrize("label", list(TEETH))
def test_mutants_of_both_passes_break_a_row_gate(label, causal):
    case, group, block, _ = _teeth(label, causal)
    for off in B.FWD_OFFSETS:
        _bites("m4", label, case, B.m4_other_mask(case, off, HEAD, group))
        _bites("m5", label, case, B.m5_heads_swapped(case, off, (0, 2), 1))
        if not causal:
            _bites("m9", label, case, B.m9_next_heads_keys(case, off, HEAD))


def test_check_names_the_tensor_the_head_and_the_group():
    case, group, block, _ = _teeth("scale-one-128-1100")
    with pytest.raises(AssertionError, match=rf"dQ row gate missed at \(h {HEAD}, row 6[4-7]\d\).*h{HEAD}: \d+ rows, per 32-row group {group}:\d+$"):
        B.check("m6", B.m6_handoff_lost(case, HEAD, group, block), case)
    with pytest.raises(AssertionError, match=rf"O row gate missed at \(b 0, h {HEAD}, row .*b0 h{HEAD}: 32 rows, per 32-row group {group}:32$"):
        B.check("m1", B.m1_key_block_missing_from_pv(case, 0.0, HEAD, group, 64), case, heads=TEETH_H)
    nan = case.emulate_forward(0.0)
    nan["O"][2, 5, 3] = np.nan
    with pytest.raises(AssertionError, match="NaN left in O"):
        B.check("nan", nan, case)


# ------------------------------------------------------------------------------------------------ why the file exists
@pytest.mark.parametrize("label", list(TEETH))
def test_the_tensor_gate_misses_a_shifted_mask(label):
    case, group, _, _ = _teeth(label)
    got = B.m3_mask_shifted_backward(case, HEAD, group)
    rel = {n: R.rel(got[n], case.ref[n]) for n in B.GRADS}
    print(f"TENSOR m3 {label}: " + " ".join(f"{n} {e:.2e}" for n, e in rel.items()))
    assert all(e <= B.TENSOR_GATED.get(case.regime, {}).get(n, B.BF16_REL) for n, e in rel.items()), rel


def test_the_tensor_gate_misses_a_neighbours_d_on_dq():
    case, _, _, row = _teeth("spikes-128-1100")
    assert (HEAD, row + 1) in {(h, r) for h, r, *_ in R.spike_rows(1100, 1100, TEETH_H, True)}      # the neighbour sits on a spike
    got = B.m8_neighbours_d(case, HEAD, row)
    rel = {n: R.rel(got[n], case.ref[n]) for n in B.GRADS}
    print("TENSOR m8 spikes-128-1100: " + " ".join(f"{n} {e:.2e}" for n, e in rel.items()))
    assert rel["dQ"] <= B.BF16_REL


# ------------------------------------------------------------------------------------------------ the pieces
def test_the_forward_flow_is_the_reference_up_to_its_roundings():
    """Without the two bf16 roundings nothing is left: forward_flow at either offset is ref_attention (L to 1e-12 as it stands)."""
    case = B.dense_case("peaked", 2, 2, 257, 257, 64, True)
    for off in B.FWD_OFFSETS:
        got = case.emulate_forward(off)
        assert np.abs(got["L"] - case.ref["L"]).max() <= 1e-12
        assert R.rel(got["O"], case.ref["O"]) <= 3e-3


def test_the_backward_blocks_add_up():
    """What the mutants rest on: regimes.emulate on the two halves of a row group's keys adds up to the whole."""
    case = B.dense_case("scale-one", 2, 2, 257, 257, 64, False)
    rows = slice(64, 96)
    whole = B._block(case, 1, rows, slice(0, 257), False)
    a, b = B._block(case, 1, rows, slice(0, 100), False), B._block(case, 1, rows, slice(100, 257), False)
    assert np.abs(whole[0] - (a[0] + b[0])).max() <= 1e-12
    for i in (1, 2):
        assert np.abs(whole[i] - np.concatenate([a[i], b[i]])).max() == 0.0
    shifted = B._block(case, 1, rows, slice(0, 97), True)[0]               # the causal mask moved by one key
    S = np.where(B.visible(257, 257, True, 1)[rows, :97], 0.0, -np.inf)
    assert np.isfinite(S[0, :66]).all() and np.isneginf(S[0, 66:]).all() and np.isfinite(shifted).all()


def test_the_routing_rule_is_the_headers():
    ones = lambda d: [n for n in range(1, 1300) if B.single_kernel(n, d)]
    span = lambda a, b: list(range(a, b + 1))
    assert ones(128) == span(129, 256) + span(321, 1299)
    assert ones(64) == span(193, 256) + span(449, 512) + span(705, 768) + span(897, 1024) + span(1153, 1280)
