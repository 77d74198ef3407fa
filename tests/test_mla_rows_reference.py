"""CPU: what the row gates of the MLA decode rest on (tests/mla_ref.py; the gate itself is tests/decode_rows_ref.py's, unchanged).

(i) THE CERTIFICATE.  mla_ref.emulate -- the MLA kernel's own data flow: the waves split the columns and their partial S meet
in fp32, one online softmax per split, splits on multiples of 32 -- uses at most ROOM = 0.75 of the O row gate at the family's
KAPPA, of decode_ref's L gates and of the keyless-row rule on every row of everything tests/test_gpu_mla_rows.py and
tests/test_gpu_mla_decode.py hand a kernel: the uniform inputs at (H, N_q) = (16, 1), (16, 2), (5, 3), (40, 1), (11, 3), (2, 17),
(128, 1) and the (1, 1) pair of the cache past 4 GiB (that one at its default of 26 too), both masks, at 1, 2 and 5 splits (5 is the largest explicit count and leaves
an empty split even on the longest sequence; n_splits = 0 is 1 on these shapes); the four regimes at (11, 3), both masks, at 1 and
7 splits (7 leaves the 300-key sequence two empty splits) and at what n_splits = 0 stands for.  Nothing here is a new tolerance.
`low-level` keeps its offset in the rotary columns: spread over all 576 columns V = K[:, :512] is near-constant, every element
of O rounds the same way and the emulation uses 0.99 to 1.05 of the gate (mla_ref's docstring) -- the input was changed, not the gate.
(ii) THE REGIMES, from the reference alone: a row that sees its spike has L above regimes.SPIKE_L, every finite `low-level` L
lies below regimes.LOW_LEVEL_L.
(iii) THE MUTANTS a1 .. a5 of mla_ref: each fails the row gate (a1: the L gate) on every row it touches and holds on every other.
THE GAP THAT IS CLOSED: on all four shapes tests/test_gpu_mla_decode.py runs, a3 -- the causal kmax from the row WITHIN the
32-row block -- changes NO BIT of the emulation's output: (16, 1), (16, 2) and (5, 3) have one row block, and (40, 1) has
q_len = 1, where % 1 is 0 either way.  A kernel with that fault passed every test the project had.  On (11, 3), causal, it fails:
row 32 is head 10's token 2 and a3 takes it for token 0, so the row loses its last two keys.  On the uniform inputs the row gate
fails on 5 of the 9 touched rows (up to 205 x) and the row gate or the L gate on all 9: where the two keys weigh less than the
bf16 rounding of P no gate on O can see them.  Under `scale-one` and `low-level` the row gate fails on every touched row.
(iv) THE FORMULA by hand: one visible key gives O = C[0, :512], a gate of (KAPPA + 1) u |v| and L = S exactly; a keyless row has
gate 0."""
import numpy as np
import pytest
import torch

import decode_ref as dr
import decode_rows_ref as rows
import mla_ref as mr
import regimes

GROUPS = ("uniform", "regimes")
TOP = {g: [] for g in GROUPS}
MASKS = ((True, "causal"), (False, "full"))


def _certify(group, label, O, L, ref):
    e = dr.errors(O, L, ref)
    top = float(rows.ratios(O, ref).max(initial=0.0))
    ltop = float(mr.l_ratios(L, ref).max(initial=0.0))
    print(f"ROWS-CPU mla {group} {label}: row ratio {top:.3f}  L ratio {ltop:.3f}  dL {e[1]:.2e}  dL(|L| > 25) {e[2]:.2e}")
    assert top <= rows.ROOM, (group, label, top)
    assert e[1] <= rows.ROOM * dr.L_ABS and e[2] <= rows.ROOM * dr.L_ABS_LARGE and e[3], (group, label, e)
    TOP[group].append(top)
    return top


# ------------------------------------------------------------------------------------------------ (i)
def test_the_inputs_are_the_existing_files():
    """mla_ref's uniform inputs, lengths, shapes, scale and reference are tests/test_gpu_mla_decode.py's, and its append model is
    tests/test_gpu_mla_append.py's."""
    import qk_norm_ref as nr
    import rope_ref as rr
    import test_gpu_mla_append as ta
    import test_gpu_mla_decode as td

    assert (td.LENS, td.SHAPES, td.SPLITS, td.N_CAP, td.SCALE) == (mr.UNIFORM_LENS, mr.OLD_SHAPES, mr.UNIFORM_SPLITS, mr.UNIFORM_CAP, mr.UNIFORM_SCALE)
    for H, nq in ((5, 3), (40, 1)):
        for a, b in zip(td._inputs(H, nq), mr.uniform_inputs(H, nq)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        old, new = td._reference(H, nq, True), mr.uniform_reference(H, nq, True)
        np.testing.assert_allclose(new[0], old[0], rtol=0, atol=1e-13)
        np.testing.assert_allclose(new[1], old[1], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(new.quad, old.quad)
    H, n_new, lens = 5, 2, ta._lens(2)
    host = ta._sources(len(lens), H, n_new, 3)
    w, (cos, sin) = nr.weights(512, nr.WEIGHT_SEED)[1], rr.random_tables(ta.CAP, 64, 9)
    for table in (None, ta._table(len(lens), bad=True)):
        shape = (len(lens), ta.CAP, 576) if table is None else (len(lens) * (ta.CAP // ta.P) + 3, ta.P, 576)
        a, b = (torch.full(shape, ta.SENTINEL, dtype=torch.bfloat16) for _ in range(2))
        qa = ta._model(a, table, ta._views(*host, H), lens, w, cos, sin, True)
        qb = mr.append_model(b, table, ta._views(*host, H), lens, w, cos, sin, True)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(qa.view(torch.int16), qb.view(torch.int16))
        assert (a != ta.SENTINEL).any()


@pytest.mark.parametrize("H,nq", mr.OLD_SHAPES + mr.NEW_SHAPES)
def test_certificate_uniform(H, nq):
    Q, C = mr.uniform_inputs(H, nq)
    assert mr.num_splits(len(mr.UNIFORM_LENS), H, nq, mr.UNIFORM_CAP) == 1
    assert mr.split_range(mr.UNIFORM_CAP, 5, 4) == (384, 384)      # 5 splits: the fifth is empty on the longest sequence too
    for causal, name in MASKS:
        for n_splits in (1, 2, 5):
            O, L = mr.emulate(Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, causal, n_splits)
            _certify("uniform", f"H {H} nq {nq} {name} splits {n_splits}", O, L, mr.uniform_reference(H, nq, causal))


def test_certificate_past_4_gib():
    Q, C = mr.far_inputs()
    default = mr.num_splits(mr.FAR_B, *mr.FAR_SHAPE, mr.FAR_CAP)
    assert Q.shape[1:3] == mr.FAR_SHAPE and default == 26      # what n_splits = 0 stands for there: 300 keys fill 10 of the 26
    for causal, name in MASKS:
        for n_splits in (1, 2, 5, default):
            O, L = mr.emulate(Q, C, mr.FAR_LENS, mr.UNIFORM_SCALE, causal, n_splits)
            _certify("uniform", f"far {name} splits {n_splits}", O, L, mr.far_reference(causal))


@pytest.mark.parametrize("regime", mr.REGIMES)
def test_certificate_regimes(regime):
    Q, C, scale, lens = mr.regime_inputs(regime)
    default = mr.num_splits(len(mr.LENS), mr.H, mr.NQ, mr.N_CAP)
    assert default == 4 and mr.split_range(300, 7, 5) == (320, 300)      # 7 splits: the short sequence's last two are empty
    for causal, name in MASKS:
        ref = mr.regime_reference(regime, causal)
        for n_splits in (1, 7, default):
            _certify("regimes", f"{regime} {name} splits {n_splits}", *mr.emulate(Q, C, lens.tolist(), scale, causal, n_splits), ref)
        # (ii) the regimes, from the reference alone
        rL = ref[1]
        assert np.isfinite(rL).all()
        if regime == "spikes":
            seen = mr.spike_rows(causal)
            assert {i for _, i in seen} == {0, 1} and len(seen) == 4
            for index, i in seen:
                assert rL[index] > regimes.SPIKE_L[i], (regime, name, index, rL[index])
        if regime == "low-level":
            print(f"ROWS-CPU mla low-level {name}: largest L {rL.max():.1f}")
            assert (rL < regimes.LOW_LEVEL_L).all(), (name, rL.max())


def test_the_largest_ratios():
    """Over what ran before this test: the largest row ratio per group (DESIGN.md section 6d quotes them)."""
    for g in GROUPS:
        print(f"ROWS-CPU mla largest row ratio, {g}: {max(TOP[g], default=0.0):.3f} over {len(TOP[g])} emulated calls")
        assert max(TOP[g], default=0.0) <= rows.ROOM
    assert (rows.KAPPA, rows.ROOM, dr.L_ABS, dr.L_ABS_LARGE) == (1.5, 0.75, 1e-4, 1e-3)      # the family's, unchanged


# ------------------------------------------------------------------------------------------------ (iii)
def _touched(shape, index):
    t = np.zeros(shape, dtype=bool)
    t[index] = True
    return t


def _fails_exactly(label, O, L, ref, touched, l_untouched=True):
    """The row gate fails on every touched row and holds (inside ROOM) on every other; L stays inside its gates if `l_untouched`."""
    r = rows.ratios(O, ref)
    print(f"ROWS-MUTANT mla {label}: touched rows {r[touched].min():.2f} .. {r[touched].max():.2f} x gate, the others at most "
          f"{r[~touched].max(initial=0.0):.2f}")
    assert touched.any() and (r[touched] > 1.0).all(), (label, float(r[touched].min()))
    assert (r[~touched] <= rows.ROOM).all(), label
    lr = mr.l_ratios(L, ref)
    assert (lr[~touched] <= rows.ROOM).all(), label
    if l_untouched:
        assert (lr <= rows.ROOM).all(), label


H3, NQ3 = mr.NEW_SHAPES[0]


@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
@pytest.mark.parametrize("n_splits", (1, 5))
def test_a1_fails_the_l_gate_and_a2_the_row_gate(n_splits, causal):
    Q, C = mr.uniform_inputs(H3, NQ3)
    ref = mr.uniform_reference(H3, NQ3, causal)
    args = (Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, causal, n_splits)
    O0, L0 = mr.emulate(*args)
    O, L, b = mr.a1_no_rotary_columns(*args)
    touched = _touched(L0.shape, b)
    lr = mr.l_ratios(L, ref)
    print(f"ROWS-MUTANT mla a1 splits {n_splits}: L of the touched rows {lr[touched].min():.1f} .. {lr[touched].max():.1f} x gate")
    assert mr.UNIFORM_LENS[b] == mr.UNIFORM_CAP and (lr[touched] > 1.0).all() and (lr[~touched] <= rows.ROOM).all()
    assert np.array_equal(O[~touched], O0[~touched]) and np.array_equal(L[~touched], L0[~touched])
    O, L, b = mr.a2_neighbours_columns(*args)
    assert np.array_equal(L, L0)      # the second product alone
    _fails_exactly(f"a2 splits {n_splits}", O, L, ref, _touched(L0.shape, b))


@pytest.mark.parametrize("n_splits", (1, 5))
def test_a3_changes_no_bit_on_the_old_shapes_and_fails_on_11_3(n_splits):
    for H, nq in mr.OLD_SHAPES:      # THE GAP: one row block, or q_len = 1
        Q, C = mr.uniform_inputs(H, nq)
        args = (Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, True, n_splits)
        for got, want in zip(mr.a3_row_within_the_block(*args), mr.emulate(*args)):
            assert np.array_equal(got, want, equal_nan=True), (H, nq)
        assert not mr.a3_touched(H, nq, mr.UNIFORM_LENS).any()
    Q, C = mr.uniform_inputs(H3, NQ3)
    touched = mr.a3_touched(H3, NQ3, mr.UNIFORM_LENS)
    assert touched.sum() == len(mr.UNIFORM_LENS) - 1 and touched[1:, H3 - 1, NQ3 - 1].all()      # row 32 of every sequence with a key
    O, L = mr.a3_row_within_the_block(Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, True, n_splits)
    ref = mr.uniform_reference(H3, NQ3, True)
    r, lr = rows.ratios(O, ref), mr.l_ratios(L, ref)
    print(f"ROWS-MUTANT mla a3 (11, 3) causal splits {n_splits}: touched rows O {np.round(r[touched], 2)} L {np.round(lr[touched], 1)} x gate, "
          f"the others at most {r[~touched].max():.2f} and {lr[~touched].max():.2f}")
    # a touched row loses its last two keys.  What they weigh is the data's (scores of standard deviation 2): where it is more
    # than the bf16 rounding of P the row gate fails, and on EVERY touched row the row gate or the L gate does -- the GPU file
    # applies both to every row.  With one key the row is keyless under a3: O = 0 against C[0, :512]
    assert (np.maximum(r, lr)[touched] > 1.0).all() and (r[touched] > 1.0).any() and r[1, H3 - 1, NQ3 - 1] > 1.0 / (rows.KAPPA + 1.0) / rows.U / 2
    assert (r[~touched] <= rows.ROOM).all() and (lr[~touched] <= rows.ROOM).all()
    for H, nq in mr.NEW_SHAPES[1:]:      # (2, 17) is touched too; (128, 1) is not: the four blocks are for the row mapping
        assert mr.a3_touched(H, nq, mr.UNIFORM_LENS).any() == (nq > 1)
    # without the mask there is no kmax to get wrong
    for got, want in zip(mr.a3_row_within_the_block(Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, False, n_splits),
                         mr.emulate(Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, False, n_splits)):
        assert np.array_equal(got, want)


def test_a3_on_the_regimes():
    """Row 32 of both sequences loses its last two keys: under `scale-one` and `low-level` the row gate fails on both.  (Row 32 is
    the row of the 130-unit spike, and under `peaked` a handful of keys hold a row's weight: there the two lost keys weigh nothing,
    which is those regimes' point -- the mask on that row is held by the other two and by the uniform inputs.)"""
    for regime in ("scale-one", "low-level"):
        Q, C, scale, lens = mr.regime_inputs(regime)
        O, L = mr.a3_row_within_the_block(Q, C, lens.tolist(), scale, True, 7)
        _fails_exactly(f"a3 {regime}", O, L, mr.regime_reference(regime, True), mr.a3_touched(mr.H, mr.NQ, mr.LENS), l_untouched=False)


@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
def test_a4_a_middle_splits_tile(causal):
    Q, C = mr.uniform_inputs(H3, NQ3)
    args = (Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, causal, 5)
    O, L, b, t0 = mr.a4_middle_split_tile(*args)
    assert (mr.UNIFORM_LENS[b], t0) == (384, 256)      # splits of 96 keys: split 2 is [192, 288), its last tile [256, 288)
    assert np.array_equal(L, mr.emulate(*args)[1])
    _fails_exactly("a4 uniform", O, L, mr.uniform_reference(H3, NQ3, causal), _touched(L.shape, b))
    Q, C, scale, lens = mr.regime_inputs("scale-one")
    O, L, b, t0 = mr.a4_middle_split_tile(Q, C, lens.tolist(), scale, causal, 7)
    assert (mr.LENS[b], t0) == (1100, 608)             # splits of 160 keys: split 3 is [480, 640)
    _fails_exactly("a4 scale-one", O, L, mr.regime_reference("scale-one", causal), _touched(L.shape, b))


def test_a5_an_empty_split_read_as_zero():
    """Under `low-level` (every L below -105) the weight exp(0 - m) of the empty split is all there is: O = 0 and L = log(2), and
    both gates fail on every row of the sequence with an empty split.  On the uniform inputs (L about 8 at 384 keys) the same
    fault moves O by exp(-L) of itself: the row gate PASSES it on every row of the longest sequence (asserted: the L gate alone
    sees it there, at 1.3 to 3.4 times its limit) -- it takes the regime for the row gate to see it."""
    Q, C, scale, lens = mr.regime_inputs("low-level")
    ref = mr.regime_reference("low-level", True)
    O, L, seqs = mr.a5_empty_split_read_as_zero(Q, C, lens.tolist(), scale, True, 7)
    assert seqs == [0]                                  # 300 keys in 7 splits of 64: splits 5 and 6 are empty; 1100 keys fill all 7
    touched = _touched(L.shape, seqs)
    _fails_exactly("a5 low-level", O, L, ref, touched, l_untouched=False)
    assert (mr.l_ratios(L, ref)[touched] > 1.0).all()
    Q, C = mr.uniform_inputs(H3, NQ3)
    ref = mr.uniform_reference(H3, NQ3, True)
    O, L, seqs = mr.a5_empty_split_read_as_zero(Q, C, mr.UNIFORM_LENS, mr.UNIFORM_SCALE, True, 5)
    assert seqs == [1, 2, 3, 4, 5, 6, 9]                # lengths 1 .. 128 and 384 (splits of 96: the fifth is empty); 129 and 300 fill all five
    r, lr = rows.ratios(O, ref), mr.l_ratios(L, ref)
    print(f"ROWS-MUTANT mla a5 uniform, the longest sequence: O rows {r[-1].min():.2f} .. {r[-1].max():.2f} x gate, L rows {lr[-1].min():.1f} .. {lr[-1].max():.1f} x gate")
    assert (r[-1] <= 1.0).all() and (lr[-1] > 1.0).all()


# ------------------------------------------------------------------------------------------------ (iv)
def test_the_formula_by_hand():
    g = torch.Generator().manual_seed(7)
    Q = (torch.rand(2, 1, 1, mr.D, generator=g) - 0.5).bfloat16()
    C = (torch.rand(2, 4, mr.D, generator=g) - 0.5).bfloat16()
    scale = 0.125
    ref = mr.reference64(Q, C, [1, 0], scale, True)
    v = C[0, 0, :mr.DV].double().numpy()
    np.testing.assert_array_equal(ref[0][0, 0, 0], v)                                              # one visible key: P = 1, O = C[0, :512]
    assert ref[1][0, 0, 0] == scale * float(Q[0, 0, 0].double() @ C[0, 0].double())                # L = S exactly
    np.testing.assert_allclose(rows.gate(ref)[0, 0, 0], (rows.KAPPA + 1.0) * 2.0 ** -9 * np.linalg.norm(v), rtol=1e-14)
    assert rows.gate(ref)[1, 0, 0] == 0.0 and np.isneginf(ref[1][1, 0, 0]) and (ref[0][1] == 0).all()      # no key: gate 0, O exactly 0
    O, L = mr.emulate(Q, C, [1, 0], scale, True, 1)
    np.testing.assert_array_equal(O[0, 0, 0], v)
    assert abs(L[0, 0, 0] - ref[1][0, 0, 0]) < 1e-6 and np.isneginf(L[1, 0, 0]) and (O[1] == 0).all()
    O64 = ref[0].copy()
    assert rows.ratios(O64, ref).max() == 0.0
    O64[1, 0, 0, 5] = 1e-30
    assert np.isinf(rows.ratios(O64, ref)[1, 0, 0])
    # the lengths are clamped to [0, capacity] as the kernel clamps them
    for got, want in zip(mr.emulate(Q, C, [-5, 9], scale, True, 2), mr.emulate(Q, C, [0, 4], scale, True, 2)):
        assert np.array_equal(got, want)
