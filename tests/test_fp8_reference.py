"""CPU: the inputs, the reference and the per-row gate of tests/fp8_ref.py, certified before the fp8 kernel sees them.

ROOM.  For every (regime, N) that tests/test_gpu_fp8_rows.py hands the kernel, one head, both masks: emulate() -- the kernel's
data flow, P rounded to e4m3, at the references row maximum - 0, 1.5, 3, 4.5, 6 -- stays within ROOM = 0.75 of the gate on every
row, and its L is the reference's.  A condition on the INPUTS: a case that breaks it is changed, the factor is not.
Measured (largest |O_emu - O_ref| / gate over rows, masks and offsets):
    flat 0.37 (N = 65; 0.34 at 1100)   scale-one 0.31   scale-small 0.32   peaked 0.32   offsets 0.56 (N = 257; 0.51 at 1100)
    peaked-offsets 0.44   round edges (N = 1600: spikes, quiet keys, loud rows) 0.31, 0.31, 0.31   descaled scale-one 0.30, offsets 0.55
TEETH.  Each mutant of the data flow breaks the O gate or the L gate on at least one row at EVERY offset
(largest ratio to the broken gate, smallest over the offsets and cases run):
    (a) a 64-key body missing from P V alone: O 1.9 (flat, 1100 keys, full) to 26 (offsets, 130 keys), L untouched
    (b) a row block of two heads swapped (scale-one, N = 520): every swapped row fails, O >= 3.9
    (c) 32 rows under the other mask: L 3400 and more (O 5.8 and more)     (d) the mask shifted by one key, either way: L 1900 and more
    (e) the last N % 64 keys dropped: L 2.0 (offsets, 577 keys, causal: the 33 last rows see them) to 3000; O alone would miss it
    (f) a 28-unit key on the last / first key of a round, p saturated at 448 under a reference that never saw it: O 6.9, L exact
    (g) keys below 2^-6 of the row maximum flushed: O 1.7 (peaked-offsets, 577 keys, causal) to 12.6 (offsets, 1100 keys)
Mutant (g) is stated against the row maximum (keys below 2^-6 of it lose their share of P V): against a lagging reference the
same threshold flushes only keys below 2^-6 e^-offset, which from offset 2.8 on is a subset of what a correct kernel whose
reference sits at the maximum flushes -- no gate that admits the kernel can refuse that.
The reference is pinned to oracle.attention_forward at two shapes.

DESCALES.  fa2_forward_fp8_scaled through the stub launchers of tests/capi_harness.py: a descale of +inf, like NaN, 0 and a
negative one, is FA2_ERR_INVALID_SHAPE with nothing launched (include/fa2_mi355x.h: positive and finite)."""
import math

import numpy as np
import pytest
import torch

import capi_harness as ch
import fp8_ref as F

ROOM = 0.75
MASKS = (False, True)
CASES = {label: rest for label, *rest in F.cpu_cases()}


def _ratios(O, L, ref, gate, lgate):
    eo, el = F.row_errors(O, L, ref)
    return float((eo / gate).max()), float((el / lgate).max())


def _prepared(label, causal):
    Q, K, V, s = CASES[label]
    ref = F.reference(Q, K, V, s, causal)
    return Q, K, V, s, ref, F.row_gate(ref, V), F.l_gate(ref)


# ------------------------------------------------------------------------------------------------ inputs and reference
def test_inputs_are_what_they_claim():
    for regime in F.REGIMES:
        Q, K, V, s = F.inputs(regime, 2, 3, 130, 11)
        assert s == F.scale_of(regime)
        for t in (Q, K, V):
            assert t.dtype == torch.float8_e4m3fn and tuple(t.shape) == (2, 3, 130, F.D) and torch.isfinite(t.float()).all()
        again = F.inputs(regime, 2, 3, 130, 11)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(again[:3], (Q, K, V)))
        one = F.inputs(regime, 1, 1, 130, 11)
        assert all(torch.equal(a[0, 0].float(), b[0, 0].float()) for a, b in zip(one[:3], (Q, K, V)))      # head (0, 0) is the one-head problem
        heads = [Q[b, h].float() for b in range(2) for h in range(3)]
        assert all(not torch.equal(heads[i], heads[j]) for i in range(6) for j in range(i))                # every head its own data
        sigma, vbar = F._TABLE[regime][1:]
        sc = F.scores(Q, K, s, False)
        assert 0.88 * sigma < sc.std() < 1.12 * sigma, (regime, sc.std())       # e4m3 rounding adds a few per cent
        assert abs(float(V.double().mean()) - vbar) < 0.01, regime


def test_modifiers():
    Q, K, V, s = F.inputs("flat", 1, 2, 200, 5)
    K2 = F.spike(K, Q, s, 1, 150, 64)
    sc = F.scores(Q, K2, s, False)
    assert abs(sc[0, 1, 150, 64] - F.SPIKE_SCORE) < 0.06 * F.SPIKE_SCORE and np.abs(np.delete(sc[0, 1, 150], 64)).max() < 2.0
    others = [j for j in range(200) if j != 64]
    assert torch.equal(K2[0, 0].float(), K[0, 0].float()) and torch.equal(K2[0, 1].float()[others], K[0, 1].float()[others])
    Q2 = F.loud_row(Q, (0, 0), 7, 16.0)
    assert torch.equal(Q2[0, 0, 7].float(), Q[0, 0, 7].float() * 16.0) and torch.equal(Q2[0, 1].float(), Q[0, 1].float())
    K3 = F.heavy_quiet_key(K, 0, 99)
    assert abs(float(K3[0, 0, 99].float().norm()) - 4.0 * F.D ** 0.5) < 1e-3
    assert np.abs(F.scores(Q, K3, s, False)[0, 0, :, 99]).max() < F.RESCALE_THR        # a large norm, scores below every threshold
    Q, K, V, s = F.round_edge_inputs()
    sc = F.scores(Q, K, s, True)
    for i, key in enumerate(F.ROUND_SPIKE_KEYS):                                       # every spike visible to its row under the mask
        assert sc[0, 0, F.ROUND_N - 1 - i, key] > 26.0
    assert np.abs(sc[0, 1][np.isfinite(sc[0, 1])]).max() <= F.L_SCORE_BOUND            # head 1 keeps the 1e-4 gate on L
    assert F.l_gate(F.reference(Q[0, 1], K[0, 1], V[0, 1], s, True))[0] == F.L_GATE_SMALL


@pytest.mark.parametrize("regime,B,H,N,causal", [("flat", 1, 2, 130, False), ("offsets", 2, 1, 65, True)])
def test_reference_is_the_oracle(regime, B, H, N, causal):
    import oracle
    Q, K, V, s = F.inputs(regime, B, H, N, 3)
    ref = F.reference(Q, K, V, s, causal)
    Or, Lr = oracle.attention_forward(*(t.float().numpy() for t in (Q, K, V)), s, causal=causal)
    assert np.abs(ref["O"] - Or).max() <= 2e-6 * max(1.0, np.abs(Or).max()) and np.abs(ref["L"] - Lr).max() <= 1e-5
    assert np.allclose(ref["P"].sum(-1), 1.0, atol=1e-12) and (ref["l"] >= 1.0).all() and ref["seen"].all()


def test_rows_without_a_key_are_gated_exactly():
    """The empty-row rule: O = 0 and L = -inf, anything else is an infinite error."""
    Q, K, V, s = F.inputs("flat", 1, 1, 8, 1)
    ref = F.reference(Q, K, V, s, True)
    ref["seen"] = ref["seen"].copy()
    ref["seen"][..., 3] = False
    O, L = ref["O"].copy(), ref["L"].copy()
    assert np.isinf(F.row_errors(O, L, ref)[0][0, 0, 3])
    O[0, 0, 3], L[0, 0, 3] = 0.0, -np.inf
    eo, el = F.row_errors(O, L, ref)
    assert eo.max() == 0.0 and el.max() == 0.0


# ------------------------------------------------------------------------------------------------ room
@pytest.mark.parametrize("label", list(CASES))
def test_every_gpu_case_leaves_the_kernel_room(label):
    worst = 0.0
    for causal in MASKS:
        Q, K, V, s, ref, gate, lgate = _prepared(label, causal)
        assert (gate > 0).all() and np.isfinite(gate).all()
        for off in F.OFFSETS:
            ro, rl = _ratios(*F.emulate(Q, K, V, s, causal, off), ref, gate, lgate)
            assert ro <= ROOM, (label, causal, off, ro)
            assert rl <= 1e-6, (label, causal, off, rl)
            worst = max(worst, ro)
    print(f"ROOM {label} {worst:.3f}")


# ------------------------------------------------------------------------------------------------ teeth
def _bites(label, causal, mutant, want=None):
    """Smallest over the offsets of the mutant's largest ratio to the O gate / the L gate; asserts that one of them is broken at
    every offset (want: "O" or "L" -- the gate that has to break)."""
    Q, K, V, s, ref, gate, lgate = _prepared(label, causal)
    out = []
    for off in F.OFFSETS:
        ro, rl = _ratios(*mutant(ref["S"], F.f64(V), off), ref, gate, lgate)
        broken = {"O": ro > 1.0, "L": rl > 1.0, None: ro > 1.0 or rl > 1.0}[want]
        assert broken, (label, causal, off, ro, rl)
        out.append((ro, rl))
    ro, rl = min(o for o, _ in out), min(l for _, l in out)
    print(f"TEETH {mutant.__name__} {label} {'causal' if causal else 'full'}: O {ro:.2f} L {rl:.2f}")
    return ro, rl


def _at(S, off):
    """The reference `off` below the row maxima of (mutated) scores S."""
    return S.max(axis=-1) - off


TEETH_CASES = ("flat-577", "flat-1100", "scale-one-520", "peaked-1100", "offsets-577", "peaked-offsets-1100", "offsets-130")


@pytest.mark.parametrize("label", TEETH_CASES)
@pytest.mark.parametrize("causal", MASKS)
def test_a_body_missing_from_the_second_product_breaks_the_o_gate(label, causal):
    def body_dropped(S, V, off):
        def edit(p8, p):
            p8 = p8.copy()
            p8[:, 64:128] = 0.0
            return p8
        return F.flow(S, V, _at(S, off), edit)
    ro, rl = _bites(label, causal, body_dropped, "O")
    assert rl <= 1e-6          # L is exact under this mutant: only the row gate on O can see it


@pytest.mark.parametrize("causal", MASKS)
def test_rows_of_two_heads_swapped_break_the_gates(causal):
    Q, K, V, s = F.case_inputs(F.ORDER_REGIME, 1, 2, F.ORDER_N)
    ref = F.reference(Q, K, V, s, causal)
    gate, lgate = F.row_gate(ref, V), F.l_gate(ref)
    for off in F.OFFSETS:
        O, L = F.emulate(Q, K, V, s, causal, off)
        ok = _ratios(O, L, ref, gate, lgate)
        assert ok[0] <= ROOM and ok[1] <= 1e-6
        O[0, [0, 1], 256:512], L[0, [0, 1], 256:512] = O[0, [1, 0], 256:512], L[0, [1, 0], 256:512]      # one row block
        eo, el = F.row_errors(O, L, ref)
        bad = (eo > gate) | (el > lgate)
        assert bad[0, :, 256:512].all() and not bad[0, :, :256].any() and not bad[0, :, 512:].any(), (causal, off)
    print(f"TEETH heads_swapped {'causal' if causal else 'full'}: O {float((eo / gate)[0, :, 256:512].min()):.2f} (smallest over the swapped rows)")


@pytest.mark.parametrize("label", ("flat-129", "offsets-577", "scale-one-520"))
@pytest.mark.parametrize("causal", MASKS)
def test_a_row_block_under_the_other_mask_breaks_the_gates(label, causal):
    Q, K, V, s = CASES[label]
    other = F.scores(Q, K, s, not causal)

    def other_mask_rows_32_to_63(S, V, off):
        S = S.copy()
        S[32:64] = other[32:64]
        return F.flow(S, V, _at(S, off))
    _bites(label, causal, other_mask_rows_32_to_63, "L")


@pytest.mark.parametrize("label", ("flat-129", "offsets-577", "peaked-1100"))
@pytest.mark.parametrize("shift", (1, -1))
def test_a_mask_shifted_by_one_key_breaks_the_l_gate(label, shift):
    Q, K, V, s = CASES[label]
    n = Q.shape[0]
    full = F.scores(Q, K, s, False)

    def mask_shifted(S, V, off):
        S2 = np.where(np.arange(n)[None, :] <= np.maximum(np.arange(n)[:, None] + shift, 0), full, -np.inf)
        return F.flow(S2, V, _at(S2, off))
    mask_shifted.__name__ = f"mask_shifted_{shift:+d}"
    _bites(label, True, mask_shifted, "L")


@pytest.mark.parametrize("label", ("offsets-130", "offsets-577", "flat-1100", "peaked-offsets-1100"))
@pytest.mark.parametrize("causal", MASKS)
def test_the_ragged_tail_dropped_breaks_the_l_gate(label, causal):
    n = CASES[label][0].shape[0]
    assert n % 64

    def tail_dropped(S, V, off):
        S2 = S.copy()
        S2[:, n - n % 64:] = -np.inf
        return F.flow(S2, V, _at(S2, off))
    _bites(label, causal, tail_dropped, "L")


@pytest.mark.parametrize("causal", MASKS)
@pytest.mark.parametrize("key", (511, 512, 1023, 1024))
def test_a_spike_clamped_at_448_breaks_the_o_gate(key, causal):
    """What a round wrongly run without lane maxima does to a row whose dominant key lies in it: the reference stays where the
    keys before left it, p = e^28 saturates at 448 in the second product and enters the row sum unrounded."""
    N, row = 1100, 1097
    Q, K, V, s = F.case_inputs("flat", 1, 1, N)
    K = F.spike(K, Q, s, 0, row, key)
    Q, K, V = Q[0, 0], K[0, 0], V[0, 0]
    ref = F.reference(Q, K, V, s, causal)
    gate, lgate = F.row_gate(ref, V), F.l_gate(ref)
    assert ref["P"][row, key] > 0.999
    worst = math.inf
    for off in F.OFFSETS:
        ok = _ratios(*F.emulate(Q, K, V, s, causal, off), ref, gate, lgate)
        assert ok[0] <= ROOM and ok[1] <= 1e-6, (key, causal, off, ok)
        m_ref = ref["m"] - off
        m_ref[row] = np.delete(ref["S"][row], key).max() - off          # the reference never saw the spike
        eo, el = F.row_errors(*F.flow(ref["S"], F.f64(V), m_ref), ref)
        assert eo[row] > gate[row] and el[row] <= lgate[0], (key, causal, off, eo[row] / gate[row])
        worst = min(worst, eo[row] / gate[row])
    print(f"TEETH spike_clamped key {key} {'causal' if causal else 'full'}: O {worst:.1f}")


@pytest.mark.parametrize("label", ("offsets-577", "offsets-1100", "peaked-offsets-577", "peaked-offsets-1100"))
@pytest.mark.parametrize("causal", MASKS)
def test_a_flush_at_2_to_the_minus_6_breaks_the_o_gate(label, causal):
    def flush_at_2_to_minus_6(S, V, off):
        small = np.exp(S - S.max(axis=-1)[:, None]) < 2.0 ** -6
        return F.flow(S, V, _at(S, off), lambda p8, p: np.where(small, 0.0, p8))
    _bites(label, causal, flush_at_2_to_minus_6, "O")


# ------------------------------------------------------------------------------------------------ descale validation
@pytest.fixture(scope="module")
def stub():
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        yield ch.Lib(ch.build(os.path.join(ch.ROOT, "cuda_flashattention_amd", "csrc", "fa2_capi.cpp"), tmp))


def test_fp8_descales_must_be_positive_and_finite(stub):
    fn, base = ch._dense("fa2_forward_fp8_scaled", 128, 577, 1)
    _, status, records = stub.call(1, fn, base)
    assert status == 0 and "fwd_fp8" in records
    for name in ("q_descale", "k_descale", "v_descale"):
        for bad in (math.inf, math.nan, 0.0, -1.0, -math.inf):
            _, status, records = stub.call(1, fn, dict(base, **{name: bad}))
            assert status == -2 and not records, (name, bad, status, records)          # FA2_ERR_INVALID_SHAPE, nothing launched
        _, status, records = stub.call(1, fn, dict(base, **{name: 3.0e38 if name == "v_descale" else 1.0e18}))
        assert status == 0 and "fwd_fp8" in records, name                              # large and finite is served
