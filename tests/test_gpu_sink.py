"""GPU: attention sinks -- one learned logit per query head in every row's softmax (include/fa2_mi355x.h, fa2_forward_sink) -- on
the dense (fa2_forward_sink / fa2_backward_sink) and packed (fa2_forward_varlen_sink / fa2_backward_varlen_sink) routes.

REFERENCE: tests/sink_ref.py (float64; tests/test_sink_reference.py pins it to plain attention with one more key), on the
bf16-rounded inputs and the fp32-rounded sinks, K / V repeated to H_q heads on the host, dK / dV summed over each group.
SINKS differ per head and span -inf (no sink), -30 (a sink that vanishes), log N_k - 1, log N_k, log N_k + 1, log N_k + 3 (about
the row's own mass on flat scores) and log N_k + 20 (the sink takes all but ~2e-9 of the row), cycled over the heads; the
three-head cases start the cycle at a different place for every shape (_dense_case says where, and why (1, 1) gets the three
larger ones: with one key the relative error of dQ and dK is set by the bf16 O that D is formed from, about 2^-9 exp(S - s) on a
row, not by the kernels -- measured on the eight-head cases at (1, 1), which hold every sink: dQ, dK 2.5e-3 .. 4.3e-3 on the GPU,
2.0e-3 .. 4.0e-3 in regimes.emulate, the CPU emulation of the formats).

GATES, the project's bf16 ones (tests/test_gpu_qk.py): rel-L2 <= 5e-3 on O, dQ, dK, dV over the whole tensor; max |dL| <= 1e-4 over
the finite rows; the rows with L = -inf are exactly the reference's (a row without a key under a head without a sink); O and dQ
are exactly 0 on every row without a key, whatever its sink; no NaN and no Inf anywhere.

dsink has two gates, both worst-case rounding bounds of the formats (not tuned numbers), u = 2^-24:
  ISOLATING -- against the float64 value of -sum exp(s - L) rowsum(dO o O) on the GPU's OWN bf16 O and fp32 L, the arrays the
    kernel is fed.  What is left is the kernel's arithmetic: D summed in fp32 over d products (d u of its terms), the fp32 sum
    over the head's B N_q rows (B N_q u of its terms), and exp2((s - L) log2 e) in fp32 -- the difference, the product and the
    exponential each round once, an argument error of |s - L| 2 u log2 e plus an ulp of the result: (4 + |s - L|) 4 u covers it.
    |got - that| <= ((d + B N_q) 2^-24 + (4 + max |s - L|) 2^-22) M,   M = sum_rows P_sink sum_c |dO_c O_c|.
  END TO END -- against ref_attention_sink: O comes from P and V with P rounded to bf16 (2^-9 of sum_j P_j |v_j|) and is itself
    rounded to bf16 (2^-9 |O|), L is off by at most the 1e-4 of its own gate (P_sink moves by that relative amount), and the sum is
    fp32:  |got - ref| <= 2^-9 A + 1e-4 PD + B N_q 2^-24 PD,   A = sum_rows P_sink sum_c |dO_c| (sum_j P_j |v_jc| + |O_c|),
    PD = sum_rows P_sink |D|.
  On centred data the terms of dsink cancel and the end-to-end bound exceeds |dsink| itself: such inputs show nothing.  The dsink
  test therefore runs the `offsets` regime of tests/regimes.py (a mean of 0.5 in V and of 0.1 in dO) and asserts on the CPU,
  before any GPU call, that |dsink_ref| >= 50 x the end-to-end bound for every head with a finite sink."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import regimes as R
from sink_ref import dsink_from_kernel_feed, ref_attention_sink

pytestmark = pytest.mark.gpu

BF16_REL, L_ABS = 5e-3, 1e-4
B = 2
HEADS = ((8, 2), (3, 3))
DENSE_SHAPES = ((1, 1),
                (300, 300),                  # a ragged second row block
                (600, 600),                  # causal: the second row block of a pair
                (1024, 1024),                # the single-kernel backward
                (64, 257),
                (257, 64),                   # causal: rows without a key
                (300, 1100))                 # the rounds without maxima at both head dims
PACKED = {"one": R.PACKED_ONE, "two": R.PACKED_TWO}
CASES = tuple(itertools.product(HEADS, (64, 128), (False, True)))
NAMES = ("O", "L", "dQ", "dK", "dV")
SPIKE_SINK = 26.0


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _f(t):
    return t.float().cpu().numpy()


def _id(case):
    (hq, hkv), d, causal, *rest = case
    return f"{hq}-{hkv}-d{d}-{'causal' if causal else 'full'}" + "".join(f"-{r}" for r in rest)


def _sinks(hq, nk, start=0):
    """fp32 [hq]: the seven sinks of the module's docstring, cycled over the heads from position `start`."""
    base = math.log(max(nk, 1))
    vals = (-math.inf, -30.0, base - 1, base, base + 1, base + 3, base + 20)
    return torch.tensor([vals[(start + i) % len(vals)] for i in range(hq)], dtype=torch.float32)


def _no_key(nq, nk, causal):
    """bool [nq]: the rows that see no key."""
    return np.arange(nq) + (nk - nq) < 0 if causal and nk else np.full(nq, nk == 0)


def _grouped_ref(Q, K, V, dO, s, causal, sink):
    """ref_attention_sink for host tensors Q, dO [..., H_q, N_q, d] and K, V [..., H_kv, N_k, d]."""
    hq, hkv = Q.shape[-3], K.shape[-3]
    k, v = (R.f64(t.repeat_interleave(hq // hkv, dim=-3)) for t in (K, V))
    O, L, dQ, dK, dV, dsink, mag = ref_attention_sink(R.f64(Q), k, v, R.f64(dO), s, causal, sink.double().numpy())
    return (O, L, dQ, R._group_sum(dK, hkv), R._group_sum(dV, hkv), dsink), mag


def _run_dense(Q, K, V, dO, sink, s, causal, phases=(7,)):
    """O, L, dQ, dK, dV, dsink of fa2_forward_sink and fa2_backward_sink (the phase masks in turn on one workspace)."""
    fa = _fa()
    b, hq, nq, d = Q.shape
    O, L = fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal, sink=sink)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    dsink = torch.full((hq,), float("nan"), device="cuda")
    ws = torch.empty(fa._capi.lib().fa2_backward_sink_workspace_bytes(b, hq, K.shape[1], nq, K.shape[2], d, 0), dtype=torch.uint8, device="cuda")
    for ph in phases:
        fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph, sink=sink,
                                         dsink=dsink)
    return O, L, dQ, dK, dV, dsink


def _run_packed(Q, K, V, dO, sink, plan, s, causal):
    fa = _fa()
    O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal, sink=sink)
    return (O, L) + tuple(fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, sink=sink))


def _check(where, got, ref, none):
    """The module's gates on O, L, dQ, dK, dV; `none`: bool mask over L's shape of the rows without a key."""
    errs = {}
    O, L, dQ, dK, dV = got[:5]
    minus = torch.from_numpy(np.isneginf(ref[1])).cuda()
    assert torch.equal(torch.isneginf(L), minus), (where, "the rows with L == -inf", int(torch.isneginf(L).sum()), int(minus.sum()))
    assert torch.isfinite(L[~minus]).all(), (where, "L")
    for n, t in (("O", O), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert torch.isfinite(t.float()).all(), (where, n)
    none = torch.from_numpy(none).cuda()
    assert (O[none] == 0).all() and (dQ[none] == 0).all(), (where, "O / dQ of a row without a key")
    finite = np.isfinite(ref[1])
    for n, t, r in zip(NAMES, got, ref):
        errs[n] = float(np.abs(_f(t)[finite] - r[finite]).max(initial=0.0)) if n == "L" else R.rel(_f(t), r)
    print(where, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for n, e in errs.items():
        assert e <= (L_ABS if n == "L" else BF16_REL), (where, n, e)


# ------------------------------------------------------------------------------------------------ 1. shapes
@functools.lru_cache(maxsize=None)
def _dense_case(case, shape):
    """Host inputs (uniform +-0.5 as in tests/test_gpu_qk.py, dO +-0.2), sinks and reference of a dense case (made once)."""
    (hq, hkv), d, causal = case
    nq, nk = shape
    g = torch.Generator().manual_seed(9100 + 16 * CASES.index(case) + DENSE_SHAPES.index(shape))
    mk = lambda h, n, s: ((torch.rand(B, h, n, d, generator=g) - 0.5) * s).bfloat16()
    Q, K, V, dO = mk(hq, nq, 1.0), mk(hkv, nk, 1.0), mk(hkv, nk, 1.0), mk(hq, nq, 0.4)
    # three heads: the cycle starts at 4, 0, 3, 6, 2, 5, 1 over the seven shapes -- every start once, and (1, 1) with the three
    # sinks from log N_k + 1 up: with one key dS = P (dP - D) = P P_sink dP is a difference the kernels form from D = rowsum(dO o O)
    # on the bf16 O, so the relative error of dQ and dK is about 2^-9 P / P_sink = 2^-9 exp(S - s) whatever the kernel does (as
    # the N_k = 1 shape of tests/test_gpu_qk.py), and two rows per head are too few to average a head with exp(S - s) > 1 out
    sink = _sinks(hq, nk, (4 + 3 * DENSE_SHAPES.index(shape)) % 7 if hq < 7 else 0)
    ref, _ = _grouped_ref(Q, K, V, dO, 1.0 / d ** 0.5, causal, sink)
    return (Q, K, V, dO, sink), ref


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dense_shapes_meet_the_gates(case, shape):
    (hq, hkv), d, causal = case
    nq, nk = shape
    host, ref = _dense_case(case, shape)
    Q, K, V, dO, sink = (t.cuda() for t in host)
    got = _run_dense(Q, K, V, dO, sink, 1.0 / d ** 0.5, causal)
    torch.cuda.synchronize()
    assert got[0].shape == Q.shape and got[1].shape == Q.shape[:3] and got[2].shape == Q.shape
    assert got[3].shape == K.shape and got[4].shape == V.shape and got[5].shape == (hq,) and got[5].dtype == torch.float32
    none = np.broadcast_to(_no_key(nq, nk, causal), (B, hq, nq)).copy()
    _check(f"{_id(case)} {shape}", got, ref, none)
    # rows without a key: L is the sink itself
    Lg, s = got[1].cpu().numpy(), host[4].numpy()
    assert (Lg[none] == np.broadcast_to(s[None, :, None], Lg.shape)[none]).all(), "L of a row without a key is its sink"
    assert torch.isfinite(got[5]).all() and (got[5][torch.isneginf(sink)] == 0).all()


@functools.lru_cache(maxsize=None)
def _packed_case(case, name):
    """Host inputs, plan offsets, sinks and the reference (sequence by sequence; dsink and the magnitudes summed) of a packed case."""
    (hq, hkv), d, causal = case
    seqs = PACKED[name]
    cq, ck = ([0] + list(itertools.accumulate(x)) for x in zip(*seqs))
    g = torch.Generator().manual_seed(9700 + 2 * CASES.index(case) + (name == "two"))
    mk = lambda h, t, s: ((torch.rand(h, t, d, generator=g) - 0.5) * s).bfloat16()
    Q, K, V, dO = mk(hq, cq[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(hq, cq[-1], 0.4)
    sink = _sinks(hq, max(b for _, b in seqs), 3 if hq < 7 else 0)
    O, L, dQ = np.zeros((hq, cq[-1], d)), np.zeros((hq, cq[-1])), np.zeros((hq, cq[-1], d))
    dK, dV, dsink = np.zeros((hkv, ck[-1], d)), np.zeros((hkv, ck[-1], d)), np.zeros(hq)
    none = np.zeros((hq, cq[-1]), dtype=bool)
    for q0, q1, k0, k1 in zip(cq[:-1], cq[1:], ck[:-1], ck[1:]):
        r, _ = _grouped_ref(Q[:, q0:q1], K[:, k0:k1], V[:, k0:k1], dO[:, q0:q1], 1.0 / d ** 0.5, causal, sink)
        O[:, q0:q1], L[:, q0:q1], dQ[:, q0:q1], dK[:, k0:k1], dV[:, k0:k1] = r[:5]
        dsink += r[5]
        none[:, q0:q1] = _no_key(q1 - q0, k1 - k0, causal)
    return (Q, K, V, dO, sink), (cq, ck), (O, L, dQ, dK, dV, dsink), none


@pytest.mark.parametrize("name", list(PACKED))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_packed_sets_meet_the_gates_and_equal_the_dense_calls_per_sequence(case, name):
    fa = _fa()
    (hq, hkv), d, causal = case
    host, (cq, ck), ref, none = _packed_case(case, name)
    Q, K, V, dO, sink = (t.cuda() for t in host)
    plan = fa.VarlenPlan(cq) if cq == ck else fa.VarlenPlan(cq, ck)
    assert plan.two_sided == (name == "two")
    s = 1.0 / d ** 0.5
    got = _run_packed(Q, K, V, dO, sink, plan, s, causal)
    torch.cuda.synchronize()
    assert got[0].shape == Q.shape and got[1].shape == Q.shape[:2] and got[3].shape == K.shape and got[5].shape == (hq,)
    _check(f"{_id(case)} packed-{name}", got, ref, none)
    sb = host[4].numpy()[:, None]
    Lg = got[1].cpu().numpy()
    assert (Lg[none] == np.broadcast_to(sb, Lg.shape)[none]).all(), "L of a row without a key is its sink"
    assert torch.isfinite(got[5]).all() and (got[5][torch.isneginf(sink)] == 0).all()
    for i, (q0, q1, k0, k1) in enumerate(zip(cq[:-1], cq[1:], ck[:-1], ck[1:])):
        where = f"sequence {i} (rows {q0}:{q1}, keys {k0}:{k1})"
        if q1 == q0:                                     # keys without queries: their gradients are written, as zeros
            assert (got[3][:, k0:k1] == 0).all() and (got[4][:, k0:k1] == 0).all(), where
        if q1 == q0 or k1 == k0:
            continue
        qc, kc = (lambda t: t[None, :, q0:q1].contiguous()), (lambda t: t[None, :, k0:k1].contiguous())
        want = _run_dense(qc(Q), kc(K), kc(V), qc(dO), sink, s, causal, phases=(1, 6))
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, got, want):            # a block's arithmetic does not depend on where its sequence lives
            cut = a[:, k0:k1] if n in ("dK", "dV") else a[:, q0:q1]
            assert torch.equal(cut, b[0]), (where, n, "the dense call on the sequence alone")


# ------------------------------------------------------------------------------------------------ 2. bit identities
@pytest.mark.parametrize("d,causal", [(128, True), (128, False), (64, True), (64, False)])
def test_a_sink_of_minus_infinity_is_the_call_without_a_sink_bit_for_bit(d, causal):
    fa = _fa()
    hq, hkv = 8, 2
    s = 1.0 / d ** 0.5
    sink = torch.full((hq,), -math.inf, device="cuda")
    for nq, nk in ((300, 300), (1024, 1024), (257, 64), (300, 1100)):
        g = torch.Generator().manual_seed(9900 + nq + nk + d)
        mk = lambda h, n, sc: ((torch.rand(B, h, n, d, generator=g) - 0.5) * sc).bfloat16().cuda()
        Q, K, V, dO = mk(hq, nq, 1.0), mk(hkv, nk, 1.0), mk(hkv, nk, 1.0), mk(hq, nq, 0.4)
        for phases in ((7,), (1, 6)):
            got = _run_dense(Q, K, V, dO, sink, s, causal, phases)
            if nq == nk:                                 # the square calls
                O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
                call = fa.flash_attention_2_backward
                ws = torch.empty(fa._capi.lib().fa2_backward_gqa_workspace_bytes(B, hq, hkv, nq, d, 0), dtype=torch.uint8, device="cuda")
            else:
                O, L = fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal)
                call = fa.flash_attention_2_qk_backward
                ws = torch.empty(fa._capi.lib().fa2_backward_qk_workspace_bytes(B, hq, hkv, nq, nk, d, 0), dtype=torch.uint8, device="cuda")
            dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
            for ph in phases:
                call(Q, K, V, O, L, dO, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph)
            torch.cuda.synchronize()
            for n, a, b in zip(NAMES, got, (O, L, dQ, dK, dV)):
                assert torch.equal(a, b), ((nq, nk), phases, n)
            assert (got[5] == 0).all(), ((nq, nk), phases, "dsink")
    for name in PACKED:
        host, (cq, ck), _, _ = _packed_case(((hq, hkv), d, causal), name)
        Q, K, V, dO = (t.cuda() for t in host[:4])
        plan = fa.VarlenPlan(cq) if cq == ck else fa.VarlenPlan(cq, ck)
        got = _run_packed(Q, K, V, dO, sink, plan, s, causal)
        O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal)
        want = (O, L) + tuple(fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal))
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, got, want):
            assert torch.equal(a, b), (name, n)
        assert (got[5] == 0).all(), (name, "dsink")


# ------------------------------------------------------------------------------------------------ 3. off the flat softmax
@functools.lru_cache(maxsize=8)
def _regime_case(regime, hq, hkv, nq, nk, d, causal):
    Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
    sink = _sinks(hq, nk, 2)
    spiked = sorted({h for h, *_ in R.spike_rows(nq, nk, hq, False)}) if regime in R.SPIKED else []
    for h in spiked:
        sink[h] = SPIKE_SINK
    ref, _ = _grouped_ref(Q, K, V, dO, s, causal, sink)
    return (Q, K, V, dO, sink), s, ref, spiked


@pytest.mark.parametrize("regime,shape", [("spikes", (1100, 1100)), ("spikes", (300, 1100)), ("lift", (1100, 1100)), ("lift", (300, 1100)),
                                          ("peaked", (1100, 1100)), ("peaked", (300, 1100))], ids=lambda x: x if isinstance(x, str) else f"{x[0]}x{x[1]}")
@pytest.mark.parametrize("d,causal", [(128, True), (128, False), (64, True), (64, False)])
def test_restart_lift_and_peaked_scores_under_a_sink(regime, shape, d, causal):
    """The sink is applied once, to what the row ends with: after the restart with maxima (spikes: the 130-unit key), after a lift
    of the reference (lift: the 28-unit key alone), under a pending rescale, and on peaked scores.  A sink of 26 on the spiked
    heads: a row that sees its 28-unit spike keeps 88 % of its mass on it, its neighbours lose all but ~4e-9 of theirs to the sink,
    the row with the 130-unit spike does not notice it.  FORWARD against ref_attention_sink: the module's gates, and every spiked
    row and its two neighbours one by one -- rel-L2 <= 5e-3 on the row of O (P and O each round to bf16 once: 2^-8 where one key
    holds the row), |dL| <= 1e-4 (|L_ref| <= 25) or 1e-3 (beyond: the project's two L gates, tests/test_gpu_regimes.py).
    BACKWARD against regimes.ref_flow fed the GPU forward's own O and L (the arrays the kernels are handed; with a spike the
    rounding of O alone moves the exact gradient past 5e-3: tests/regimes.py): rel-L2 <= 5e-3 on dQ, dK, dV on both routes."""
    hq, hkv = R.HEADS_GQA
    nq, nk = shape
    host, s, ref, spiked = _regime_case(regime, hq, hkv, nq, nk, d, causal)
    Q, K, V, dO = (t[None].cuda() for t in host[:4])
    sink = host[4].cuda()
    where = f"{regime} {shape} d{d} {'causal' if causal else 'full'}"
    flow = first = None
    for phases in ((7,), (1, 6)):
        got = _run_dense(Q, K, V, dO, sink, s, causal, phases)
        torch.cuda.synchronize()
        O, L = _f(got[0][0]), got[1][0].cpu().numpy().astype(np.float64)
        assert np.isfinite(O).all() and np.isfinite(L).all(), where          # (N_q <= N_k: every row of this test sees a key)
        dL = np.abs(L - ref[1])
        near = np.abs(ref[1]) <= 25.0
        errs = {"O": R.rel(O, ref[0]), "L": float(dL[near].max(initial=0.0)), "L far": float(dL[~near].max(initial=0.0))}
        print(where, phases, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        assert errs["O"] <= BF16_REL and errs["L"] <= L_ABS and errs["L far"] <= 1e-3, (where, errs)
        for h, r, j, i in R.spike_rows(nq, nk, hq, causal, R.SPIKED.get(regime, ())):
            assert ref[1][h, r] > max(R.SPIKE_L[i], SPIKE_SINK), (where, "the reference row does not see its spike")
            for row in (r - 1, r, r + 1):                # (the two spiked rows of a head lie 35 rows apart)
                if not 0 <= row < nq:
                    continue
                e = R.rel(O[h, row], ref[0][h, row])
                print(where, f"head {h} row {row} (spike {i} at row {r}): O {e:.3e} L {L[h, row]:.5f} ref {ref[1][h, row]:.5f}")
                assert e <= BF16_REL, (where, h, row, e)
                assert dL[h, row] <= (L_ABS if abs(ref[1][h, row]) <= 25.0 else 1e-3), (where, h, row, dL[h, row])
        if flow is None:                                 # (the second route is handed the same O and L, bit for bit)
            flow, first = R.ref_flow(host[0], host[1], host[2], host[3], s, causal, got[0][0].cpu(), got[1][0].cpu()), got
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
        for n, t, w in zip(NAMES[2:], got[2:5], flow):
            assert np.isfinite(_f(t)).all(), (where, n)
            e = R.rel(_f(t[0]), w)
            print(where, phases, n, f"{e:.3e}")
            assert e <= BF16_REL, (where, phases, n, e)
        feed = dsink_from_kernel_feed(host[4].double().numpy(), L, O, R.f64(host[3]))
        assert torch.isfinite(got[5]).all()
        print(where, phases, "dsink", got[5].cpu().numpy(), "from the kernel's feed", feed)


# ------------------------------------------------------------------------------------------------ 4. dsink
DSINK_CASES = ((300, 300, 128, False), (600, 600, 64, True), (257, 64, 128, True), (300, 1100, 64, True), (1024, 1024, 128, True))


@functools.lru_cache(maxsize=None)
def _dsink_case(nq, nk, d, causal):
    hq, hkv = R.HEADS_GQA
    parts = [R.inputs("offsets", nq, nk, hq, hkv, d, R.seed_of("offsets", nq, nk, d) + 17 * b) for b in range(B)]
    Q, K, V, dO = (torch.stack([p[j] for p in parts]) for j in range(4))
    s = parts[0][4]
    sink = _sinks(hq, nk)
    ref, mag = _grouped_ref(Q, K, V, dO, s, causal, sink)
    return (Q, K, V, dO, sink), s, ref, mag


@pytest.mark.parametrize("nq,nk,d,causal", DSINK_CASES)
def test_dsink_meets_its_two_rounding_bounds(nq, nk, d, causal):
    hq, hkv = R.HEADS_GQA
    host, s, ref, mag = _dsink_case(nq, nk, d, causal)
    sk = host[4].double().numpy()
    has = np.isfinite(sk)
    u = 2.0 ** -24
    e2e = 2.0 ** -9 * mag["A"] + 1e-4 * mag["PD"] + B * nq * u * mag["PD"]
    ratio = np.abs(ref[5][has]) / e2e[has]
    print(f"dsink ({nq}, {nk}) d{d}: |dsink_ref| / end-to-end bound", ratio)
    assert (ratio >= 50).all(), "the inputs do not show dsink: its terms cancel below the bound"        # on the CPU, before any GPU call
    Q, K, V, dO, sink = (t.cuda() for t in host)
    runs = [_run_dense(Q, K, V, dO, sink, s, causal, phases) for phases in ((7,), (7,), (1, 6))]
    torch.cuda.synchronize()
    assert torch.equal(runs[0][5], runs[1][5]), "two runs give the same bits"
    none = np.broadcast_to(_no_key(nq, nk, causal), (B, hq, nq))
    for got in (runs[0], runs[2]):                       # the routing rule's pick, and the two kernels on what phase 1 left
        ds = got[5].double().cpu().numpy()
        assert np.isfinite(ds).all() and (ds[~has] == 0).all()
        O16, L32 = _f(got[0]).astype(np.float64), got[1].cpu().numpy().astype(np.float64)
        feed = dsink_from_kernel_feed(sk, L32, O16, R.f64(host[3]))
        gap = np.where(none | ~has[None, :, None], 0.0, np.abs(sk[None, :, None] - np.where(np.isfinite(ref[1]), ref[1], 0.0)))
        iso = ((d + B * nq) * u + (4 + gap.max(axis=(0, 2))) * 4 * u) * mag["M"]
        print(f"dsink ({nq}, {nk}) d{d}: got {ds}\n  |got - feed| {np.abs(ds - feed)}\n  isolating bound {iso}\n  |got - ref| {np.abs(ds - ref[5])}\n"
              f"  end-to-end bound {e2e}")
        assert (np.abs(ds - feed)[has] <= iso[has]).all(), "the isolating gate"
        assert (np.abs(ds - ref[5])[has] <= e2e[has]).all(), "the end-to-end gate"


# ------------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("entry", ["attention", "attention_qk", "attention_varlen"])
def test_autograd_takes_a_bf16_sink_parameter(entry):
    fa = _fa()
    hq, hkv = 8, 2
    d, causal = {"attention": (64, True), "attention_qk": (128, True), "attention_varlen": (64, False)}[entry]
    s = 1.0 / d ** 0.5
    if entry == "attention_varlen":
        host, (cq, ck), _, _ = _packed_case(((hq, hkv), d, causal), "two")
        plan = fa.VarlenPlan(cq, ck)
        Q, K, V, dO = (t.cuda() for t in host[:4])
        param = host[4].bfloat16().cuda()
        run = lambda q, k, v, p: fa.attention_varlen(q, k, v, plan, causal=causal, sink=p)
        want = _run_packed(Q, K, V, dO, param.float(), plan, s, causal)
    else:
        shape = (300, 300) if entry == "attention" else (257, 64)
        host, _ = _dense_case(((hq, hkv), d, causal), shape)
        Q, K, V, dO = (t.cuda() for t in host[:4])
        param = host[4].bfloat16().cuda()
        run = (lambda q, k, v, p: fa.attention(q, k, v, causal=causal, sink=p)) if entry == "attention" else \
              (lambda q, k, v, p: fa.attention_qk(q, k, v, causal=causal, sink=p))
        want = _run_dense(Q, K, V, dO, param.float(), s, causal)
    q, k, v, p = (t.clone().requires_grad_(True) for t in (Q, K, V, param))
    out = run(q, k, v, p)
    out.backward(dO)
    p32 = param.float().requires_grad_(True)
    run(Q, K, V, p32).backward(dO)
    plain = run(Q, K, V, None)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want[0]) and not torch.equal(plain, want[0])
    for n, a, b in (("dQ", q.grad, want[2]), ("dK", k.grad, want[3]), ("dV", v.grad, want[4])):
        assert a.shape == b.shape and torch.equal(a, b), n
    assert p.grad.dtype == torch.bfloat16 and p.grad.shape == param.shape and torch.equal(p.grad, want[5].bfloat16())
    assert p32.grad.dtype == torch.float32 and torch.equal(p32.grad, want[5])
    assert torch.isfinite(want[5]).all() and (want[5] != 0).any()
