"""GPU: every bf16 attention entry point away from flat softmax and the default scale -- the square, grouped-query, N_q != N_k and
packed calls, forward and backward on every backward route, and the resumable forward step -- on the regimes of
tests/regimes.py (softmax scale 1 and 2^-5, peaked scores, two late spikes that make the forward lift its reference and run a
row block again, the first of them alone so that the lift is what the result comes from, means in V and dO, and scores around
-115 where exp(-L) overflows).  tests/test_regimes_reference.py certifies
those inputs on the CPU.

FORWARD, against ref_attention on the bf16 inputs: O rel-L2 <= 5e-3; |dL| <= 1e-4 on the rows with |L_ref| <= 25 and <= 1e-3 on the
others (the project's two L gates, tests/test_gpu_parity.py); in the spikes and lift regimes head 0 keeps 1e-4 on every row; the rows with
L = -inf are exactly the reference's and O = 0 there; everything else finite.

BACKWARD.  The kernels are handed O16 = bf16(O_ref) and L32 = fp32(L_ref) of the reference (as test_bwd_bf16_golden_k4 does), so no
forward kernel sits between the inputs and the verdict, and they are judged against ref_flow -- the float64 formulas fed the SAME
two arrays: rel-L2 <= 5e-3 on dQ, dK, dV on every route, everything finite, dQ = 0 exactly on the rows without a key.  (The
kernels take D = rowsum(dO o O) from the bf16 O; with spikes or a mean in V that rounding alone puts the exact gradient 6e-3 to
9e-3 away: tests/regimes.py.)  scale-one and scale-small are also held to 5e-3 against the exact gradients of ref_attention.
low-level: the gates of test_ragged_lengths_run_the_single_kernel (dQ <= 0.15 -- it cancels to ~1e-4 of its terms -- dK, dV <=
2e-2); that case is about every output being finite.
Routes: square and grouped-query N = 1024 -- phases 7; 1 then 6; 8 | 1 (fa2_backward_plan says 1 at both head dims); N = 1100 and the
rectangles -- phases 7; 1 then 6; the packed calls have one route.

BIT FOR BIT, in the spikes and lift regimes (a restart inside a packed item, a lift under grouped heads): each packed sequence's five outputs
equal the dense qk calls on that sequence alone (forward, then backward phases 1 and 6 on the forward's own O and L); grouped-
query O, L and dQ equal the expanded multi-head calls.
PLUMBING: attention / attention_qk / attention_varlen with softmax_scale=1.0 return what the two direct calls return.
Every measured error is printed (pytest -s); DESIGN.md "Tolerances" records the worst per regime and entry point."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import regimes as R

pytestmark = pytest.mark.gpu

BF16_REL = 5e-3
L_ABS, L_ABS_FAR, L_NEAR = 1e-4, 1e-3, 25.0
LOW_LEVEL_GATES = {"dQ": 0.15, "dK": 2e-2, "dV": 2e-2}
GRADS = ("dQ", "dK", "dV")
DENSE = {"square-1024": (R.HEADS_PLAIN, (1024, 1024)), "square-1100": (R.HEADS_PLAIN, (1100, 1100)),
         "gqa-1024": (R.HEADS_GQA, (1024, 1024)), "gqa-1100": (R.HEADS_GQA, (1100, 1100)),
         "qk-300x1100": (R.HEADS_GQA, (300, 1100)), "qk-1100x300": (R.HEADS_GQA, (1100, 300))}
PACKED = {"packed-one": R.PACKED_ONE, "packed-two": R.PACKED_TWO}
# (d, causal) outermost and each packed entry right behind the dense one whose sequence it shares: _case finds it cached
ENTRIES = ("square-1024", "square-1100", "gqa-1024", "gqa-1100", "packed-one", "qk-1100x300", "qk-300x1100", "packed-two")
CASES = tuple((e, d, c) for d, c in itertools.product((64, 128), (False, True)) for e in ENTRIES)


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _f(t):
    return t.float().cpu().numpy()


def _id(case):
    entry, d, causal = case
    return f"{entry}-d{d}-{'causal' if causal else 'full'}"


@functools.lru_cache(maxsize=20)
def _case(regime, hq, hkv, nq, nk, d, causal):
    """One sequence: the host inputs, the float64 reference, what the backward is handed, and ref_flow on that (computed once per
    sequence, shared by the dense and the packed test that hold it, never written)."""
    Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
    ref = R.ref_grouped(Q, K, V, dO, s, causal)
    O16, L32 = R.kernel_feed(ref[0], ref[1])
    return (Q, K, V, dO), s, ref, (O16, L32), R.ref_flow(Q, K, V, dO, s, causal, O16, L32)


def _packed_case(regime, seqs, d, causal):
    """The sequences of a packed batch side by side along the row axis: inputs, reference, feed and ref_flow."""
    hq, hkv = R.HEADS_GQA
    parts = [_case(regime, hq, hkv, nq, nk, d, causal) for nq, nk in seqs]
    cat = lambda xs: torch.cat(xs, dim=1) if isinstance(xs[0], torch.Tensor) else np.concatenate(xs, axis=1)
    pick = lambda i: tuple(cat([p[i][j] for p in parts]) for j in range(len(parts[0][i])))
    return pick(0), parts[0][1], pick(2), pick(3), pick(4)


def _check_forward(where, regime, O, L, ref):
    """O [H, rows, d], L [H, rows] of the kernels against the reference's; returns the measured errors."""
    Of, Lf, Or, Lr = _f(O), L.cpu().numpy().astype(np.float64), ref[0], ref[1]
    none = np.isneginf(Lr)
    dL = np.abs(np.where(none, 0.0, Lf) - np.where(none, 0.0, Lr))
    near = ~none & (np.abs(Lr) <= L_NEAR)
    errs = {"O": R.rel(Of, Or), "L": float(dL[near].max(initial=0.0)), "L far": float(dL[~none & ~near].max(initial=0.0))}
    if regime in R.SPIKED:
        errs["L head 0"] = float(dL[0].max(initial=0.0))
    print(where, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    if regime == "low-level":
        assert Lr[~none].max(initial=-np.inf) < R.LOW_LEVEL_L, (where, "the reference's L is not below -88")
    assert (np.isneginf(Lf) == none).all(), (where, "the rows with L == -inf", int(np.isneginf(Lf).sum()), int(none.sum()))
    assert np.isfinite(Lf[~none]).all() and np.isfinite(Of).all(), (where, "finite")
    assert (Of[none] == 0).all(), (where, "O of a row without a key")
    assert errs["O"] <= BF16_REL and errs["L"] <= L_ABS and errs["L far"] <= L_ABS_FAR, (where, errs)
    assert errs.get("L head 0", 0.0) <= L_ABS, (where, errs)
    return errs


def _check_backward(where, regime, got, case):
    """dQ, dK, dV of one route against ref_flow (and, for the two scale regimes, against the exact gradients)."""
    _, _, ref, _, flow = case
    gf = [_f(t) for t in got]
    errs = {n: R.rel(g, w) for n, g, w in zip(GRADS, gf, flow)}
    exact = {n: R.rel(g, w) for n, g, w in zip(GRADS, gf, ref[2:])}
    print(where, " ".join(f"{k} {v:.3e}" for k, v in errs.items()), "| exact", " ".join(f"{k} {v:.3e}" for k, v in exact.items()))
    for n, g in zip(GRADS, gf):
        assert np.isfinite(g).all(), (where, n, "finite")
    assert (gf[0][np.isneginf(ref[1])] == 0).all(), (where, "dQ of a row without a key")
    for n, e in errs.items():
        assert e <= (LOW_LEVEL_GATES[n] if regime == "low-level" else BF16_REL), (where, n, e)
    if regime in ("scale-one", "scale-small"):
        for n, e in exact.items():
            assert e <= BF16_REL, (where, "against the exact gradient", n, e)
    return errs


# ------------------------------------------------------------------------------------------------ the calls
def _plan_says(hq, n, d, causal):
    return _fa()._capi.lib().fa2_backward_plan(1, hq, n, d, 0, int(causal), ctypes.POINTER(ctypes.c_char_p)())


def _dense_forward(Q, K, V, s, causal):
    fa = _fa()
    if Q.shape[2] == K.shape[2]:
        return fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
    return fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal)


def _dense_backward(Q, K, V, O, L, dO, s, causal, phases):
    """One route of the dense backward ([1, H, N, d] tensors): the phase masks in turn on one workspace."""
    fa = _fa()
    lib = fa._capi.lib()
    _, hq, nq, d = Q.shape
    hkv, nk = K.shape[1], K.shape[2]
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    if nq == nk:
        ws = torch.empty(lib.fa2_backward_gqa_workspace_bytes(1, hq, hkv, nq, d, 0), dtype=torch.uint8, device="cuda")
        call = fa.flash_attention_2_backward
    else:
        ws = torch.empty(lib.fa2_backward_qk_workspace_bytes(1, hq, hkv, nq, nk, d, 0), dtype=torch.uint8, device="cuda")
        call = fa.flash_attention_2_qk_backward
    for ph in phases:
        call(Q, K, V, O, L, dO, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph)
    return dQ, dK, dV


def _plan(seqs):
    fa = _fa()
    cq, ck = ([0] + list(itertools.accumulate(x)) for x in zip(*seqs))
    return (fa.VarlenPlan(cq) if cq == ck else fa.VarlenPlan(cq, ck)), cq, ck


def _routes(hq, nq, nk, d, causal):
    routes = [(7,), (1, 6)]
    if nq == nk == 1024:
        assert _plan_says(hq, nq, d, causal) == 1, "fa2_backward_plan: the single kernel takes N = 1024 at both head dims"
        routes.append((9,))
    return routes


# ------------------------------------------------------------------------------------------------ the tests
def _dense(entry, d, causal):
    fa = _fa()
    (hq, hkv), (nq, nk) = DENSE[entry]
    for regime in R.REGIMES:
        case = _case(regime, hq, hkv, nq, nk, d, causal)
        (Q, K, V, dO), s, ref, (O16, L32), _ = case
        Q, K, V, dO, O16, L32 = (t[None].cuda() for t in (Q, K, V, dO, O16, L32))
        where = f"{_id((entry, d, causal))} {regime}"
        O, L = _dense_forward(Q, K, V, s, causal)
        torch.cuda.synchronize()
        assert O.shape == Q.shape and L.shape == Q.shape[:3]
        _check_forward(where, regime, O[0], L[0], ref)
        grouped_spikes = regime in R.SPIKED and hq != hkv and nq == nk
        if grouped_spikes:                                             # the expanded multi-head call, bit for bit
            Ke, Ve = (t.repeat_interleave(hq // hkv, dim=1).contiguous() for t in (K, V))
            Oe, Le = fa.flash_attention_2_forward(Q, Ke, Ve, s, causal=causal)
            torch.cuda.synchronize()
            assert torch.equal(O, Oe) and torch.equal(L, Le), (where, "O / L of the expanded call")
        for phases in _routes(hq, nq, nk, d, causal):
            got = _dense_backward(Q, K, V, O16, L32, dO, s, causal, phases)
            torch.cuda.synchronize()
            assert got[0].shape == Q.shape and got[1].shape == K.shape and got[2].shape == V.shape
            _check_backward(f"{where} phases {phases}", regime, [t[0] for t in got], case)
            if grouped_spikes:
                dQe = _dense_backward(Q, Ke, Ve, O16, L32, dO, s, causal, phases)[0]
                torch.cuda.synchronize()
                assert torch.equal(got[0], dQe), (where, phases, "dQ of the expanded call")


def _packed(entry, d, causal):
    fa = _fa()
    seqs = PACKED[entry]
    plan, cq, ck = _plan(seqs)
    assert plan.two_sided == (entry == "packed-two")
    for regime in R.REGIMES:
        case = _packed_case(regime, seqs, d, causal)
        (Q, K, V, dO), s, ref, (O16, L32), _ = case
        Q, K, V, dO, O16, L32 = (t.contiguous().cuda() for t in (Q, K, V, dO, O16, L32))
        where = f"{_id((entry, d, causal))} {regime}"
        O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal)
        got = fa.flash_attention_2_varlen_backward(Q, K, V, O16, L32, dO, plan, s, causal=causal)
        torch.cuda.synchronize()
        assert O.shape == Q.shape and L.shape == Q.shape[:2]
        assert got[0].shape == Q.shape and got[1].shape == K.shape and got[2].shape == V.shape
        _check_forward(where, regime, O, L, ref)
        _check_backward(where, regime, got, case)
        for q0, q1, k0, k1 in zip(cq[:-1], cq[1:], ck[:-1], ck[1:]):
            if q1 == q0:                                               # keys without queries: their gradients are written, as zeros
                assert (got[1][:, k0:k1] == 0).all() and (got[2][:, k0:k1] == 0).all(), (where, q0, k0)
        if regime not in R.SPIKED:
            continue
        own = (O, L) + tuple(fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal))
        for i, (q0, q1, k0, k1) in enumerate(zip(cq[:-1], cq[1:], ck[:-1], ck[1:])):
            if q1 == q0 or k1 == k0:
                continue
            qc, kc = (lambda t: t[None, :, q0:q1].contiguous()), (lambda t: t[None, :, k0:k1].contiguous())
            Od, Ld = fa.flash_attention_2_qk_forward(qc(Q), kc(K), kc(V), s, causal=causal)
            want = (Od, Ld) + _dense_backward(qc(Q), kc(K), kc(V), Od, Ld, qc(dO), s, causal, (1, 6))
            torch.cuda.synchronize()
            for n, a, b in zip(("O", "L") + GRADS, own, want):
                cut = a[:, k0:k1] if n in ("dK", "dV") else a[:, q0:q1]
                assert torch.equal(cut, b[0]), (where, f"sequence {i}", n, "the dense call on the sequence alone")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_regime_meets_the_gates(case):
    entry, d, causal = case
    (_dense if entry in DENSE else _packed)(entry, d, causal)


@pytest.mark.parametrize("d", [64, 128])
def test_forward_step_meets_the_gates_on_both_shard_orders(d):
    """N = 1100, H = 3, K / V cut at [0, 300, 1100] and folded in through the carried (Oacc, l, m) in either order, at softmax scale
    1 and 2^-5 and on peaked scores: against the one-shot reference (the sequence of square-1100)."""
    fa = _fa()
    hq, hkv = R.HEADS_PLAIN
    N, cuts = R.STEP_N, R.STEP_CUTS
    for regime in R.STEP_REGIMES:
        (Q, K, V, _), s, ref, _, _ = _case(regime, hq, hkv, N, N, d, False)
        Q, K, V = (t[None].cuda() for t in (Q, K, V))
        for order in ((0, 1), (1, 0)):
            O, L = torch.empty_like(Q), torch.empty(1, hq, N, device="cuda")
            Oacc, M = torch.empty(1, hq, N, d, device="cuda"), torch.empty(1, hq, N, device="cuda")
            for i, blk in enumerate(order):
                ks, vs = (t[:, :, cuts[blk]:cuts[blk + 1]].contiguous() for t in (K, V))
                fa.forward_step(Q, ks, vs, O, L, Oacc, M, s, first=(i == 0), last=(i == len(order) - 1))
            torch.cuda.synchronize()
            _check_forward(f"forward_step-d{d} {regime} order {order}", regime, O[0], L[0], ref)


@pytest.mark.parametrize("entry", ["attention", "attention_qk", "attention_varlen"])
def test_softmax_scale_reaches_the_kernels_through_autograd(entry):
    """softmax_scale=1.0 on scale-one inputs: output and gradients are bit for bit those of the two direct calls at scale 1 -- and
    not those of the default scale."""
    fa = _fa()
    d, causal = {"attention": (64, True), "attention_qk": (128, True), "attention_varlen": (64, False)}[entry]
    hq, hkv = R.HEADS_GQA
    if entry == "attention_varlen":
        plan, _, _ = _plan(R.PACKED_TWO)
        Q, K, V, dO = (torch.cat([R.sequence("scale-one", hq, hkv, nq, nk, d)[j] for nq, nk in R.PACKED_TWO], dim=1).contiguous().cuda()
                       for j in range(4))
        run = lambda q, k, v, **kw: fa.attention_varlen(q, k, v, plan, causal=causal, **kw)
        O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, 1.0, causal=causal)
        want = (O,) + tuple(fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, 1.0, causal=causal))
    else:
        nq, nk = (300, 300) if entry == "attention" else R.QK_SHAPES[0]
        Q, K, V, dO = (t[None].cuda() for t in R.sequence("scale-one", hq, hkv, nq, nk, d)[:4])
        if entry == "attention":
            run = lambda q, k, v, **kw: fa.attention(q, k, v, causal=causal, **kw)
            O, L = fa.flash_attention_2_forward(Q, K, V, 1.0, causal=causal)
            want = (O,) + tuple(fa.flash_attention_2_backward(Q, K, V, O, L, dO, 1.0, causal=causal))
        else:
            run = lambda q, k, v, **kw: fa.attention_qk(q, k, v, causal=causal, **kw)
            O, L = fa.flash_attention_2_qk_forward(Q, K, V, 1.0, causal=causal)
            want = (O,) + tuple(fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, 1.0, causal=causal))
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = run(q, k, v, softmax_scale=1.0)
    out.backward(dO)
    default = run(Q, K, V)
    torch.cuda.synchronize()
    for n, a, b in zip(("O",) + GRADS, (out.detach(), q.grad, k.grad, v.grad), want):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b), n
    assert not torch.equal(default, want[0])
