"""CPU: tests/lse_ref.py -- the float64 references of the differentiable log-sum-exp and of merging partial results -- pinned to
trusted code with no constant of their own, the CPU floor of the composite route, and what the new entry points refuse without
a GPU.

PINS (relative 1e-12, as tests/test_sink_reference.py):
  * lse_ref.attention without dL is regimes.ref_attention (grouped: ref_grouped) and, with a sink, sink_ref.ref_attention_sink;
  * the keys of a regimes problem split at arbitrary points: merging the parts' forwards is the forward of the whole problem, and
    the chain rule -- merge backward, then every part's backward with its dO_i and dL_i -- reproduces the whole problem's dQ (the
    sum over the parts), dK and dV (the parts' side by side).  The gradient for L that this exercises is not a formula the test
    trusts: it must reproduce the gradients of code that has no such input;
  * with a gradient for the final L: central differences of the scalar loss sum(g o O) + sum(gl L) in float64 on a small problem.
THE FLOOR.  lse_ref.composite_emulation is attention_segments in the kernels' formats (regimes.emulate's convention: bf16 O_i, dO_i
and merged O, fp32 L and dL, P and dS rounded to bf16).  On every case tests/test_gpu_lse.py gates at 5e-3 against the exact
gradient it must stay within 2.5e-3: the formats alone leave the kernels half of the gate."""
import ctypes

import numpy as np
import pytest
import torch

import lse_ref as LR
import regimes as R
from sink_ref import ref_attention_sink

TOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    inf = np.isinf(b)
    assert (np.isinf(a) == inf).all() and (a[inf] == b[inf]).all(), (what, "the infinite entries")
    err = np.abs(a[~inf] - b[~inf]).max(initial=0.0) / max(np.abs(b[~inf]).max(initial=0.0), 1e-300)
    assert err <= TOL, (what, err)


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("nq,nk,causal", [(40, 40, False), (40, 40, True), (24, 70, True), (70, 24, True), (70, 24, False)])
def test_reference_without_dl_is_ref_attention(nq, nk, causal):
    hq, hkv, d = 4, 2, 16
    Q, K, V, dO, s = R.inputs("scale-one", nq, nk, hq, hkv, d, 4100 + nq + nk)
    shift = nk - nq if causal else None
    got = LR.attention(Q, K, V, dO, None, s, shift)
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), got, R.ref_grouped(Q, K, V, dO, s, causal)):
        _close(a, b, n)
    sink = np.array([0.3, -np.inf, 2.0, -1.0])
    got = LR.attention(Q, K, V, dO, None, s, shift, sink)
    k, v = (np.repeat(R.f64(t), hq // hkv, axis=0) for t in (K, V))
    O, L, dQ, dK, dV, dsink, _ = ref_attention_sink(R.f64(Q), k, v, R.f64(dO), s, causal, sink)
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV", "dsink"), got, (O, L, dQ, R._group_sum(dK, hkv), R._group_sum(dV, hkv), dsink)):
        _close(a, b, n + " (sink)")


def _chain(Q, K, V, dO, s, nq, nk, causal, cuts, sink=None, gl=None):
    """O, L of the merged parts and dQ, dK, dV (, dsink) by the chain rule, the keys cut at `cuts`; the sink in the last part."""
    bounds = list(zip((0,) + tuple(cuts), tuple(cuts) + (nk,)))
    parts = []
    for c0, c1 in bounds:
        last = c1 == nk
        O, L = LR.forward(Q, K[:, c0:c1], V[:, c0:c1], s, nk - nq - c0 if causal else None, sink if last else None)
        parts.append((O, L))
    Os, Ls = [p[0] for p in parts], [p[1] for p in parts]
    O, L = LR.merge_forward(Os, Ls)
    dOs, dLs, _ = LR.merge_backward(Os, Ls, O, L, R.f64(dO), gl)
    dQ, dK, dV, dsink = 0.0, [], [], None
    for (c0, c1), Oi, Li, gi, gli in zip(bounds, Os, Ls, dOs, dLs):
        last = c1 == nk
        out = LR.flow(Q, K[:, c0:c1], V[:, c0:c1], gi, gli, s, nk - nq - c0 if causal else None, Oi, Li, sink if last else None)
        dQ = dQ + out[0]
        dK.append(out[1]); dV.append(out[2])
        if last and sink is not None:
            dsink = out[3]
    return (O, L, dQ, np.concatenate(dK, axis=-2), np.concatenate(dV, axis=-2)) + ((dsink,) if sink is not None else ()), Ls


SPLIT_CASES = [  # regime, nq, nk, causal, cuts
    ("scale-one", 40, 100, False, (37,)),
    ("scale-one", 40, 100, True, (60,)),              # the diagonal lies in the last part alone
    ("peaked", 40, 100, True, (13, 59)),
    ("offsets", 100, 40, False, (17,)),               # N_q > N_k
    ("scale-one", 100, 40, True, (25,)),              # N_q > N_k, causal: rows without any key, and more rows without a key of the last part
    ("scale-one", 60, 50, True, (10, 45)),            # the last part (5 keys) is absent from most rows; rows 0..9 see nothing at all
    ("scale-small", 33, 64, False, (1, 2, 3, 40, 41, 63)),
]


@pytest.mark.parametrize("regime,nq,nk,causal,cuts", SPLIT_CASES)
def test_merged_parts_are_the_whole_problem_forward_and_backward(regime, nq, nk, causal, cuts):
    hq, hkv, d = 4, 2, 16
    Q, K, V, dO, s = R.inputs(regime, nq, nk, hq, hkv, d, 4200 + nq + 3 * nk)
    got, Ls = _chain(Q, K, V, dO, s, nq, nk, causal, cuts)
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), got, R.ref_grouped(Q, K, V, dO, s, causal)):
        _close(a, b, n)
    if causal and nq > nk - cuts[-1]:
        assert np.isneginf(Ls[-1]).any(), "the case is meant to hold rows from which the last part is absent"
    if causal and nq > nk:
        assert np.isneginf(got[1]).any() and np.isneginf(np.stack(Ls)).all(axis=0).any()


@pytest.mark.parametrize("nq,nk,causal,cuts", [(40, 100, True, (60,)), (100, 40, True, (25,)), (40, 100, False, (13, 59))])
def test_merged_parts_with_a_sink_in_the_last_part(nq, nk, causal, cuts):
    hq, hkv, d = 4, 2, 16
    Q, K, V, dO, s = R.inputs("offsets", nq, nk, hq, hkv, d, 4300 + nq + 3 * nk)
    sink = np.array([1.0, -np.inf, 4.0, -2.0])
    got, _ = _chain(Q, K, V, dO, s, nq, nk, causal, cuts, sink)
    k, v = (np.repeat(R.f64(t), hq // hkv, axis=0) for t in (K, V))
    O, L, dQ, dK, dV, dsink, _ = ref_attention_sink(R.f64(Q), k, v, R.f64(dO), s, causal, sink)
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV", "dsink"), got, (O, L, dQ, R._group_sum(dK, hkv), R._group_sum(dV, hkv), dsink)):
        _close(a, b, n)


def test_a_gradient_for_l_against_central_differences():
    """loss = sum(g o O) + sum(gl L) on a problem with a sink and rows without a key, split in two: the analytic gradients of the
    direct call and of the chain through the merge agree to 1e-12, and both with central differences (h = 1e-5 on values of order
    1: a truncation error of about h^2 = 1e-10 relative, rounding 1e-16 / h = 1e-11; gate 1e-7)."""
    hq, hkv, d, nq, nk, causal = 2, 1, 8, 9, 6, True
    Q, K, V, dO, s = R.inputs("scale-one", nq, nk, hq, hkv, d, 4400)
    Q, K, V, g = (R.f64(t) for t in (Q, K, V, dO))
    rng = np.random.default_rng(5)
    gl = rng.standard_normal((hq, nq))
    sink = np.array([0.5, -np.inf])
    direct = LR.attention(Q, K, V, g, gl, s, nk - nq, sink)
    chain, _ = _chain(Q, K, V, g, s, nq, nk, causal, (4,), sink, gl)
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV", "dsink"), chain, direct):
        _close(a, b, n)

    def loss(q, k, v, sk):
        O, L = LR.forward(q, k, v, s, nk - nq, sk)
        return (g * O).sum() + (gl * np.where(np.isfinite(L), L, 0.0)).sum()

    h = 1e-5
    for idx, (x, grad) in enumerate(((Q, direct[2]), (K, direct[3]), (V, direct[4]), (sink, direct[5]))):
        num = np.zeros_like(x)
        for at in np.ndindex(x.shape):
            if not np.isfinite(x[at]):
                continue
            vals = []
            for sgn in (1.0, -1.0):
                y = x.copy()
                y[at] += sgn * h
                args = [Q, K, V, sink]
                args[idx] = y
                vals.append(loss(*args))
            num[at] = (vals[0] - vals[1]) / (2 * h)
        err = np.abs(num - grad).max() / np.abs(grad).max()
        assert err <= 1e-7, (idx, err)


def test_merge_rules_for_absent_parts():
    rng = np.random.default_rng(9)
    Os = [rng.standard_normal((5, 4)) for _ in range(3)]
    Ls = [rng.standard_normal(5) for _ in range(3)]
    Ls[1][2] = -np.inf
    Os[1][2] = np.nan                                                # never read
    for l in Ls:
        l[4] = -np.inf
    O, L = LR.merge_forward(Os, Ls)
    assert np.isfinite(O).all() and (O[4] == 0).all() and L[4] == -np.inf and np.isfinite(L[:4]).all()
    dOs, dLs, _ = LR.merge_backward(Os, Ls, O, L, rng.standard_normal((5, 4)), rng.standard_normal(5))
    assert all(np.isfinite(x).all() for x in dOs + dLs)
    assert (dOs[1][2] == 0).all() and dLs[1][2] == 0 and all((x[4] == 0).all() for x in dOs) and all(x[4] == 0 for x in dLs)
    o1, l1 = LR.merge_forward(Os[:1], Ls[:1])
    assert (o1[:4] == Os[0][:4]).all() and (l1[:4] == Ls[0][:4]).all()


# ------------------------------------------------------------------------------------------------ the floor of the composite route
def _floor(regime, split, hkv, d, causal):
    Q, K, V, dO, s = LR.e2e_inputs(regime, split, hkv, d)
    Q, K, V, dO = (R.f64(t) for t in (Q, K, V, dO))
    nq, nk = Q.shape[-2], K.shape[-2]
    exact = LR.attention(Q, K, V, dO, None, s, nk - nq if causal else None)
    got = LR.composite_emulation(Q, K, V, dO, s, causal, split)
    errs = {n: R.rel(a, b) for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), got, exact) if n != "L"}
    errs["L"] = float(np.abs(got[1] - exact[1]).max())
    print(regime, split, hkv, d, causal, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    return errs


_ids = lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


@pytest.mark.parametrize("regime,split,hkv,d,causal", [c for c in LR.e2e_cases() if c not in LR.E2E_DROPPED], ids=_ids)
def test_composite_route_in_the_kernels_formats_leaves_half_the_gate(regime, split, hkv, d, causal):
    errs = _floor(regime, split, hkv, d, causal)
    assert all(errs[n] <= 2.5e-3 for n in ("O", "dQ", "dK", "dV")), errs
    assert errs["L"] <= 5e-5, errs


@pytest.mark.parametrize("regime,split,hkv,d,causal", list(LR.E2E_DROPPED), ids=_ids)
def test_a_case_left_out_of_the_gradient_gates_does_exceed_the_floor(regime, split, hkv, d, causal):
    errs = _floor(regime, split, hkv, d, causal)
    worst = max(errs[n] for n in ("O", "dQ", "dK", "dV"))
    assert 2.5e-3 < worst < 3e-3 and abs(worst - LR.E2E_DROPPED[(regime, split, hkv, d, causal)]) < 5e-6, errs


# ------------------------------------------------------------------------------------------------ status codes, without a GPU
def test_new_entry_points_return_the_documented_codes():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: validation fails first
    dense = lambda ptrs, *tail: lib.fa2_backward_lse(*ptrs, *tail)
    # Q K V sink O L dO dL dQ dK dV dsink
    ok = [one] * 12
    shape = (1, 4, 2, 128, 64, 64, 0.125, 0, 0, one, 1 << 30, None, 7)
    no_sink = [one, one, one, None, one, one, one, one, one, one, one, None]
    assert dense([None] + ok[1:], *shape) == -1
    assert dense(ok[:3] + [None] + ok[4:], *shape) == -1                       # a sink without a dsink ...
    assert dense(ok[:11] + [None], *shape) == -1                               # ... and the other way round
    assert dense(no_sink, 1, 4, 3, 128, 64, 64, 0.125, 0, 0, one, 1 << 30, None, 7) == -2          # 3 K/V heads on 4
    assert dense(no_sink, 1, 4, 2, 128, 0, 64, 0.125, 0, 0, one, 1 << 30, None, 7) == -2
    assert dense(no_sink, 1, 4, 2, 128, 64, 96, 0.125, 0, 0, one, 1 << 30, None, 7) == -3
    assert dense(no_sink, 1, 4, 2, 128, 64, 64, 0.125, 1, 0, one, 1 << 30, None, 7) == -4
    assert dense(no_sink, 1, 4, 2, 128, 64, 64, 0.125, 0, 0, one, 16, None, 7) == -5
    assert dense(no_sink, 1, 4, 2, 128, 64, 64, 0.125, 0, 0, one, 1 << 30, None, 8) == -6          # the single kernel on a rectangle
    no_dl = no_sink[:7] + [None] + no_sink[8:]
    assert dense(no_dl, 1, 4, 2, 128, 64, 64, 0.125, 0, 0, one, 16, None, 7) == -5                   # dL may be NULL: validation goes on
    packed = lambda ptrs, *tail: lib.fa2_backward_varlen_lse(*ptrs, *tail)
    ptail = (one, one, 64, one, 1 << 30, None)
    assert packed([None] + no_sink[1:], 4, 2, 128, 128, 64, 0.125, 0, 0, *ptail) == -1
    assert packed(ok[:3] + [None] + ok[4:], 4, 2, 128, 128, 64, 0.125, 0, 0, *ptail) == -1
    assert packed(no_sink, 4, 3, 128, 128, 64, 0.125, 0, 0, *ptail) == -2
    assert packed(no_sink, 4, 2, 0, 128, 64, 0.125, 0, 0, *ptail) == -2
    assert packed(no_sink, 4, 2, 128, 128, 64, 0.125, 0, 0, one, one, 8, one, 1 << 30, None) == -2    # a plan shorter than its header
    # merge: host arrays of device pointers (the entries are never dereferenced)
    arr = lambda *p: (ctypes.c_void_p * len(p))(*p)
    two, nul = arr(16, 16), arr(16, None)
    fwd = lib.fa2_merge_states
    assert fwd(None, two, 2, one, one, 10, 64, 0, None) == -1
    assert fwd(two, two, 2, None, one, 10, 64, 0, None) == -1
    assert fwd(two, nul, 2, one, one, 10, 64, 0, None) == -1
    assert fwd(two, two, 0, one, one, 10, 64, 0, None) == -2
    assert fwd(two, two, 9, one, one, 10, 64, 0, None) == -2
    assert fwd(two, two, 2, one, one, 0, 64, 0, None) == -2
    assert fwd(two, two, 2, one, one, 10, 96, 0, None) == -3
    assert fwd(two, two, 2, one, one, 10, 128, 1, None) == -4
    bwd = lib.fa2_merge_states_backward
    assert bwd(two, two, one, one, one, None, None, two, 2, 10, 64, 0, None) == -1
    assert bwd(two, two, one, one, None, one, two, two, 2, 10, 64, 0, None) == -1
    assert bwd(two, two, one, one, one, None, two, two, 9, 10, 64, 0, None) == -2
    assert bwd(two, two, one, one, one, None, two, two, 2, 0, 64, 0, None) == -2
    assert bwd(two, two, one, one, one, None, two, two, 2, 10, 32, 0, None) == -3
    assert bwd(two, two, one, one, one, None, two, two, 2, 10, 64, 2, None) == -4
    assert bwd(two, two, one, one, one, None, two, nul, 2, 10, 64, 0, None) == -1


# ------------------------------------------------------------------------------------------------ Python validation
class _Fake(torch.Tensor):
    """A CPU tensor that claims to live on a device (tests/test_ops_validation.py): the validation runs without a GPU, and the
    calls below must raise before any pointer reaches the library."""
    @property
    def is_cuda(self):
        return True


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Fake)


def _parts(n, shape=(2, 3, 5, 64)):
    return [_t(*shape) for _ in range(n)], [_t(*shape[:-1], dtype=torch.float32) for _ in range(n)]


def test_merge_validation_errors():
    import cuda_flashattention_amd as fa
    with pytest.raises(ValueError, match="1..8 parts"):
        fa.merge_states_forward([], [])
    with pytest.raises(ValueError, match="1..8 parts"):
        fa.merge_states_forward(*_parts(9))
    with pytest.raises(ValueError, match="1..8 parts"):
        fa.merge_attention_states(*_parts(9))
    Os, Ls = _parts(2)
    with pytest.raises(ValueError, match="as many Ls"):
        fa.merge_states_forward(Os, Ls[:1])
    with pytest.raises(ValueError, match=r"Os\[1\]: shape"):
        fa.merge_states_forward([Os[0], _t(2, 3, 6, 64, dtype=torch.bfloat16)], Ls)
    with pytest.raises(ValueError, match=r"Ls\[0\]: shape"):
        fa.merge_states_forward(Os, [_t(2, 3, 5, 1, dtype=torch.float32), Ls[1]])
    with pytest.raises(ValueError, match=r"Os\[1\] must be contiguous"):
        fa.merge_states_forward([Os[0], _t(2, 5, 3, 64, dtype=torch.bfloat16).transpose(1, 2)], Ls)
    with pytest.raises(ValueError, match=r"Os\[0\]: dtype"):
        fa.merge_states_forward([Os[0].float(), Os[1]], Ls)
    with pytest.raises(ValueError, match=r"Ls\[1\]: dtype"):
        fa.merge_states_forward(Os, [Ls[0], Ls[1].double()])
    O, L = torch.zeros_like(Os[0]), torch.zeros_like(Ls[0])
    with pytest.raises(ValueError, match="dL: dtype"):
        fa.merge_states_backward(Os, Ls, O, L, O, dL=L.double())
    with pytest.raises(ValueError, match="dO: shape"):
        fa.merge_states_backward(Os, Ls, O, L, O[:1])
    with pytest.raises(ValueError, match="lists of 2"):
        fa.merge_states_backward(Os, Ls, O, L, O, dOs=[O])


def test_a_gradient_for_l_is_checked_like_l():
    import cuda_flashattention_amd as fa
    Q = _t(2, 4, 70, 64, dtype=torch.bfloat16)
    K = _t(2, 2, 30, 64, dtype=torch.bfloat16)
    L = _t(2, 4, 70, dtype=torch.float32)
    with pytest.raises(ValueError, match="dL"):
        fa.flash_attention_2_qk_backward(Q, K, K, Q, L, Q, dL=L.double())
    with pytest.raises(ValueError, match="dL"):
        fa.flash_attention_2_qk_backward(Q, K, K, Q, L, Q, dL=L[:, :, :69])
    with pytest.raises(ValueError, match="dL"):
        fa.flash_attention_2_qk_backward(Q, K, K, Q, L, Q, dL=_t(2, 70, 4, dtype=torch.float32).transpose(1, 2))
    plan = fa.VarlenPlan([0, 30, 70], [0, 10, 30])
    Qp, Kp = _t(4, 70, 64, dtype=torch.bfloat16), _t(2, 30, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="dL"):
        fa.flash_attention_2_varlen_backward(Qp, Kp, Kp, Qp, L[0], Qp, plan, dL=L[0].double())


def test_attention_segments_refuses_a_causal_last_segment_shorter_than_the_queries():
    import cuda_flashattention_amd as fa
    Q = _t(2, 4, 70, 64, dtype=torch.bfloat16)
    seg = lambda n: (_t(2, 2, n, 64, dtype=torch.bfloat16),) * 2
    with pytest.raises(ValueError, match="at least N_q = 70 keys"):
        fa.attention_segments(Q, [seg(300), seg(69)], causal=True)
    with pytest.raises(ValueError, match="1..8"):
        fa.attention_segments(Q, [seg(8)] * 9)
    with pytest.raises(ValueError, match="1..8"):
        fa.attention_segments(Q, [])
    with pytest.raises(ValueError, match="pair"):
        fa.attention_segments(Q, [seg(70)[0]])
