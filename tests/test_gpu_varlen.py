"""GPU: packed variable-length attention (fa2_forward_varlen / fa2_backward_varlen; Q, O, dO, dQ [H_q, T, d], K, V, dK, dV
[H_kv, T, d], L [H_q, T]; sequence i owns rows cu_seqlens[i] : cu_seqlens[i+1] of every head and attends only itself).

"Oracle" = oracle.attention_forward / attention_backward per sequence on the bf16-rounded inputs as [1, H_q, len, d], K / V
repeated to H_q heads on the host, its dK / dV summed over each group in float64.  Gates: the project's bf16 ones (rel-L2 <= 5e-3
on O, dQ, dK, dV over the whole packed tensor; max |dL| <= 1e-4).  "Dense" = fa2_forward_gqa and fa2_backward_gqa (phases 1, then
6: the two kernels forced) on the sequence alone as [1, H, len, d]: a block's arithmetic does not depend on where its sequence
lives, so every output of the packed calls is compared with them BIT FOR BIT."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_REL = 5e-3
L_ABS = 1e-4
PAIRS = ((8, 8), (8, 2), (6, 3), (4, 1))                  # both branches of map_block, multi-head, GQA, MQA
SET_A = (1, 63, 64, 65, 0, 255, 256, 257, 300, 33)        # every 32-key body, 64/128-key tile and 256-row block boundary; a
#                                                           sequence starting at a row that is no multiple of 32; an empty one
SET_B = (600, 1100, 0, 40)                                # the forward's rounds without maxima at both head dims; a ragged end
SETS = {"A": SET_A, "B": SET_B}
CASES = tuple(itertools.product(PAIRS, (64, 128), (False, True), ("A", "B")))
SENTINEL16, SENTINEL32 = 0x5A5A, 0x5A5A5A5A               # bf16 1.5e16 / fp32 1.5e16: nothing these inputs produce


def _id(case):
    (hq, hkv), d, causal, name = case
    return f"{hq}-{hkv}-d{d}-{'causal' if causal else 'full'}-{name}"


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _f(t):
    return t.float().cpu().numpy()


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _cu(lengths):
    return [0] + list(itertools.accumulate(lengths))


@functools.lru_cache(maxsize=None)
def _plan(name):
    return _fa().VarlenPlan(_cu(SETS[name]))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Host bf16 Q, K, V, dO of a case (made once, never written)."""
    (hq, hkv), d, causal, name = case
    T = sum(SETS[name])
    g = torch.Generator().manual_seed(9100 + CASES.index(case))
    mk = lambda h, s: ((torch.rand(h, T, d, generator=g) - 0.5) * s).bfloat16()
    return mk(hq, 1.0), mk(hkv, 1.0), mk(hkv, 1.0), mk(hq, 0.4)


@functools.lru_cache(maxsize=None)
def _oracle_case(case):
    """Packed oracle O, L, dQ and the group sums of dK, dV (float64), sequence by sequence (computed once per case)."""
    import oracle
    (hq, hkv), d, causal, name = case
    G, s = hq // hkv, 1.0 / d ** 0.5
    Q, K, V, dO = _inputs(case)
    T = Q.shape[1]
    O, L, dQ = np.zeros((hq, T, d)), np.zeros((hq, T)), np.zeros((hq, T, d))
    dK, dV = np.zeros((hkv, T, d)), np.zeros((hkv, T, d))
    cu = _cu(SETS[name])
    for r0, r1 in zip(cu[:-1], cu[1:]):
        if r1 == r0:
            continue
        q, g = _f(Q[None, :, r0:r1]), _f(dO[None, :, r0:r1])
        k, v = (_f(t[None, :, r0:r1].repeat_interleave(G, dim=1)) for t in (K, V))
        o, l = oracle.attention_forward(q, k, v, s, causal=causal)
        gq, gk, gv = oracle.attention_backward(q, k, v, g, s, causal=causal)
        O[:, r0:r1], L[:, r0:r1], dQ[:, r0:r1] = o[0], l[0], gq[0]
        dK[:, r0:r1] = gk[0].astype(np.float64).reshape(hkv, G, r1 - r0, d).sum(axis=1)
        dV[:, r0:r1] = gv[0].astype(np.float64).reshape(hkv, G, r1 - r0, d).sum(axis=1)
    return O, L, dQ, dK, dV


def _packed(case, Q, K, V, dO, plan=None):
    """O, L, dQ, dK, dV of the two packed calls."""
    fa = _fa()
    (hq, hkv), d, causal, name = case
    plan = plan or _plan(name)
    s = 1.0 / d ** 0.5
    O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal)
    dQ, dK, dV = fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal)
    return O, L, dQ, dK, dV


def _dense_one_sequence(q, k, v, g, s, causal):
    """fa2_forward_gqa, then fa2_backward_gqa with phases 1 and 6, on [1, H, len, d] (through the C ABI itself: ops sends equal
    head counts to the multi-head calls)."""
    lib = _fa()._capi.lib()
    _, hq, n, d = q.shape
    hkv = k.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    O, L = torch.empty_like(q), torch.empty(1, hq, n, dtype=torch.float32, device="cuda")
    assert lib.fa2_forward_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), L.data_ptr(), 1, hq, hkv, n, d, s, 0,
                               int(causal), st) == 0
    need = lib.fa2_backward_gqa_workspace_bytes(1, hq, hkv, n, d, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dQ, dK, dV = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    for ph in (1, 6):
        assert lib.fa2_backward_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), L.data_ptr(), g.data_ptr(), dQ.data_ptr(),
                                    dK.data_ptr(), dV.data_ptr(), 1, hq, hkv, n, d, s, 0, int(causal), ws.data_ptr(), need, st, ph) == 0
    return O[0], L[0], dQ[0], dK[0], dV[0]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_packed_calls_meet_the_gates_and_equal_the_dense_calls_per_sequence(case):
    (hq, hkv), d, causal, name = case
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    got = _packed(case, Q, K, V, dO)
    torch.cuda.synchronize()
    names = ("O", "L", "dQ", "dK", "dV")
    assert got[0].shape == Q.shape and got[1].shape == Q.shape[:2] and got[2].shape == Q.shape
    assert got[3].shape == K.shape and got[4].shape == V.shape
    for n, t in zip(names, got):
        assert torch.isfinite(t.float()).all(), n
    ref = _oracle_case(case)
    errs = {n: (float(np.abs(_f(t) - r).max()) if n == "L" else _rel(_f(t), r)) for n, t, r in zip(names, got, ref)}
    print(_id(case), " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for n, e in errs.items():
        assert e <= (L_ABS if n == "L" else BF16_REL), (n, e)
    s = 1.0 / d ** 0.5
    cu = _cu(SETS[name])
    for i, (r0, r1) in enumerate(zip(cu[:-1], cu[1:])):
        if r1 == r0:
            continue
        cut = lambda t: t[None, :, r0:r1].contiguous()
        want = _dense_one_sequence(cut(Q), cut(K), cut(V), cut(dO), s, causal)
        torch.cuda.synchronize()
        for n, a, b in zip(names, got, want):
            assert torch.equal(a[:, r0:r1], b), (f"sequence {i} (rows {r0}:{r1})", n)


@pytest.mark.parametrize("d,causal", [(128, True), (128, False), (64, True), (64, False)])
def test_a_sequence_of_nan_keys_stays_inside_its_sequence(d, causal):
    """K and V of the 257-row sequence of set A are NaN: its own outputs are NaN, every other sequence's are bit for bit those of
    the clean run (no DMA row, row constant or fragment of a neighbour is ever part of a sum)."""
    case = ((8, 2), d, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    clean = _packed(case, Q, K, V, dO)
    cu = _cu(SET_A)
    i = SET_A.index(257)
    r0, r1 = cu[i], cu[i + 1]
    Kn, Vn = K.clone(), V.clone()
    Kn[:, r0:r1] = float("nan")
    Vn[:, r0:r1] = float("nan")
    dirty = _packed(case, Q, Kn, Vn, dO)
    torch.cuda.synchronize()
    keep = torch.ones(Q.shape[1], dtype=torch.bool, device="cuda")
    keep[r0:r1] = False
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), clean, dirty):
        assert torch.isfinite(b[:, keep].float()).all(), n
        assert torch.equal(a[:, keep], b[:, keep]), n
        assert torch.isnan(b[:, r0:r1].float()).all(), n


def _carve(flat, offset, shape):
    n = int(np.prod(shape))
    return flat[offset:offset + n].view(shape)


@pytest.mark.parametrize("pair,d,causal", [((8, 2), 128, True), ((6, 3), 64, False), ((4, 1), 128, False), ((8, 8), 64, True)])
def test_nothing_is_written_outside_the_packed_tensors_and_every_row_is_written(pair, d, causal):
    """Q and the outputs live inside larger flat buffers filled with a sentinel: after forward and backward the elements in front
    of row 0 of head 0 and behind row T of the last head still hold it, and no element of a row in [0, T) does."""
    fa = _fa()
    case = (pair, d, causal, "A")
    hq, hkv = pair
    Qh, Kh, Vh, dOh = _inputs(case)
    T, plan, s, pad = Qh.shape[1], _plan("A"), 1.0 / d ** 0.5, 4096
    flat16 = lambda n: torch.full((n + 2 * pad,), SENTINEL16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    bufs = {n: flat16(h * T * d) for n, h in (("Q", hq), ("O", hq), ("dQ", hq), ("dK", hkv), ("dV", hkv))}
    Lbuf = torch.full((hq * T + 2 * pad,), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    t = {n: _carve(b, pad, (hq if n in ("Q", "O", "dQ") else hkv, T, d)) for n, b in bufs.items()}
    L = _carve(Lbuf, pad, (hq, T))
    t["Q"].copy_(Qh)
    K, V, dO = Kh.cuda(), Vh.cuda(), dOh.cuda()
    fa.flash_attention_2_varlen_forward(t["Q"], K, V, plan, s, causal=causal, O=t["O"], L=L)
    fa.flash_attention_2_varlen_backward(t["Q"], K, V, t["O"], L, dO, plan, s, causal=causal, dQ=t["dQ"], dK=t["dK"], dV=t["dV"])
    torch.cuda.synchronize()
    for n, b in list(bufs.items()) + [("L", Lbuf)]:
        raw = b.view(torch.int16 if n != "L" else torch.int32)
        sent = SENTINEL16 if n != "L" else SENTINEL32
        assert (raw[:pad] == sent).all() and (raw[-pad:] == sent).all(), n
        inner = raw[pad:-pad]
        if n == "Q":
            assert torch.equal(t["Q"].cpu(), Qh)
        else:
            assert not (inner == sent).any(), n
    ref = _packed(case, Qh.cuda(), K, V, dO)
    torch.cuda.synchronize()
    for n, a in zip(("O", "L", "dQ", "dK", "dV"), ref):
        assert torch.equal(a, L if n == "L" else t[n]), n


@pytest.mark.parametrize("pair,d,causal", [((8, 2), 128, True), ((6, 3), 64, True), ((8, 8), 128, False), ((4, 1), 64, False)])
def test_two_runs_are_bit_identical(pair, d, causal):
    case = (pair, d, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    first = _packed(case, Q, K, V, dO)
    again = _packed(case, Q, K, V, dO, plan=_fa().VarlenPlan(_cu(SET_A)))          # a plan of its own: two builds, one order
    torch.cuda.synchronize()
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), first, again):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b), n


@pytest.mark.parametrize("causal", [False, True])
def test_autograd_returns_what_the_two_calls_return(causal):
    fa = _fa()
    case = ((8, 2), 128, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = fa.attention_varlen(q, k, v, _plan("A"), causal=causal)
    out.backward(dO)
    O, L, dQ, dK, dV = _packed(case, Q, K, V, dO)
    torch.cuda.synchronize()
    assert k.grad.shape == K.shape and v.grad.shape == V.shape and q.grad.shape == Q.shape
    assert torch.equal(out.detach(), O)
    for n, a, b in (("dQ", q.grad, dQ), ("dK", k.grad, dK), ("dV", v.grad, dV)):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b), n


@pytest.mark.parametrize("d,causal", [(128, True), (64, False)])
def test_forward_and_backward_replay_from_a_captured_graph(d, causal):
    """One capture of forward + backward (one stream, no branches) and one replay reproduce the eager results bit for bit: the
    calls allocate nothing and synchronise nothing.  The eager run comes first: it uploads the plan, which is a copy."""
    fa = _fa()
    case = ((8, 2), d, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    plan, s = _plan("A"), 1.0 / d ** 0.5
    want = _packed(case, Q, K, V, dO)
    H, T, _ = Q.shape
    O, L = torch.empty_like(Q), torch.empty(H, T, dtype=torch.float32, device="cuda")
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    ws = torch.empty(fa._capi.lib().fa2_backward_varlen_workspace_bytes(H, K.shape[0], T, d, 0), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal, O=O, L=L)
        fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws)
    for t in (O, dQ, dK, dV):
        t.view(torch.int16).fill_(SENTINEL16)
    L.view(torch.int32).fill_(SENTINEL32)
    ws.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), want, (O, L, dQ, dK, dV)):
        assert torch.equal(a, b), n
