"""GPU: attention over different query and key lengths, dense (fa2_forward_qk / fa2_backward_qk: Q, O, dO, dQ [B, H_q, N_q, d],
K, V, dK, dV [B, H_kv, N_k, d]) and packed (fa2_forward_varlen_qk / fa2_backward_varlen_qk under a two-sided VarlenPlan: Q
[H_q, T_q, d], K, V [H_kv, T_k, d]).  Causal mask bottom-right aligned: key j visible to query i iff j <= i + (len_k - len_q).

REFERENCE.  The oracle computes square problems only, so tests/regimes.py carries a float64 NumPy reference for rectangular
attention, forward and backward (ref_attention, imported here), with the mask and the empty-row rules of include/fa2_mi355x.h: a query row that sees no
key has O = 0, L = -inf, dQ = 0 and adds nothing to dK / dV.  tests/test_qk_plan.py pins it to the oracle on square shapes.  It
runs on the bf16-rounded inputs, K / V repeated to H_q heads on the host, dK / dV summed over each group.

GATES: the project's bf16 ones (tests/test_gpu_varlen.py) -- rel-L2 <= 5e-3 on O, dQ, dK, dV over the whole tensor, max |dL| <=
1e-4 over the rows whose reference L is finite; the set of rows with L == -inf is EXACTLY the reference's, and O and dQ are
exactly 0 on them; nothing in O, dQ, dK, dV is NaN or Inf.
One dense shape has no relative error to gate: with N_k = 1 every visible row has P = 1 exactly, so dS = P (dP - D) = 0 and dQ
and dK vanish IDENTICALLY, whatever the inputs (the reference returns ~1e-17 or 0).  dP - D is the difference of two sums of d
products that are equal in exact arithmetic; summed in fp32 in two orders they differ by at most 2 d u sum|dO_c V_c|, u = 2^-24.
There the gate on dQ and dK is that worst-case rounding bound of the formats: ||got - ref|| <= d 2^-23 ||the same formula on
absolute values|| (the magnitude of the terms that cancel) -- at d = 128 about 300 times tighter than 5e-3 of that magnitude.

"Dense" in the packed tests = fa2_forward_qk and fa2_backward_qk (phases 1, then 6) on the sequence alone as [1, H, len, d]: a
block's arithmetic does not depend on where its sequence lives, so the packed outputs are compared with them BIT FOR BIT."""
import functools
import itertools

import numpy as np
import pytest
import torch

from regimes import _group_sum, ref_attention

pytestmark = pytest.mark.gpu

BF16_REL = 5e-3
L_ABS = 1e-4
PAIRS = ((8, 8), (8, 2), (6, 3), (4, 1))                  # both branches of map_block, multi-head, GQA, MQA
DENSE_B = 2
DENSE_SHAPES = ((1, 300), (300, 1), (64, 257), (257, 64), (256, 512),
                (512, 256),                                # a whole row block without a visible key (causal)
                (600, 1100),                               # the forward's rounds without maxima
                (300, 300))
SET_A = ((1, 300), (300, 1), (64, 257), (257, 64), (0, 77), (77, 0), (0, 0), (256, 512), (512, 256), (33, 600), (255, 255))
SET_B = ((600, 1100), (1100, 600), (40, 0), (0, 40))
SETS = {"A": SET_A, "B": SET_B}
DENSE_CASES = tuple(itertools.product(PAIRS, (64, 128), (False, True)))
PACKED_CASES = tuple(itertools.product(PAIRS, (64, 128), (False, True), ("A", "B")))
SENTINEL16, SENTINEL32 = 0x5A5A, 0x5A5A5A5A               # bf16 1.5e16 / fp32 1.5e16: nothing these inputs produce (test_gpu_varlen.py)
NAMES = ("O", "L", "dQ", "dK", "dV")


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _f(t):
    return t.float().cpu().numpy()


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _id(case):
    (hq, hkv), d, causal, *rest = case
    return f"{hq}-{hkv}-d{d}-{'causal' if causal else 'full'}" + "".join(f"-{r}" for r in rest)


def _check_rows_without_a_key(where, got, ref_L):
    """The rows with L == -inf are exactly the reference's; O and dQ are exactly 0 there; O, dQ, dK, dV hold no NaN and no Inf."""
    O, L, dQ, dK, dV = got
    none = torch.from_numpy(np.isneginf(ref_L)).to(L.device)
    assert torch.equal(torch.isneginf(L), none), (where, "the rows with L == -inf", int(torch.isneginf(L).sum()), int(none.sum()))
    assert torch.isfinite(L[~none]).all(), (where, "L")
    for n, t in (("O", O), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert torch.isfinite(t.float()).all(), (where, n)
    assert (O[none] == 0).all() and (dQ[none] == 0).all(), (where, "O / dQ of a row without a key")


def _gate(where, got, ref):
    errs = {}
    finite = np.isfinite(ref[1])
    for n, t, r in zip(NAMES, got, ref):
        errs[n] = float(np.abs(_f(t)[finite] - r[finite]).max(initial=0.0)) if n == "L" else _rel(_f(t), r)
    print(where, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    return errs


# ------------------------------------------------------------------------------------------------ dense
@functools.lru_cache(maxsize=None)
def _dense_inputs(case, shape):
    """Host bf16 Q, K, V, dO (made once, never written)."""
    (hq, hkv), d, causal = case
    nq, nk = shape
    g = torch.Generator().manual_seed(7300 + 16 * DENSE_CASES.index(case) + DENSE_SHAPES.index(shape))
    mk = lambda h, n, s: ((torch.rand(DENSE_B, h, n, d, generator=g) - 0.5) * s).bfloat16()
    return mk(hq, nq, 1.0), mk(hkv, nk, 1.0), mk(hkv, nk, 1.0), mk(hq, nq, 0.4)


def _dense_ref(case, shape, want_abs=False):
    (hq, hkv), d, causal = case
    Q, K, V, dO = _dense_inputs(case, shape)
    G = hq // hkv
    k, v = (_f(t.repeat_interleave(G, dim=1)) for t in (K, V))
    out = ref_attention(_f(Q), k, v, _f(dO), 1.0 / d ** 0.5, causal, want_abs)
    r, mag = out if want_abs else (out, None)
    r = r[:3] + (_group_sum(r[3], hkv), _group_sum(r[4], hkv))
    return (r, (mag[0], _group_sum(mag[1], hkv))) if want_abs else r


def _dense_qk(Q, K, V, dO, s, causal, phases=(7,)):
    fa = _fa()
    O, L = fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    B, hq, nq, d = Q.shape
    ws = torch.empty(fa._capi.lib().fa2_backward_qk_workspace_bytes(B, hq, K.shape[1], nq, K.shape[2], d, 0), dtype=torch.uint8, device="cuda")
    for ph in phases:
        fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph)
    return O, L, dQ, dK, dV


@pytest.mark.parametrize("case", DENSE_CASES, ids=_id)
def test_dense_calls_meet_the_gates(case):
    (hq, hkv), d, causal = case
    s = 1.0 / d ** 0.5
    for shape in DENSE_SHAPES:
        nq, nk = shape
        Q, K, V, dO = (t.cuda() for t in _dense_inputs(case, shape))
        got = _dense_qk(Q, K, V, dO, s, causal)
        torch.cuda.synchronize()
        where = f"{_id(case)} {shape}"
        assert got[0].shape == Q.shape and got[1].shape == Q.shape[:3] and got[2].shape == Q.shape
        assert got[3].shape == K.shape and got[4].shape == V.shape
        ref, mag = _dense_ref(case, shape, want_abs=True)
        _check_rows_without_a_key(where, got, ref[1])
        errs = _gate(where, got, ref)
        for n, e in errs.items():
            if nk == 1 and n in ("dQ", "dK"):      # identically zero: the rounding bound of the formats (the module's docstring)
                a = mag[0] if n == "dQ" else mag[1]
                err = float(np.linalg.norm(_f(got[NAMES.index(n)]) - ref[NAMES.index(n)]))
                print(where, n, f"|got - ref| {err:.3e} against d 2^-23 |terms| {d * 2.0 ** -23 * np.linalg.norm(a):.3e}")
                assert err <= d * 2.0 ** -23 * float(np.linalg.norm(a)), (where, n, err)
            else:
                assert e <= (L_ABS if n == "L" else BF16_REL), (where, n, e)


@pytest.mark.parametrize("case", DENSE_CASES, ids=_id)
def test_equal_lengths_are_the_grouped_query_calls_bit_for_bit(case):
    (hq, hkv), d, causal = case
    lib = _fa()._capi.lib()
    s, st = 1.0 / d ** 0.5, torch.cuda.current_stream().cuda_stream
    for n in (300, 256):
        g = torch.Generator().manual_seed(7900 + n + DENSE_CASES.index(case))
        mk = lambda h, sc: ((torch.rand(DENSE_B, h, n, d, generator=g) - 0.5) * sc).bfloat16().cuda()
        Q, K, V, dO = mk(hq, 1.0), mk(hkv, 1.0), mk(hkv, 1.0), mk(hq, 0.4)
        need = lib.fa2_backward_gqa_workspace_bytes(DENSE_B, hq, hkv, n, d, 0)
        assert lib.fa2_backward_qk_workspace_bytes(DENSE_B, hq, hkv, n, n, d, 0) == need
        for phases in ((7,), (1, 6)):
            got = _dense_qk(Q, K, V, dO, s, causal, phases)
            O, L = torch.empty_like(Q), torch.empty(DENSE_B, hq, n, dtype=torch.float32, device="cuda")
            assert lib.fa2_forward_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), DENSE_B, hq, hkv, n, d, s, 0,
                                       int(causal), st) == 0
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
            for ph in phases:
                assert lib.fa2_backward_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), dO.data_ptr(),
                                            dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), DENSE_B, hq, hkv, n, d, s, 0, int(causal),
                                            ws.data_ptr(), need, st, ph) == 0
            torch.cuda.synchronize()
            for name, a, b in zip(NAMES, got, (O, L, dQ, dK, dV)):
                assert torch.isfinite(a.float()).all(), (n, phases, name)
                assert torch.equal(a, b), (n, phases, name)


# ------------------------------------------------------------------------------------------------ packed
def _cu(lengths):
    return [0] + list(itertools.accumulate(lengths))


def _cus(name):
    return _cu([a for a, _ in SETS[name]]), _cu([b for _, b in SETS[name]])


@functools.lru_cache(maxsize=None)
def _plan(name):
    return _fa().VarlenPlan(*_cus(name))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Host bf16 Q, K, V, dO of a packed case (made once, never written)."""
    (hq, hkv), d, causal, name = case
    cq, ck = _cus(name)
    g = torch.Generator().manual_seed(8100 + PACKED_CASES.index(case))
    mk = lambda h, t, s: ((torch.rand(h, t, d, generator=g) - 0.5) * s).bfloat16()
    return mk(hq, cq[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(hq, cq[-1], 0.4)


@functools.lru_cache(maxsize=None)
def _packed_ref(case):
    """Packed reference O, L, dQ, dK, dV (float64), sequence by sequence (computed once per case, never written)."""
    (hq, hkv), d, causal, name = case
    G, s = hq // hkv, 1.0 / d ** 0.5
    Q, K, V, dO = _inputs(case)
    cq, ck = _cus(name)
    O, L, dQ = np.zeros((hq, cq[-1], d)), np.zeros((hq, cq[-1])), np.zeros((hq, cq[-1], d))
    dK, dV = np.zeros((hkv, ck[-1], d)), np.zeros((hkv, ck[-1], d))
    for q0, q1, k0, k1 in zip(cq[:-1], cq[1:], ck[:-1], ck[1:]):
        k, v = (_f(t[:, k0:k1].repeat_interleave(G, dim=0)) for t in (K, V))
        o, l, gq, gk, gv = ref_attention(_f(Q[:, q0:q1]), k, v, _f(dO[:, q0:q1]), s, causal)
        O[:, q0:q1], L[:, q0:q1], dQ[:, q0:q1] = o, l, gq
        dK[:, k0:k1], dV[:, k0:k1] = _group_sum(gk, hkv), _group_sum(gv, hkv)
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
    """fa2_forward_qk, then fa2_backward_qk with phases 1 and 6, on [1, H, len, d] (through the C ABI itself)."""
    lib = _fa()._capi.lib()
    _, hq, nq, d = q.shape
    hkv, nk = k.shape[1], k.shape[2]
    st = torch.cuda.current_stream().cuda_stream
    O, L = torch.empty_like(q), torch.empty(1, hq, nq, dtype=torch.float32, device="cuda")
    assert lib.fa2_forward_qk(q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), L.data_ptr(), 1, hq, hkv, nq, nk, d, s, 0,
                              int(causal), st) == 0
    need = lib.fa2_backward_qk_workspace_bytes(1, hq, hkv, nq, nk, d, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dQ, dK, dV = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    for ph in (1, 6):
        assert lib.fa2_backward_qk(q.data_ptr(), k.data_ptr(), v.data_ptr(), O.data_ptr(), L.data_ptr(), g.data_ptr(), dQ.data_ptr(),
                                   dK.data_ptr(), dV.data_ptr(), 1, hq, hkv, nq, nk, d, s, 0, int(causal), ws.data_ptr(), need, st, ph) == 0
    return O[0], L[0], dQ[0], dK[0], dV[0]


@pytest.mark.parametrize("case", PACKED_CASES, ids=_id)
def test_packed_calls_meet_the_gates_and_equal_the_dense_calls_per_sequence(case):
    (hq, hkv), d, causal, name = case
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    got = _packed(case, Q, K, V, dO)
    torch.cuda.synchronize()
    assert got[0].shape == Q.shape and got[1].shape == Q.shape[:2] and got[2].shape == Q.shape
    assert got[3].shape == K.shape and got[4].shape == V.shape
    ref = _packed_ref(case)
    _check_rows_without_a_key(_id(case), got, ref[1])
    for n, e in _gate(_id(case), got, ref).items():
        assert e <= (L_ABS if n == "L" else BF16_REL), (n, e)
    s = 1.0 / d ** 0.5
    cq, ck = _cus(name)
    for i, (q0, q1, k0, k1) in enumerate(zip(cq[:-1], cq[1:], ck[:-1], ck[1:])):
        where = f"sequence {i} (rows {q0}:{q1}, keys {k0}:{k1})"
        if q1 == q0:                                     # keys without queries: their gradients are written, as zeros
            assert (got[3][:, k0:k1] == 0).all() and (got[4][:, k0:k1] == 0).all(), where
        if k1 == k0:                                     # queries without keys
            assert (got[0][:, q0:q1] == 0).all() and (got[2][:, q0:q1] == 0).all() and torch.isneginf(got[1][:, q0:q1]).all(), where
        if q1 == q0 or k1 == k0:
            continue
        qc, kc = (lambda t: t[None, :, q0:q1].contiguous()), (lambda t: t[None, :, k0:k1].contiguous())
        want = _dense_one_sequence(qc(Q), kc(K), kc(V), qc(dO), s, causal)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, got, want):
            cut = a[:, k0:k1] if n in ("dK", "dV") else a[:, q0:q1]
            assert torch.equal(cut, b), (where, n)


@pytest.mark.parametrize("d,causal", [(128, True), (128, False), (64, True), (64, False)])
def test_equal_lists_are_the_one_sided_plan_through_either_entry_point(d, causal):
    """cu_seqlens_k equal to cu_seqlens gives the one-sided plan; fa2_forward_varlen_qk / fa2_backward_varlen_qk on it (total_k =
    total_q) return bit for bit what fa2_forward_varlen / fa2_backward_varlen return."""
    fa = _fa()
    lib = fa._capi.lib()
    hq, hkv, lengths = 8, 2, (1, 63, 0, 300, 257)
    cu, s = _cu(lengths), 1.0 / d ** 0.5
    T = cu[-1]
    g = torch.Generator().manual_seed(8700 + d + causal)
    mk = lambda h, sc: ((torch.rand(h, T, d, generator=g) - 0.5) * sc).bfloat16().cuda()
    Q, K, V, dO = mk(hq, 1.0), mk(hkv, 1.0), mk(hkv, 1.0), mk(hq, 0.4)
    one, two = fa.VarlenPlan(cu), fa.VarlenPlan(cu, list(cu))
    assert not two.two_sided and two.total_k == T and bytes(one._blob) == bytes(two._blob)
    O, L = fa.flash_attention_2_varlen_forward(Q, K, V, one, s, causal=causal)
    want = (O, L) + tuple(fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, one, s, causal=causal))
    st, dev = torch.cuda.current_stream().cuda_stream, two.device(Q.device)
    O2, L2 = torch.empty_like(Q), torch.empty_like(L)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    assert lib.fa2_forward_varlen_qk(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O2.data_ptr(), L2.data_ptr(), hq, hkv, T, T, d, s, 0,
                                     int(causal), two.host_ptr(), dev.data_ptr(), two.nbytes, st) == 0
    need = lib.fa2_backward_varlen_qk_workspace_bytes(hq, hkv, T, T, d, 0)
    assert need == lib.fa2_backward_varlen_workspace_bytes(hq, hkv, T, d, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.fa2_backward_varlen_qk(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O2.data_ptr(), L2.data_ptr(), dO.data_ptr(), dQ.data_ptr(),
                                      dK.data_ptr(), dV.data_ptr(), hq, hkv, T, T, d, s, 0, int(causal), two.host_ptr(), dev.data_ptr(),
                                      two.nbytes, ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, want, (O2, L2, dQ, dK, dV)):
        assert torch.isfinite(a.float()).all(), n
        assert torch.equal(a, b), n


@pytest.mark.parametrize("d,causal", [(128, True), (128, False), (64, True), (64, False)])
def test_a_sequence_of_nan_keys_stays_inside_its_sequence(d, causal):
    """K and V of the (64, 257) sequence of set A are NaN: every other sequence's five outputs are bit for bit those of the clean
    run and finite (no DMA row, row constant or fragment of a neighbour is ever part of a sum)."""
    case = ((8, 2), d, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    clean = _packed(case, Q, K, V, dO)
    cq, ck = _cus("A")
    i = SET_A.index((64, 257))
    Kn, Vn = K.clone(), V.clone()
    Kn[:, ck[i]:ck[i + 1]] = float("nan")
    Vn[:, ck[i]:ck[i + 1]] = float("nan")
    dirty = _packed(case, Q, Kn, Vn, dO)
    torch.cuda.synchronize()
    keep_q = torch.ones(cq[-1], dtype=torch.bool, device="cuda")
    keep_k = torch.ones(ck[-1], dtype=torch.bool, device="cuda")
    keep_q[cq[i]:cq[i + 1]] = False
    keep_k[ck[i]:ck[i + 1]] = False
    none = torch.from_numpy(np.isneginf(_packed_ref(case)[1])).cuda()
    for n, a, b in zip(NAMES, clean, dirty):
        keep = keep_k if n in ("dK", "dV") else keep_q
        fin = torch.isfinite(b[:, keep].float())
        assert (fin | none[:, keep]).all() if n == "L" else fin.all(), n       # (L = -inf on the rows without a key, as in the clean run)
        assert torch.equal(a[:, keep], b[:, keep]), n
    assert torch.isnan(dirty[0][:, cq[i]:cq[i + 1]].float()).all()             # the sequence itself did see its keys


def _carve(flat, offset, shape):
    n = int(np.prod(shape))
    return flat[offset:offset + n].view(shape)


@pytest.mark.parametrize("pair,d,causal", [((8, 2), 128, True), ((6, 3), 64, False), ((4, 1), 128, False), ((8, 8), 64, True)])
def test_nothing_is_written_outside_the_packed_tensors_and_every_row_is_written(pair, d, causal):
    """Q and the outputs live inside larger flat buffers filled with a sentinel: after forward and backward the elements in front
    of row 0 of head 0 and behind the last row of the last head still hold it, and no element of a row in [0, T_q) / [0, T_k) does
    -- the zero stores of the empty sides (O, dQ of queries without keys; dK, dV of keys without queries) included."""
    fa = _fa()
    case = (pair, d, causal, "A")
    hq, hkv = pair
    Qh, Kh, Vh, dOh = _inputs(case)
    Tq, Tk, plan, s, pad = Qh.shape[1], Kh.shape[1], _plan("A"), 1.0 / d ** 0.5, 4096
    flat16 = lambda n: torch.full((n + 2 * pad,), SENTINEL16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    dims = {"Q": (hq, Tq, d), "O": (hq, Tq, d), "dQ": (hq, Tq, d), "dK": (hkv, Tk, d), "dV": (hkv, Tk, d)}
    bufs = {n: flat16(int(np.prod(shape))) for n, shape in dims.items()}
    Lbuf = torch.full((hq * Tq + 2 * pad,), SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    t = {n: _carve(b, pad, dims[n]) for n, b in bufs.items()}
    L = _carve(Lbuf, pad, (hq, Tq))
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
    for n, a in zip(NAMES, ref):
        assert torch.equal(a, L if n == "L" else t[n]), n


@pytest.mark.parametrize("pair,d,causal", [((8, 2), 128, True), ((6, 3), 64, True), ((8, 8), 128, False), ((4, 1), 64, False)])
def test_two_runs_are_bit_identical(pair, d, causal):
    case = (pair, d, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    first = _packed(case, Q, K, V, dO)
    again = _packed(case, Q, K, V, dO, plan=_fa().VarlenPlan(*_cus("A")))          # a plan of its own: two builds, one order
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, first, again):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("causal", [False, True])
def test_autograd_returns_what_the_two_calls_return(causal):
    fa = _fa()
    case = ((8, 2), 128, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = fa.attention_varlen(q, k, v, _plan("A"), causal=causal)
    out.backward(dO)
    want = _packed(case, Q, K, V, dO)
    dcase, shape = ((8, 2), 128, causal), (257, 64)
    Qd, Kd, Vd, dOd = (t.cuda() for t in _dense_inputs(dcase, shape))
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (Qd, Kd, Vd))
    outd = fa.attention_qk(qd, kd, vd, causal=causal)
    outd.backward(dOd)
    wantd = _dense_qk(Qd, Kd, Vd, dOd, 1.0 / 128 ** 0.5, causal)
    torch.cuda.synchronize()
    for (o, a, b, c), w, (X, Y, Z) in (((out, q, k, v), want, (Q, K, V)), ((outd, qd, kd, vd), wantd, (Qd, Kd, Vd))):
        assert a.grad.shape == X.shape and b.grad.shape == Y.shape and c.grad.shape == Z.shape
        assert torch.equal(o.detach(), w[0])
        for n, x, y in (("dQ", a.grad, w[2]), ("dK", b.grad, w[3]), ("dV", c.grad, w[4])):
            assert torch.isfinite(x.float()).all(), n
            assert torch.equal(x, y), n


@pytest.mark.parametrize("d,causal", [(128, True), (64, False)])
def test_forward_and_backward_replay_from_a_captured_graph(d, causal):
    """One capture of forward + backward (one stream, no branches) and one replay reproduce the eager results bit for bit, packed
    and dense: the calls allocate nothing and synchronise nothing.  The eager runs come first: they upload the plan (a copy)."""
    fa = _fa()
    lib = fa._capi.lib()
    case = ((8, 2), d, causal, "A")
    Q, K, V, dO = (t.cuda() for t in _inputs(case))
    plan, s = _plan("A"), 1.0 / d ** 0.5
    want = _packed(case, Q, K, V, dO)
    H, T, _ = Q.shape
    Hkv, Tk, _ = K.shape
    O, L = torch.empty_like(Q), torch.empty(H, T, dtype=torch.float32, device="cuda")
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    ws = torch.empty(lib.fa2_backward_varlen_qk_workspace_bytes(H, Hkv, T, Tk, d, 0), dtype=torch.uint8, device="cuda")
    shape = (256, 512)
    Qd, Kd, Vd, dOd = (t.cuda() for t in _dense_inputs(case[:3], shape))
    wantd = _dense_qk(Qd, Kd, Vd, dOd, s, causal)
    Od, Ld = torch.empty_like(Qd), torch.empty(Qd.shape[:3], dtype=torch.float32, device="cuda")
    dQd, dKd, dVd = torch.empty_like(Qd), torch.empty_like(Kd), torch.empty_like(Vd)
    wsd = torch.empty(lib.fa2_backward_qk_workspace_bytes(DENSE_B, H, Hkv, *shape, d, 0), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal, O=O, L=L)
        fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws)
        fa.flash_attention_2_qk_forward(Qd, Kd, Vd, s, causal=causal, O=Od, L=Ld)
        fa.flash_attention_2_qk_backward(Qd, Kd, Vd, Od, Ld, dOd, s, causal=causal, dQ=dQd, dK=dKd, dV=dVd, workspace=wsd)
    for t in (O, dQ, dK, dV, Od, dQd, dKd, dVd):
        t.view(torch.int16).fill_(SENTINEL16)
    for t in (L, Ld):
        t.view(torch.int32).fill_(SENTINEL32)
    ws.zero_()
    wsd.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES + NAMES, want + wantd, (O, L, dQ, dK, dV, Od, Ld, dQd, dKd, dVd)):
        assert torch.equal(a, b), n
