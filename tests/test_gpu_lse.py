"""GPU: a gradient for the log-sum-exp L (fa2_backward_lse / fa2_backward_varlen_lse), merging partial results (fa2_merge_states /
fa2_merge_states_backward) and attention over key segments (attention_segments), against tests/lse_ref.py (float64; pinned on the
CPU by tests/test_lse_reference.py).

GATES, the project's bf16 ones (tests/test_gpu_qk.py, tests/test_gpu_regimes.py): rel-L2 <= 5e-3 on O, dQ, dK, dV over the whole
tensor; |dL| <= 1e-4 where |L_ref| <= 25, 1e-3 beyond.
1. dL IN THE BACKWARD.  Reference: lse_ref.flow fed the GPU forward's own bf16 O and fp32 L and the dL of the call (the arrays the
   kernels are handed), so that what is left is the kernels' own error.  dL is random of the size of D = rowsum(dO o O), and once
   100 x that, so that the row constant D' = D - dL is dominated by it.  dsink: the isolating bound of tests/test_gpu_sink.py with
   dL among the terms of D' (one more fp32 rounding): |got - feed| <= ((d + 1 + B N_q) 2^-24 + (4 + max |s - L|) 2^-22) M,
   M = sum_rows P_sink (sum_c |dO_c O_c| + |dL|).
2. MERGE FORWARD against lse_ref.merge_forward of the same bf16 parts: every element of O within one bf16 rounding,
   |d| <= 2^-8 |ref| + 2^-133 (the smallest bf16 subnormal).  The kernel sums in fp32, each weight exp2((L_i - m) log2 e) good to a
   few 2^-24: its own error is about n 2^-23 of sum_i w_i |O_i|, which stays far below the 2^-9 |ref| that the bound leaves beside
   the final rounding only where the terms do not cancel.  The parts of these tests are therefore positive (the `offsets` regime's V
   has a mean of 0.5; the synthetic O_i lie in [0.1, 1)): on centred data a bound relative to |ref| alone is missed on the few
   elements in 10^4 whose terms cancel to 2^-14 of their size, by any fp32 implementation.
3. MERGE BACKWARD: dO_i within one bf16 rounding of the float64 w_i dO (+ 2^-126: fp32 flushes a w_i below that to 0); dL_i within
   the fp32 worst case of the formula on the same arrays, u = 2^-24, A = rowsum(|dO| |O_i - O|), T = |dL| + A:
       w_i (2 d u A + ((4 + |L_i - L|) 4 u + 2 u) T) + 2^-126 (1 + T)
   -- the length-d sum, then the multiply by w_i = exp2((L_i - L) log2 e) (the argument's and the exponential's roundings, as the
   sink bound above) and the add and the product, each rounding once.  The measured maximum of |d| / bound is printed.
4. END TO END: attention_segments against the exact float64 attention over the concatenated keys -- O, L by the gates; the
   gradients by autograd against the exact gradient on the cases whose formats alone stay within 2.5e-3 on the CPU
   (lse_ref.E2E_DROPPED names the six that do not); every case against attention_qk on the concatenated tensors within twice
   the gate."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import lse_ref as LR
import regimes as R

pytestmark = pytest.mark.gpu

BF16_REL = 5e-3
B, H = 2, 4
U = 2.0 ** -24
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5          # NaN patterns: nothing a kernel computes from finite data


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _f(t):
    return t.float().cpu().numpy().astype(np.float64)


def _l_gate(got, ref, where):
    fin = np.isfinite(ref)
    assert (np.isneginf(got) == np.isneginf(ref)).all() and np.isfinite(got[fin]).all(), (where, "the rows with L = -inf")
    dl = np.abs(got[fin] - ref[fin])
    near = np.abs(ref[fin]) <= 25.0
    e = (float(dl[near].max(initial=0.0)), float(dl[~near].max(initial=0.0)))
    assert e[0] <= 1e-4 and e[1] <= 1e-3, (where, "L", e)
    return e


def _sinks(nk):
    base = math.log(max(nk, 1))
    return torch.tensor([-math.inf, -30.0, base, base + 3], dtype=torch.float32)


def _dsink_bound(sink_h, L, dO, O, dL, d, heads_axis):
    """The isolating bound of the module's docstring, per head, and which heads have a sink.  L, dL [.., H, ..rows], dO, O with d last."""
    sk = sink_h.double().numpy()
    has = np.isfinite(sk)
    L64 = np.moveaxis(L.cpu().numpy().astype(np.float64), heads_axis, 0).reshape(len(sk), -1)
    terms = np.moveaxis((np.abs(_f(dO)) * np.abs(_f(O))).sum(-1) + np.abs(_f(dL)), heads_axis, 0).reshape(len(sk), -1)
    live = has[:, None] & np.isfinite(L64)
    gap = np.where(live, np.abs(sk[:, None] - np.where(np.isfinite(L64), L64, 0.0)), 0.0)
    M = (np.where(live, np.exp(-gap), 0.0) * terms).sum(axis=1)          # (a sink never exceeds its row's L: exp(s - L) = exp(-gap))
    return ((d + 1 + L64.shape[1]) * U + (4 + gap.max(axis=1)) * 4 * U) * M, has


# ================================================================================================ 1. dL in the backward
DL_CASES = [(shape, hkv, d, causal, sink)
            for shape, ds, causals in (((256, 256), (128,), (False, True)), ((300, 300), (64, 128), (False, True)),
                                       ((70, 300), (64, 128), (False, True)), ((300, 70), (64, 128), (True,)))
            for hkv in (4, 2, 1) for d in ds for causal in causals for sink in (False, True)]


def _dl_id(c):
    (nq, nk), hkv, d, causal, sink = c
    return f"{nq}x{nk}-kv{hkv}-d{d}-{'causal' if causal else 'full'}{'-sink' if sink else ''}"


@functools.lru_cache(maxsize=4)
def _dl_inputs(shape, hkv, d):
    nq, nk = shape
    g = torch.Generator().manual_seed(6100 + 7 * nq + 3 * nk + 11 * hkv + d)
    mk = lambda h, n, sc: ((torch.rand(B, h, n, d, generator=g) - 0.5) * sc).bfloat16()
    return mk(H, nq, 1.0), mk(hkv, nk, 1.0), mk(hkv, nk, 1.0), mk(H, nq, 0.4), torch.randn(B, H, nq, generator=g)


def _bwd(Q, K, V, O, L, dO, s, causal, sink, dL, phases=(7,), ws=None):
    """dQ, dK, dV, dsink (None without a sink) of flash_attention_2_qk_backward, the phase masks in turn on one workspace."""
    fa = _fa()
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    dsink = None if sink is None else torch.full((Q.shape[1],), float("nan"), device="cuda")
    if ws is None:
        ws = torch.empty(fa._capi.lib().fa2_backward_qk_workspace_bytes(Q.shape[0], Q.shape[1], K.shape[1], Q.shape[2], K.shape[2], Q.shape[3], 0),
                         dtype=torch.uint8, device="cuda")
    for ph in phases:
        fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph, sink=sink,
                                         dsink=dsink, dL=dL)
    return dQ, dK, dV, dsink


def _same(a, b, what):
    for n, x, y in zip(("dQ", "dK", "dV", "dsink"), a, b):
        if x is not None:
            assert torch.equal(x, y), (what, n)


def _single_kernel(nq, nk, hkv, d, causal):
    """Whether fa2_backward takes the single kernel for this problem on this device (then phases 1 | 8 make up 7, not 1 | 6)."""
    if nq != nk:
        return False
    return _fa()._capi.lib().fa2_backward_gqa_plan(B, H, hkv, nq, d, 0, 1 if causal else 0, None) == 1


@pytest.mark.parametrize("case", DL_CASES, ids=_dl_id)
def test_backward_with_a_gradient_for_l(case):
    fa = _fa()
    (nq, nk), hkv, d, causal, with_sink = case
    host = _dl_inputs((nq, nk), hkv, d)
    Q, K, V, dO = (t.cuda() for t in host[:4])
    s = 1.0 / d ** 0.5
    sink_h = _sinks(nk) if with_sink else None
    sink = None if sink_h is None else sink_h.cuda()
    shift = nk - nq if causal else None
    O, L = fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal, sink=sink)
    Dsize = float((dO.float() * O.float()).sum(-1).std())
    where = _dl_id(case)
    base = _bwd(Q, K, V, O, L, dO, s, causal, sink, None)
    # ---- bit identities
    zero = torch.zeros_like(L)
    _same(_bwd(Q, K, V, O, L, dO, s, causal, sink, zero), base, "a zero dL is the call without it")
    lib, ws = fa._capi.lib(), torch.empty(fa._capi.lib().fa2_backward_qk_workspace_bytes(B, H, hkv, nq, nk, d, 0), dtype=torch.uint8, device="cuda")
    raw = [torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V), None if sink is None else torch.empty(H, device="cuda")]
    st = lib.fa2_backward_lse(Q.data_ptr(), K.data_ptr(), V.data_ptr(), None if sink is None else sink.data_ptr(), O.data_ptr(), L.data_ptr(),
                              dO.data_ptr(), None, raw[0].data_ptr(), raw[1].data_ptr(), raw[2].data_ptr(),
                              None if sink is None else raw[3].data_ptr(), B, H, hkv, nq, nk, d, s, 0, 1 if causal else 0, ws.data_ptr(),
                              ws.numel(), torch.cuda.current_stream().cuda_stream, 7)
    assert st == 0
    _same(raw, base, "fa2_backward_lse without dL is fa2_backward_qk / fa2_backward_sink")
    single = _single_kernel(nq, nk, hkv, d, causal)
    print(where, "phases = 7 runs", "the single kernel" if single else "the two kernels")
    Lh = L.cpu().numpy()
    none = np.isneginf(Lh)
    for scale_dl in (1.0, 100.0):
        dL = (host[4] * (Dsize * scale_dl)).cuda()
        got = _bwd(Q, K, V, O, L, dO, s, causal, sink, dL)
        _same(_bwd(Q, K, V, O, L, dO, s, causal, sink, dL), got, "two runs give the same bits")
        _same(_bwd(Q, K, V, O, L, dO, s, causal, sink, dL, phases=(1, 8) if single else (1, 6)), got, "phase 1, then the rest, is 7")
        torch.cuda.synchronize()
        ref = LR.flow(host[0], host[1], host[2], host[3], dL.cpu(), s, shift, O.cpu(), L.cpu(), sink_h)
        errs = {}
        for n, t, r in zip(("dQ", "dK", "dV"), got, ref):
            assert torch.isfinite(t.float()).all(), (where, n)
            errs[n] = R.rel(_f(t), r)
        print(where, f"dL x{scale_dl:g}", " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        assert all(e <= BF16_REL for e in errs.values()), (where, scale_dl, errs)
        assert not torch.equal(got[0], base[0]) and not torch.equal(got[1], base[1]), (where, "dL changes dQ and dK")
        assert torch.equal(got[2], base[2]), (where, "dV = P^T dO does not see dL")
        if sink is not None:
            ds = got[3].double().cpu().numpy()
            bound, has = _dsink_bound(sink_h, L, dO, O, dL, d, 1)
            print(where, f"dL x{scale_dl:g} dsink {ds} |got - feed| {np.abs(ds - ref[3])} bound {bound}")
            assert np.isfinite(ds).all() and (ds[~has] == 0).all()
            assert (np.abs(ds - ref[3])[has] <= bound[has]).all(), (where, "dsink")
            assert (ds[has] != base[3].double().cpu().numpy()[has]).any()
    # ---- rows with L = -inf ignore their dL, whatever it holds
    if none.any():
        dL = (host[4] * Dsize).cuda()
        clean = _bwd(Q, K, V, O, L, dO, s, causal, sink, torch.where(torch.isneginf(L), torch.zeros_like(dL), dL))
        for poison in (float("nan"), float("inf")):
            got = _bwd(Q, K, V, O, L, dO, s, causal, sink, torch.where(torch.isneginf(L), torch.full_like(dL, poison), dL))
            for t in got:
                assert t is None or torch.isfinite(t.float()).all(), (where, poison)
            _same(got, clean, f"dL = {poison} on the rows with L = -inf")
    else:
        assert (nq, nk, causal) != (300, 70, True), "the rectangle with more queries than keys holds rows without a key"


PACKED_PLANS = {"empty-queries": ((70, 300), (0, 40), (300, 70)), "empty-keys": ((300, 70), (40, 0), (33, 33))}


@pytest.mark.parametrize("with_sink", [False, True], ids=["plain", "sink"])
@pytest.mark.parametrize("hkv,d,causal", [(4, 64, True), (2, 128, False), (1, 128, True), (2, 64, False)])
@pytest.mark.parametrize("name", list(PACKED_PLANS))
def test_packed_backward_with_a_gradient_for_l(name, hkv, d, causal, with_sink):
    fa = _fa()
    seqs = PACKED_PLANS[name]
    cq, ck = ([0] + list(itertools.accumulate(x)) for x in zip(*seqs))
    g = torch.Generator().manual_seed(6500 + len(name) + 5 * hkv + d)
    mk = lambda h, t, sc: ((torch.rand(h, t, d, generator=g) - 0.5) * sc).bfloat16()
    hQ, hK, hV, hdO = mk(H, cq[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(H, cq[-1], 0.4)
    noise = torch.randn(H, cq[-1], generator=g)
    Q, K, V, dO = (t.cuda() for t in (hQ, hK, hV, hdO))
    plan = fa.VarlenPlan(cq, ck)
    assert plan.two_sided
    s = 1.0 / d ** 0.5
    sink_h = _sinks(300) if with_sink else None
    sink = None if sink_h is None else sink_h.cuda()
    O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal, sink=sink)
    run = lambda dL: fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, sink=sink, dL=dL)
    base = run(None)
    _same(run(torch.zeros_like(L)), base, "a zero dL is the call without it")
    lib = fa._capi.lib()
    raw = [torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V), None if sink is None else torch.empty(H, device="cuda")]
    ws = torch.empty(lib.fa2_backward_varlen_qk_workspace_bytes(H, hkv, cq[-1], ck[-1], d, 0), dtype=torch.uint8, device="cuda")
    st = lib.fa2_backward_varlen_lse(Q.data_ptr(), K.data_ptr(), V.data_ptr(), None if sink is None else sink.data_ptr(), O.data_ptr(), L.data_ptr(),
                                     dO.data_ptr(), None, raw[0].data_ptr(), raw[1].data_ptr(), raw[2].data_ptr(),
                                     None if sink is None else raw[3].data_ptr(), H, hkv, cq[-1], ck[-1], d, s, 0, 1 if causal else 0, plan.host_ptr(),
                                     plan.device(Q.device).data_ptr(), plan.nbytes, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    _same(raw, base, "fa2_backward_varlen_lse without dL is fa2_backward_varlen_qk / fa2_backward_varlen_sink")
    dL = (noise * float((dO.float() * O.float()).sum(-1).std())).cuda()
    got = run(dL)
    _same(run(dL), got, "two runs give the same bits")
    torch.cuda.synchronize()
    ref = [np.zeros(tuple(t.shape)) for t in got[:3]] + [np.zeros(H)]
    for q0, q1, k0, k1 in zip(cq[:-1], cq[1:], ck[:-1], ck[1:]):
        if q1 == q0:
            continue
        r = LR.flow(hQ[:, q0:q1], hK[:, k0:k1], hV[:, k0:k1], hdO[:, q0:q1], dL[:, q0:q1].cpu(), s, (k1 - k0) - (q1 - q0) if causal else None,
                    O[:, q0:q1].cpu(), L[:, q0:q1].cpu(), sink_h)
        ref[0][:, q0:q1], ref[1][:, k0:k1], ref[2][:, k0:k1] = r[:3]
        if with_sink:
            ref[3] += r[3]
    errs = {n: R.rel(_f(t), r) for n, t, r in zip(("dQ", "dK", "dV"), got, ref)}
    print(name, hkv, d, causal, with_sink, " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(e <= BF16_REL for e in errs.values()), errs
    for q0, q1, k0, k1 in zip(cq[:-1], cq[1:], ck[:-1], ck[1:]):
        if q1 == q0:                                     # keys without queries: zeros, with or without dL
            assert (got[1][:, k0:k1] == 0).all() and (got[2][:, k0:k1] == 0).all()
    if with_sink:
        ds = got[3].double().cpu().numpy()
        bound, has = _dsink_bound(sink_h, L, dO, O, dL, d, 0)
        print(name, hkv, d, causal, f"dsink {ds} |got - feed| {np.abs(ds - ref[3])} bound {bound}")
        assert np.isfinite(ds).all() and (ds[~has] == 0).all()
        assert (np.abs(ds - ref[3])[has] <= bound[has]).all(), "dsink"
    none = torch.isneginf(L)
    if not with_sink and (causal or name == "empty-keys"):          # (300, 70) under the mask; a sequence without keys
        assert none.any(), "the plan holds rows without a key"
    if none.any():
        clean = run(torch.where(none, torch.zeros_like(dL), dL))
        got = run(torch.where(none, torch.full_like(dL, float("nan")), dL))
        for t in got:
            assert torch.isfinite(t.float()).all()
        _same(got, clean, "dL = NaN on the rows with L = -inf")


# ================================================================================================ 2. and 3. merging
MERGE_N = (1, 2, 3, 8)
NQ_M, NK_M = 70, 320                          # R = 2 x 4 x 70 = 560 rows: 17.5 workgroups of 32 rows at d = 64


@functools.lru_cache(maxsize=None)
def _real_parts(n, d):
    """n forward results of the same queries over disjoint key ranges (`offsets` regime: V about 0.5, so O > 0), the last one
    under the causal mask of (70, its keys): where it holds fewer than 70 keys its first rows see none (L_i = -inf).  Device
    tensors [B, H, 70, d] and [B, H, 70], with the inputs and the key ranges."""
    fa = _fa()
    hkv = 2
    parts = [R.inputs("offsets", NQ_M, NK_M, H, hkv, d, 6700 + 13 * n + d + 17 * b) for b in range(B)]
    Q, K, V, dO = (torch.stack([p[j] for p in parts]).cuda() for j in range(4))
    s = parts[0][4]
    cuts = [round(NK_M * i / n) for i in range(n + 1)]
    Os, Ls = [], []
    for i, (c0, c1) in enumerate(zip(cuts[:-1], cuts[1:])):
        O, L = fa.flash_attention_2_qk_forward(Q, K[:, :, c0:c1].contiguous(), V[:, :, c0:c1].contiguous(), s, causal=(i == n - 1))
        Os.append(O); Ls.append(L)
    torch.cuda.synchronize()
    return Os, Ls, dO


@functools.lru_cache(maxsize=None)
def _synthetic_parts(n, d):
    """565 rows (no multiple of 16 or 32): O_i uniform in [0.1, 1), L_i uniform in +-60; a tenth of the (part, row) pairs absent
    (L_i = -inf) with NaN planted in their O_i rows; rows 7 and 564 absent from every part."""
    rows = 565
    g = torch.Generator().manual_seed(6800 + 13 * n + d)
    Os = [(0.1 + 0.9 * torch.rand(rows, d, generator=g)).bfloat16() for _ in range(n)]
    Ls = [(torch.rand(rows, generator=g) - 0.5) * 120.0 for _ in range(n)]
    for O, L in zip(Os, Ls):
        gone = torch.rand(rows, generator=g) < 0.1
        gone[7] = gone[564] = True
        L[gone] = -math.inf
        O[gone] = float("nan")
    dO = ((torch.rand(rows, d, generator=g) - 0.5) * 0.4).bfloat16()
    return [o.cuda() for o in Os], [l.cuda() for l in Ls], dO.cuda()


def _merge_case(kind, n, d):
    return _real_parts(n, d) if kind == "real" else _synthetic_parts(n, d)


MERGE_CASES = list(itertools.product(("real", "synthetic"), MERGE_N, (64, 128)))


@pytest.mark.parametrize("kind,n,d", MERGE_CASES)
def test_merge_forward(kind, n, d):
    fa = _fa()
    Os, Ls, _ = _merge_case(kind, n, d)
    rows = Ls[0].numel()
    pad = 40
    flatO = torch.empty((rows + pad) * d, dtype=torch.int16, device="cuda").fill_(SENT16)
    flatL = torch.empty(rows + pad, dtype=torch.int32, device="cuda").fill_(SENT32)
    O = flatO.view(torch.bfloat16)[:rows * d].view(Os[0].shape)
    L = flatL.view(torch.float32)[:rows].view(Ls[0].shape)
    fa.merge_states_forward(Os, Ls, O=O, L=L)
    O2, L2 = fa.merge_states_forward(Os, Ls)
    torch.cuda.synchronize()
    assert torch.equal(O.view(torch.int16), O2.view(torch.int16)) and torch.equal(L.view(torch.int32), L2.view(torch.int32)), "two runs, the same bits"
    assert (flatO[rows * d:] == SENT16).all() and (flatL[rows:] == SENT32).all(), "nothing is written past row R"
    assert not torch.isnan(O.float()).any() and not torch.isnan(L).any(), "no row is left unwritten, and no planted NaN shows"
    refO, refL = LR.merge_forward([o.cpu() for o in Os], [l.cpu() for l in Ls])
    gO, gL = _f(O), L.cpu().numpy().astype(np.float64)
    e = _l_gate(gL, refL, (kind, n, d))
    dead = np.isneginf(refL)
    assert (gO[dead] == 0).all(), "a row absent from every part has O = 0"
    if kind == "synthetic":
        assert dead.reshape(-1)[7] and dead.reshape(-1)[564] and np.abs(refL[~dead]).max() > 40
    else:
        assert not dead.any() and np.isneginf(Ls[-1].cpu().numpy()).any() == (n > 1 and NK_M - round(NK_M * (n - 1) / n) < NQ_M)
    excess = np.abs(gO - refO) - (2.0 ** -8 * np.abs(refO) + 2.0 ** -133)
    print(kind, n, d, f"L {e[0]:.2e} / {e[1]:.2e}; worst |dO| / (2^-8 |ref|) {float((np.abs(gO - refO) / (2.0 ** -8 * np.abs(refO) + 2.0 ** -133)).max()):.3f}")
    assert (excess <= 0).all(), (kind, n, d, int((excess > 0).sum()), float(excess.max()))
    if n == 1:
        live = ~torch.isneginf(Ls[0])
        assert torch.equal(O[live].view(torch.int16), Os[0][live].view(torch.int16)) and torch.equal(L[live], Ls[0][live]), "one part: its bits"


@pytest.mark.parametrize("with_dl", [False, True], ids=["dO", "dO+dL"])
@pytest.mark.parametrize("kind,n,d", MERGE_CASES)
def test_merge_backward(kind, n, d, with_dl):
    fa = _fa()
    Os, Ls, dO = _merge_case(kind, n, d)
    O, L = fa.merge_states_forward(Os, Ls)
    g = torch.Generator().manual_seed(6900 + n + d)
    dL = (torch.randn(L.shape, generator=g) * 0.3).cuda() if with_dl else None
    dO = dO.reshape(O.shape).contiguous()
    rows = L.numel()
    pad = 40
    flat = [(torch.empty((rows + pad) * d, dtype=torch.int16, device="cuda").fill_(SENT16), torch.empty(rows + pad, dtype=torch.int32, device="cuda").fill_(SENT32))
            for _ in range(n)]
    dOs = [a.view(torch.bfloat16)[:rows * d].view(O.shape) for a, _ in flat]
    dLs = [b.view(torch.float32)[:rows].view(L.shape) for _, b in flat]
    fa.merge_states_backward(Os, Ls, O, L, dO, dL, dOs=dOs, dLs=dLs)
    again = fa.merge_states_backward(Os, Ls, O, L, dO, dL)
    torch.cuda.synchronize()
    for a, b in flat:
        assert (a[rows * d:] == SENT16).all() and (b[rows:] == SENT32).all(), "nothing is written past row R"
    for x, y in zip(dOs + dLs, again[0] + again[1]):
        assert torch.isfinite(x.float()).all() and torch.equal(x, y), "every row written, no planted NaN, two runs the same bits"
    host = lambda ts: [t.cpu() for t in ts]
    rO, rL, A = LR.merge_backward(host(Os), host(Ls), O.cpu(), L.cpu(), dO.cpu(), None if dL is None else dL.cpu())
    w = LR.merge_weights(host(Ls), L.cpu())
    L64 = L.cpu().numpy().astype(np.float64)
    worst = 0.0
    for i in range(n):
        gone = np.isneginf(Ls[i].cpu().numpy())
        gO, gL = _f(dOs[i]), dLs[i].cpu().numpy().astype(np.float64)
        assert (gO[gone] == 0).all() and (gL[gone] == 0).all(), "an absent part gets dO_i = 0, dL_i = 0"
        assert (np.abs(gO - rO[i]) <= 2.0 ** -8 * np.abs(rO[i]) + 2.0 ** -126).all(), (kind, n, d, i, "dO_i")
        T = A[i] + (0.0 if dL is None else np.abs(_f(dL)))
        Li = Ls[i].cpu().numpy().astype(np.float64)
        gap = np.where(gone, 0.0, np.abs(np.where(gone, 0.0, Li) - np.where(np.isneginf(L64), 0.0, L64)))      # |L_i - L| where the part is present
        bound = w[i] * (2 * d * U * A[i] + ((4 + gap) * 4 * U + 2 * U) * T) + 2.0 ** -126 * (1 + T)
        ratio = np.abs(gL - rL[i]) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (kind, n, d, i, "dL_i", float(ratio.max()))
    print(kind, n, d, with_dl, f"dL_i: worst |got - ref| / bound {worst:.3f}")


# ================================================================================================ 4. end to end
_ids = lambda x: "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


@functools.lru_cache(maxsize=2)
def _e2e_exact(regime, split, hkv, d, causal):
    Q, K, V, dO, s = LR.e2e_inputs(regime, split, hkv, d)
    nq, nk = Q.shape[-2], K.shape[-2]
    return (Q, K, V, dO, s), LR.attention(Q, K, V, dO, None, s, nk - nq if causal else None)


def _segments(K, V, split):
    return [(K[:, :, c0:c1].contiguous(), V[:, :, c0:c1].contiguous()) for c0, c1 in LR.segment_bounds(split)]


@pytest.mark.parametrize("regime,split,hkv,d,causal", LR.e2e_cases(), ids=_ids)
def test_attention_segments_end_to_end(regime, split, hkv, d, causal):
    fa = _fa()
    case = (regime, split, hkv, d, causal)
    (hQ, hK, hV, hdO, s), exact = _e2e_exact(*case)
    q, K, V, dO = (t.cuda() for t in (hQ, hK, hV, hdO))
    q.requires_grad_(True)
    segs = [(k.requires_grad_(True), v.requires_grad_(True)) for k, v in _segments(K, V, split)]
    O, L = fa.attention_segments(q, segs, s, causal=causal, return_lse=True)
    O.backward(dO)
    kc, vc, qc = K.clone().requires_grad_(True), V.clone().requires_grad_(True), q.detach().clone().requires_grad_(True)
    Oc, Lc = fa.attention_qk(qc, kc, vc, s, causal=causal, return_lse=True)
    Oc.backward(dO)
    torch.cuda.synchronize()
    assert torch.equal(fa.attention_segments(q.detach(), [(k.detach(), v.detach()) for k, v in segs], s, causal=causal), O.detach())
    got = (O.detach(), L.detach(), q.grad, torch.cat([k.grad for k, _ in segs], dim=2), torch.cat([v.grad for _, v in segs], dim=2))
    cat = (Oc.detach(), Lc.detach(), qc.grad, kc.grad, vc.grad)
    errs = {n: R.rel(_f(t), r) for n, t, r in zip(("O", "L", "dQ", "dK", "dV"), got, exact) if n != "L"}
    cross = {n: R.rel(_f(t), _f(c)) for n, t, c in zip(("O", "L", "dQ", "dK", "dV"), got, cat) if n != "L"}
    eL = _l_gate(got[1].cpu().numpy().astype(np.float64), exact[1], case)
    print(case, " ".join(f"{k} {v:.3e}" for k, v in errs.items()), f"L {eL[0]:.2e}", "| against attention_qk:", " ".join(f"{k} {v:.3e}" for k, v in cross.items()))
    assert errs["O"] <= BF16_REL, errs
    if case not in LR.E2E_DROPPED:
        assert all(errs[n] <= BF16_REL for n in ("dQ", "dK", "dV")), errs
    assert all(v <= 2 * BF16_REL for v in cross.values()), cross
    assert np.abs(got[1].cpu().numpy() - cat[1].cpu().numpy()).max() <= 2e-4


def test_segments_with_a_bf16_sink_parameter_and_a_loss_on_l():
    """The sink joins the softmax once, in the last segment, and its gradient comes back in the parameter's dtype; a loss that
    uses L as well (a z-loss) reaches Q, K and the sink through the merge and through every segment's dL."""
    fa = _fa()
    split, hkv, d, causal = (300, 70), 2, 64, True
    hQ, hK, hV, hdO, s = LR.e2e_inputs("default", split, hkv, d)
    nq, nk = hQ.shape[-2], hK.shape[-2]
    param_h = _sinks(nk).bfloat16()
    gl_h = torch.randn(B, H, nq, generator=torch.Generator().manual_seed(3)) * 0.05
    q, K, V, dO, gl = (t.cuda() for t in (hQ, hK, hV, hdO, gl_h))
    q.requires_grad_(True)
    p = param_h.cuda().requires_grad_(True)
    segs = [(k.requires_grad_(True), v.requires_grad_(True)) for k, v in _segments(K, V, split)]
    O, L = fa.attention_segments(q, segs, s, causal=causal, sink=p, return_lse=True)
    ((O.float() * dO.float()).sum() + (L * gl).sum()).backward()
    torch.cuda.synchronize()
    assert p.grad.dtype == torch.bfloat16 and p.grad.shape == param_h.shape and torch.isfinite(p.grad.float()).all()
    exact = LR.attention(hQ, hK, hV, hdO, gl_h, s, nk - nq, param_h.float())
    got = (O.detach(), L.detach(), q.grad, torch.cat([k.grad for k, _ in segs], dim=2), torch.cat([v.grad for _, v in segs], dim=2))
    errs = {n: R.rel(_f(t), r) for n, t, r in zip(("O", "L", "dQ", "dK", "dV"), got, exact) if n != "L"}
    _l_gate(got[1].cpu().numpy().astype(np.float64), exact[1], "sink")
    ds, has = p.grad.double().cpu().numpy(), np.isfinite(param_h.float().numpy())
    # against the one call on the concatenated tensors under the same loss: within twice the gate (dsink: printed -- on centred
    # data its terms cancel below what bf16 rounding moves them by, tests/test_gpu_sink.py)
    qc, kc, vc, pc = (t.detach().clone().requires_grad_(True) for t in (q, K, V, p))
    Oc, Lc = fa.attention_qk(qc, kc, vc, s, causal=causal, sink=pc, return_lse=True)
    ((Oc.float() * dO.float()).sum() + (Lc * gl).sum()).backward()
    torch.cuda.synchronize()
    cross = {n: R.rel(_f(t), _f(c)) for n, t, c in zip(("O", "dQ", "dK", "dV"), (got[0],) + got[2:], (Oc.detach(), qc.grad, kc.grad, vc.grad))}
    print("segments with a sink and a loss on L:", errs, "| against attention_qk:", cross, "dsink", ds, "attention_qk", pc.grad.float().cpu().numpy(),
          "exact", exact[5])
    assert errs["O"] <= BF16_REL and all(v <= 2 * BF16_REL for v in cross.values()), (errs, cross)
    assert (ds[~has] == 0).all() and (ds[has] != 0).all()


@pytest.mark.parametrize("entry", ["attention", "attention_qk", "attention_varlen"])
def test_return_lse_on_the_autograd_ops(entry):
    """(O, L) with gradients for both equals the raw backward with dL, bit for bit; an L that the loss does not use arrives as
    no gradient at all and the call is the one without return_lse."""
    fa = _fa()
    hkv, d, causal = 2, 64, True
    s = 1.0 / d ** 0.5
    g = torch.Generator().manual_seed(7100)
    if entry == "attention_varlen":
        cq, ck = [0, 70, 70, 370], [0, 300, 340, 410]
        plan = fa.VarlenPlan(cq, ck)
        mk = lambda h, t, sc: ((torch.rand(h, t, d, generator=g) - 0.5) * sc).bfloat16().cuda()
        Q, K, V, dO = mk(H, cq[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(hkv, ck[-1], 1.0), mk(H, cq[-1], 0.4)
        run = lambda q, k, v, **kw: fa.attention_varlen(q, k, v, plan, causal=causal, **kw)
        O, L = fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal)
        raw = lambda dL: fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, dL=dL)
    else:
        nq, nk = (300, 300) if entry == "attention" else (300, 70)
        mk = lambda h, n, sc: ((torch.rand(B, h, n, d, generator=g) - 0.5) * sc).bfloat16().cuda()
        Q, K, V, dO = mk(H, nq, 1.0), mk(hkv, nk, 1.0), mk(hkv, nk, 1.0), mk(H, nq, 0.4)
        op = fa.attention if entry == "attention" else fa.attention_qk
        run = lambda q, k, v, **kw: op(q, k, v, causal=causal, **kw)
        O, L = fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal)
        raw = lambda dL: fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, s, causal=causal, dL=dL)
    gl = (torch.randn(L.shape, generator=g) * 0.05).cuda()
    for use_l in (True, False):
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        o, l = run(q, k, v, return_lse=True)
        assert torch.equal(o.detach(), O) and torch.equal(l.detach(), L) and l.dtype == torch.float32
        loss = (o.float() * dO.float()).sum()
        if use_l:
            loss = loss + (torch.where(torch.isneginf(l), torch.zeros_like(l), l) * gl).sum()
        loss.backward()
        want = raw(torch.where(torch.isneginf(L), torch.zeros_like(gl), gl) if use_l else None)
        torch.cuda.synchronize()
        for n, a, b in zip(("dQ", "dK", "dV"), (q.grad, k.grad, v.grad), want):
            assert torch.isfinite(a.float()).all() and torch.equal(a, b), (entry, use_l, n)
    q = Q.clone().requires_grad_(True)
    run(q, K, V).backward(dO)
    assert torch.equal(q.grad, raw(None)[0])


def test_segments_forward_and_backward_replay_from_a_captured_graph():
    """One capture of the raw halves -- a forward per segment, the merge, its backward, a backward with dL per segment -- on
    preallocated outputs and workspaces, and one replay, reproduce the eager results bit for bit: nothing is allocated and nothing
    synchronises."""
    fa = _fa()
    lib = fa._capi.lib()
    split, hkv, d, causal = (300, 70), 2, 128, True
    hQ, hK, hV, hdO, s = LR.e2e_inputs("default", split, hkv, d)
    Q, K, V, dO = (t.cuda() for t in (hQ, hK, hV, hdO))
    segs = _segments(K, V, split)
    n, nq = len(segs), Q.shape[2]
    new = lambda like: torch.empty_like(like)
    rowsL = lambda: torch.empty(B, H, nq, dtype=torch.float32, device="cuda")
    Os, Ls, dOs, dLs, dQs = [new(Q) for _ in segs], [rowsL() for _ in segs], [new(Q) for _ in segs], [rowsL() for _ in segs], [new(Q) for _ in segs]
    O, L = new(Q), rowsL()
    dKs, dVs = [new(k) for k, _ in segs], [new(v) for _, v in segs]
    wss = [torch.empty(lib.fa2_backward_qk_workspace_bytes(B, H, hkv, nq, k.shape[2], d, 0), dtype=torch.uint8, device="cuda") for k, _ in segs]

    def step():
        for i, (k, v) in enumerate(segs):
            fa.flash_attention_2_qk_forward(Q, k, v, s, causal=causal and i == n - 1, O=Os[i], L=Ls[i])
        fa.merge_states_forward(Os, Ls, O=O, L=L)
        fa.merge_states_backward(Os, Ls, O, L, dO, None, dOs=dOs, dLs=dLs)
        for i, (k, v) in enumerate(segs):
            fa.flash_attention_2_qk_backward(Q, k, v, Os[i], Ls[i], dOs[i], s, causal=causal and i == n - 1, dQ=dQs[i], dK=dKs[i], dV=dVs[i],
                                             workspace=wss[i], dL=dLs[i])

    outs = [O, L] + Os + Ls + dOs + dLs + dQs + dKs + dVs
    step()
    torch.cuda.synchronize()
    want = [t.clone() for t in outs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in outs:
        if t.dtype == torch.bfloat16:
            t.view(torch.int16).fill_(SENT16)
        else:
            t.view(torch.int32).fill_(SENT32)
    for w in wss:
        w.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(outs, want)):
        assert torch.equal(a, b), i
    q = Q.clone().requires_grad_(True)
    fa.attention_segments(q, segs, s, causal=causal).backward(dO)
    assert torch.equal(fa.attention_segments(Q, segs, s, causal=causal), O)
    assert torch.equal(q.grad, sum(dQs[1:], dQs[0])), "autograd is the same composition"
