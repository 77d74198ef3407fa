"""GPU: extend attention (fa2_forward_extend, fa2_forward_extend_paged through flash_attention_2_extend / _paged): more than 32 query
rows per K/V head against bf16 and e4m3 caches, contiguous and paged.

Cases, inputs and the float64 reference are tests/extend_ref.py's (tests/test_extend_reference.py certifies them on the CPU): the
eight shapes M = 33 .. 160 at d = 64 and 128, one batch of the lengths 0, 1, q_len - 1, q_len, 127, 128, 129, 300, 1100, 2500 in a
capacity of 2560 (and seqlens_k = None), n_splits in {0, 1, 2, 7, 64}, the causal mask, no mask, the causal mask under each window
of (0, 1, 31, 127, 128, 200, capacity - 1), with and without a sink, pages of 32 and 96 keys with shared pages.
Gates: decode_ref.within_gates against the float64 reference (5e-3 on O rel-L2, 1e-4 / 1e-3 on |dL|, the -inf rows exactly the
reference's with O exactly 0); PER ROW |O_i - O_ref,i| <= KAPPA u sqrt(sum_j P_ij^2 |v_j|^2) + u |O_i| (tests/decode_rows_ref.py;
the worst ratio is printed with its (sequence, head, token)); and bit equalities without a tolerance."""
import functools

import numpy as np
import pytest
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows
import decode_window_ref as wr
import extend_ref as er

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A      # bf16 / fp32 1.5e16: nothing these inputs produce
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _cuda(ts):
    return tuple(t.cuda() if isinstance(t, torch.Tensor) else t for t in ts)


@functools.lru_cache(maxsize=2)
def _dev(i, fp8):
    """(Q, K, V, k_descale, v_descale, scale, lens or None, sink) on the device; the descales are None beside bf16 caches."""
    if fp8:
        Q, K, V, kd, vd, scale, lens, sink = _cuda(er.inputs_fp8(i))
    else:
        Q, K, V, scale, lens, sink = _cuda(er.inputs(i))
        kd = vd = None
    return Q, K, V, kd, vd, scale, lens if er.CASES[i]["seqlens"] else None, sink


@functools.lru_cache(maxsize=4)
def _pages(i, P, fp8):
    Kp, Vp, table, cap = er.paged_inputs(i, P, fp8)
    return Kp.cuda(), Vp.cuda(), table.cuda(), cap


def _gather(pool, table, lens, P):
    return fr.gather(pool, table, lens, P) if pool.dtype == fr.E4M3 else pr.gather(pool, table, lens, P)


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _check(where, O, L, ref):
    O = O.float().cpu().numpy()
    e = dr.errors(O, L.cpu().numpy(), ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    rows.check(where, O, ref)


def _contiguous(i, k, fp8, n_splits, K=None, V=None, wl="variant", **kw):
    Q, K0, V0, kd, vd, scale, lens, sink = _dev(i, fp8)
    mask, w = er.VARIANTS[k]
    return _fa().flash_attention_2_extend(Q, K0 if K is None else K, V0 if V is None else V, lens, scale, causal=mask == "causal",
                                          sink=sink if er.has_sink(i, k) else None, n_splits=n_splits, k_descale=kd, v_descale=vd,
                                          window_left=w if wl == "variant" else wl, **kw)


def _paged(i, k, fp8, P, n_splits, pools=None, wl="variant", **kw):
    Q, _, _, kd, vd, scale, lens, sink = _dev(i, fp8)
    Kp, Vp, table = pools if pools is not None else _pages(i, P, fp8)[:3]
    mask, w = er.VARIANTS[k]
    return _fa().flash_attention_2_extend_paged(Q, Kp, Vp, table, lens, scale, causal=mask == "causal", sink=sink if er.has_sink(i, k) else None,
                                                n_splits=n_splits, k_descale=kd, v_descale=vd, window_left=w if wl == "variant" else wl, **kw)


# ---- 1. against the float64 reference, on all four cache kinds
@pytest.mark.parametrize("i,k", er.RUNS, ids=er.RUN_IDS)
def test_parity_with_the_reference(i, k):
    c = er.CASES[i]
    for fp8 in (False, True):
        ref = er.reference(i, k, fp8)
        for n_splits in c["splits"]:
            where = f"{er.RUN_IDS[er.RUNS.index((i, k))]} {'e4m3' if fp8 else 'bf16'} splits {n_splits}"
            _check(where, *_contiguous(i, k, fp8, n_splits), ref)
            if c["seqlens"]:      # (seqlens_k = None behind pages has the pages' capacity: test 2 ties it to the contiguous call)
                for P in er.PAGE_SIZES:
                    _check(f"{where} page {P}", *_paged(i, k, fp8, P, n_splits), ref)


# ---- 2. bit identity: with the shipped kernels row for row; paged with contiguous; a window that excludes no key with none
BIT_RUNS = tuple((i, k) for i in er.SLICED for k in range(len(er.VARIANTS)))


@pytest.mark.parametrize("i,k", BIT_RUNS, ids=[er.RUN_IDS[er.RUNS.index(r)] for r in BIT_RUNS])
def test_rows_are_the_shipped_kernels_rows_bit_for_bit(i, k):
    """The sibling once per group member g, on Q[:, g::G] with the same H_kv, q_len, lengths, window and explicit n_splits: its rows
    are the extend call's, bit for bit -- a row's arithmetic does not depend on its tile or its block."""
    fa, c = _fa(), er.CASES[i]
    G = c["hq"] // c["hkv"]
    mask, wl = er.VARIANTS[k]
    for fp8 in (False, True):
        Q, K, V, kd, vd, scale, lens, sink = _dev(i, fp8)
        sink = sink if er.has_sink(i, k) else None
        for n_splits in (1, 2, 7, 64):
            O, L = _contiguous(i, k, fp8, n_splits)
            for g in range(G):
                want = fa.flash_attention_2_decode(Q[:, g::G].contiguous(), K, V, lens, scale, causal=mask == "causal",
                                                   sink=None if sink is None else sink[g::G].contiguous(), n_splits=n_splits,
                                                   k_descale=kd, v_descale=vd, window_left=wl)
                _same_bits((O[:, g::G].contiguous(), L[:, g::G].contiguous()), want, (er.case_id(c), mask, wl, fp8, n_splits, g))


@pytest.mark.parametrize("i", range(len(er.CASES)), ids=er.IDS)
def test_paged_equals_contiguous_on_the_gathered_cache(i):
    c = er.CASES[i]
    for k in (0, 1, 4, 7):      # causal, full, windows 31 and 200
        for fp8 in (False, True):
            for P in er.PAGE_SIZES:
                Kp, Vp, table, cap = _pages(i, P, fp8)
                lens = er.lens_under(c, cap)
                K, V = _gather(Kp, table, lens, P), _gather(Vp, table, lens, P)
                assert K.shape[2] == cap
                for n_splits in c["splits"]:
                    got = _paged(i, k, fp8, P, n_splits)
                    _same_bits(got, _contiguous(i, k, fp8, n_splits, K=K, V=V), (er.case_id(c), k, fp8, P, n_splits))
                if not c["seqlens"] and not fp8:      # the capacity is the pages': the reference on the gathered cache
                    Q, _, _, scale, _, sink = er.inputs(i)
                    ref = er.reference64(Q, K.cpu(), V.cpu(), lens, scale, er.VARIANTS[k][0] == "causal", sink if er.has_sink(i, k) else None,
                                         er.VARIANTS[k][1])
                    _check(f"{er.case_id(c)} variant {k} page {P}", *got, ref)


@pytest.mark.parametrize("i", range(len(er.CASES)), ids=er.IDS)
def test_a_window_that_excludes_no_key_is_no_window(i):
    c = er.CASES[i]
    for fp8 in (False, True):
        for n_splits in c["splits"]:
            want = _contiguous(i, 0, fp8, n_splits, wl=None)
            for wl in (c["ncap"] - 1, c["ncap"], INT_MAX):
                _same_bits(_contiguous(i, 0, fp8, n_splits, wl=wl), want, (er.case_id(c), fp8, n_splits, wl))
            if c["seqlens"]:      # (one key short of the capacity excludes no key of these lengths either, through the window kernels)
                _same_bits(_contiguous(i, 0, fp8, n_splits, wl=c["ncap"] - 2), want, (er.case_id(c), fp8, n_splits, "cap - 2"))
            P = 96
            cap = _pages(i, P, fp8)[3]
            wantp = _paged(i, 0, fp8, P, n_splits, wl=None)
            for wl in (cap - 1, INT_MAX):
                _same_bits(_paged(i, 0, fp8, P, n_splits, wl=wl), wantp, (er.case_id(c), fp8, n_splits, wl, "paged"))


# ---- 3. garbage past the lengths and below the windows, guard bands, a NaN workspace
GARBAGE = [(i, k) for i, c in enumerate(er.CASES) if c["seqlens"] and (c["hq"], c["hkv"], c["nq"], c["d"]) in
           ((13, 1, 5, 64), (8, 2, 17, 128), (8, 2, 40, 64), (33, 1, 1, 128)) for k in (0, 1, 4, 7)]


def _filled(i, k, fp8, fill):
    """Host caches of CASES[i] with the rows at and past the length -- and below lo_b under VARIANTS[k]'s window -- set to `fill`."""
    c = er.CASES[i]
    K, V = (er.inputs_fp8(i) if fp8 else er.inputs(i))[1:3]
    where = fr.past_lengths(K.shape, c["lens"])
    if er.VARIANTS[k][1] is not None:
        where |= wr.below_window(K.shape, c["lens"], c["nq"], er.VARIANTS[k][1])
    if fp8:
        return fr.filled(K, where, fill), fr.filled(V, where, fill)
    return tuple(torch.where(where, torch.tensor(fill, dtype=torch.bfloat16), t) for t in (K, V))


def _pools(i, k, fp8, P, K, V, garbage):
    """Pools and a table of host caches K, V.  garbage: what no key was copied to is NaN, unused entries are -1 / INT_MAX, the
    entries of the pages wholly below lo_b are -1, INT_MAX, INT_MIN and n_pages in turn; otherwise zeros and entry 0."""
    c = er.CASES[i]
    img = (lambda t: t.to(torch.bfloat16)) if fp8 else (lambda t: t)
    Kp, Vp, table = pr.build(img(K), img(V), c["lens"], P, 98000 + 17 * i + P, fill=float("nan") if garbage else 0.0,
                             unused=pr.UNUSED if garbage else (0, 0))
    er.shared_pages(c, table, P)
    if garbage and er.VARIANTS[k][1] is not None:
        bad = (-1, INT_MAX, INT_MIN, Kp.shape[0])
        for n, (b, p) in enumerate(wr.pages_below(c["lens"], c["nq"], er.VARIANTS[k][1], P)):
            table[b, p] = bad[n % 4]
    if fp8:
        Kp, Vp = Kp.to(fr.E4M3), Vp.to(fr.E4M3)
    return Kp.cuda(), Vp.cuda(), table.cuda()


def _carved(n, dtype, pad, fill):
    """A tensor of n elements between two guard bands of `pad` elements holding `fill`: (the whole buffer, the view)."""
    big = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return big, big[pad:pad + n]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("i,k", GARBAGE, ids=[er.RUN_IDS[er.RUNS.index(r)] for r in GARBAGE])
def test_garbage_changes_nothing_and_the_guard_bands_stay(i, k, fp8):
    fa, c = _fa(), er.CASES[i]
    B, hq, nq, d = len(c["lens"]), c["hq"], c["nq"], c["d"]
    zero = _filled(i, k, fp8, 0x00 if fp8 else 0.0)
    fills = fr.NAN_CODES if fp8 else (float("nan"),)
    dirty = [_filled(i, k, fp8, f) for f in fills]
    ref = er.reference(i, k, fp8)
    pad = 512
    for n_splits in (1, 2, 7):
        need = fa.extend_workspace(B, hq, c["hkv"], nq, c["ncap"], d, n_splits, device="cpu", window_left=er.VARIANTS[k][1]).numel()
        assert (need > 0) == (n_splits > 1)
        want = _contiguous(i, k, fp8, n_splits, K=zero[0].cuda(), V=zero[1].cuda())
        _check(f"{er.case_id(c)} zeros splits {n_splits}", *want, ref)
        for f, (K, V) in zip(fills, dirty):
            bO, O = _carved(B * hq * nq * d, torch.int16, pad, SENT16)
            bL, L = _carved(B * hq * nq, torch.int32, pad, SENT32)
            bW, W = _carved(max(need // 4, 64), torch.float32, pad, float("nan"))      # the workspace starts as NaNs
            got = _contiguous(i, k, fp8, n_splits, K=K.cuda(), V=V.cuda(), O=O.view(torch.bfloat16).view(B, hq, nq, d),
                              L=L.view(torch.float32).view(B, hq, nq), workspace=W.view(torch.uint8))
            _same_bits(got, want, (er.case_id(c), n_splits, f))
            assert not (O == SENT16).any() and not (L == SENT32).any()      # every element written, sequences without keys included
            for big, sent in ((bO, SENT16), (bL, SENT32)):
                assert (big[:pad] == sent).all() and (big[-pad:] == sent).all()
            assert torch.isnan(bW[:pad]).all() and torch.isnan(bW[-pad:]).all() and torch.isnan(W[need // 4:]).all()
    for P in er.PAGE_SIZES:
        clean = _pools(i, k, fp8, P, *zero, garbage=False)
        nasty = _pools(i, k, fp8, P, *dirty[0], garbage=True)
        assert not torch.equal(clean[2], nasty[2])
        for n_splits in (1, 2, 7):
            want = _paged(i, k, fp8, P, n_splits, pools=clean)
            _check(f"{er.case_id(c)} page {P} zeros splits {n_splits}", *want, ref)
            _same_bits(_paged(i, k, fp8, P, n_splits, pools=nasty), want, (er.case_id(c), P, n_splits, "garbage"))


# ---- 4. one captured graph of {append, extend}
def test_one_captured_graph_of_append_and_extend_serves_growing_lengths():
    """Paged bf16, 17 tokens per step on 8 heads over 2 (M = 68), pages of 32 keys, window_left = 200, two splits.  Captured once
    with a caller workspace, O, L and static source buffers; between the three replays the lengths are bumped IN PLACE: sequence 0
    goes 127 -> 144 -> 161 (across the 128-key boundary, into its fifth and sixth page), sequence 1 goes 38 -> 55 -> 72 (into its
    third page).  Every replay is bit for bit the eager calls and inside the gates of the float64 reference."""
    fa = _fa()
    hq, hkv, nq, d, P, wl, B, max_pages = 8, 2, 17, 128, 32, 200, 2, 8
    n_pages = B * max_pages + 3
    g = torch.Generator().manual_seed(9700)
    rnd = lambda *shape: (torch.rand(*shape, generator=g) - 0.5).bfloat16()
    lens_host = [110, 21]                                      # before the first append
    logical_K, logical_V = rnd(B, hkv, max_pages * P, d), rnd(B, hkv, max_pages * P, d)
    table_host = torch.randperm(n_pages, generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
    Kp, Vp = (torch.full((n_pages, hkv, P, d), float("nan"), dtype=torch.bfloat16) for _ in range(2))
    for b in range(B):
        for p in range(pr.pages_for(lens_host[b], P)):
            rows = min(P, lens_host[b] - p * P)
            Kp[table_host[b, p], :, :rows] = logical_K[b, :, p * P:p * P + rows]
            Vp[table_host[b, p], :, :rows] = logical_V[b, :, p * P:p * P + rows]
    Kp, Vp, table = Kp.cuda(), Vp.cuda(), table_host.cuda()
    lens = torch.tensor(lens_host, dtype=torch.int32, device="cuda")
    Q = torch.empty(B, hq, nq, d, dtype=torch.bfloat16, device="cuda")
    kn, vn = (torch.empty(B, hkv, nq, d, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device="cuda")
    ws = fa.extend_workspace(B, hq, hkv, nq, max_pages * P, d, 2, window_left=wl)
    assert ws.numel() > 0
    sink = dr.sink_of(hq, 97).cuda()

    def step(Kp, Vp, O, L, ws):
        fa.kv_cache_append_paged(kn, vn, Kp, Vp, table, lens)
        return fa.flash_attention_2_extend_paged(Q, Kp, Vp, table, lens, sink=sink, n_splits=2, O=O, L=L, workspace=ws, window_left=wl)

    # the kernels' code objects load outside the capture, on scratch copies
    for t in (Q, kn, vn):
        t.zero_()
    lens += nq
    step(Kp.clone(), Vp.clone(), torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))
    lens -= nq
    torch.cuda.synchronize()
    eager = [Kp.clone(), Vp.clone()]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(Kp, Vp, O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(Kp.view(torch.int16), eager[0].view(torch.int16))      # the capture launched nothing
    for s in range(3):
        lens += nq                                             # 127 38 | 144 55 | 161 72
        lens_host = [n + nq for n in lens_host]
        q, k, v = rnd(B, hq, nq, d), rnd(B, hkv, nq, d), rnd(B, hkv, nq, d)
        Q.copy_(q.cuda()), kn.copy_(k.cuda()), vn.copy_(v.cuda())
        for b, n in enumerate(lens_host):
            logical_K[b, :, n - nq:n], logical_V[b, :, n - nq:n] = k[b], v[b]
        O.view(torch.int16).fill_(SENT16)
        L.view(torch.int32).fill_(SENT32)
        graph.replay()
        torch.cuda.synchronize()
        Oe, Le = step(*eager, torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))
        torch.cuda.synchronize()
        for got, want in zip((Kp, Vp), eager):
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("pool", s)
        _same_bits((O, L), (Oe, Le), ("replay", s))
        _check(f"replay {s} lens {lens_host}", O, L, er.reference64(q, logical_K, logical_V, lens_host, 1.0 / d ** 0.5, True, sink.cpu(), wl))
    assert lens_host == [161, 72]


# ---- 5. routing: at most 32 rows per K/V head is the sibling's call, its default split count included
ROUTED = [i for i, c in enumerate(wr.CASES) if (c["hq"], c["hkv"]) == (8, 2) and c["wl"] in (31, 200)]


@pytest.mark.parametrize("i", ROUTED, ids=[wr.IDS[i] for i in ROUTED])
def test_at_most_32_rows_is_the_shipped_call(i):
    fa, c = _fa(), wr.CASES[i]
    assert c["hq"] // c["hkv"] * c["nq"] <= 32
    for fp8 in (False, True):
        if fp8:
            Q, K, V, kd, vd, scale, lens, sink = _cuda(wr.inputs_fp8(i))
        else:
            Q, K, V, scale, lens, sink = _cuda(wr.inputs(i))
            kd = vd = None
        Kp, Vp, table, cap = wr.paged_inputs(i, 96, fp8)
        Kp, Vp, table = Kp.cuda(), Vp.cuda(), table.cuda()
        for wl in (None, c["wl"]):
            kw = dict(causal=True, sink=sink, k_descale=kd, v_descale=vd, window_left=wl)
            assert fa.extend_num_splits(len(c["lens"]), c["hq"], c["hkv"], c["nq"], wr.N_CAP, c["d"], window_left=wl) == \
                fa.decode_num_splits(len(c["lens"]), c["hkv"], wr.N_CAP, c["d"], q_len=c["nq"], window_left=wl)
            for n_splits in (0, 2):
                _same_bits(fa.flash_attention_2_extend(Q, K, V, lens, scale, n_splits=n_splits, **kw),
                           fa.flash_attention_2_decode(Q, K, V, lens, scale, n_splits=n_splits, **kw), (wr.IDS[i], fp8, wl, n_splits))
                _same_bits(fa.flash_attention_2_extend_paged(Q, Kp, Vp, table, lens, scale, n_splits=n_splits, **kw),
                           fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, n_splits=n_splits, **kw),
                           (wr.IDS[i], fp8, wl, n_splits, "paged"))
