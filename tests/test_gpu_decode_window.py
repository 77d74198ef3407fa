"""GPU: decode attention with a sliding window (fa2_forward_decode_window, fa2_forward_decode_paged_window through
flash_attention_2_decode / _paged with window_left=): bf16 and e4m3 caches, contiguous and paged.

Cases, inputs and the float64 reference are tests/decode_window_ref.py's (tests/test_decode_window_reference.py certifies on the
CPU that the reference alone stays inside the gates): N_cap = 1024, heads (8, 2) and (3, 3), d in {64, 128}, q_len in {1, 4},
window_left in {0, 1, 31, 127, 128, 200}, n_splits in {0, 1, 2, 5}; every case is one batch of the lengths 0, 1, q_len - 1,
window_left, window_left + 1, window_left + 2, the two that put lo_b at 256 and 257, and 1024.  Gates: decode_ref.within_gates
against the float64 reference (5e-3 on O rel-L2, 1e-4 / 1e-3 on |dL|), PER ROW |O_i - O_ref,i| <= KAPPA u sqrt(sum_j P_ij^2 |v_j|^2)
+ u |O_i| (tests/decode_rows_ref.py; the worst ratio is printed with its (sequence, head, token)), and bit equalities without a
tolerance.
e4m3 caches carry a distinct descale per head that is no power of two; their reference is the float64 one on the dequantised cache."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows
import decode_window_ref as wr

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A      # bf16 / fp32 1.5e16: nothing these inputs produce
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
ALL = range(len(wr.CASES))


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _cuda(ts):
    return tuple(t.cuda() if isinstance(t, torch.Tensor) else t for t in ts)


@functools.lru_cache(maxsize=4)
def _dev(i, fp8):
    """(Q, K, V, k_descale, v_descale, scale, lens, sink) on the device; the descales are None beside bf16 caches."""
    if fp8:
        return _cuda(wr.inputs_fp8(i))
    Q, K, V, scale, lens, sink = wr.inputs(i)
    return _cuda((Q, K, V, None, None, scale, lens, sink))


@functools.lru_cache(maxsize=8)
def _pages(i, P, fp8):
    Kp, Vp, table, cap = wr.paged_inputs(i, P, fp8)
    return Kp.cuda(), Vp.cuda(), table.cuda(), cap


def _gather(pool, table, lens, P):
    return fr.gather(pool, table, lens, P) if pool.dtype == fr.E4M3 else pr.gather(pool, table, lens, P)


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _keyless(lens, nq):
    """[B, 1, nq] bool: the rows that see no key (pos < 0)."""
    return np.array([[[q + n - nq < 0 for q in range(nq)]] for n in lens])


def _check(where, lens, nq, O, L, ref):
    O, L = O.float().cpu().numpy(), L.cpu().numpy()
    e = dr.errors(O, L, ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    assert (O[np.broadcast_to(_keyless(lens, nq), L.shape)] == 0).all(), (where, "O of a row without a key")
    rows.check(where, O, ref)


def _contiguous(i, fp8, n_splits, wl="case", K=None, V=None, **kw):
    Q, K0, V0, kd, vd, scale, lens, sink = _dev(i, fp8)
    wl = wr.CASES[i]["wl"] if wl == "case" else wl
    return _fa().flash_attention_2_decode(Q, K0 if K is None else K, V0 if V is None else V, lens, scale, causal=True, sink=sink,
                                          n_splits=n_splits, k_descale=kd, v_descale=vd, window_left=wl, **kw)


def _paged(i, fp8, P, n_splits, wl="case", pools=None, **kw):
    Q, _, _, kd, vd, scale, lens, sink = _dev(i, fp8)
    Kp, Vp, table = pools if pools is not None else _pages(i, P, fp8)[:3]
    wl = wr.CASES[i]["wl"] if wl == "case" else wl
    return _fa().flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, causal=True, sink=sink, n_splits=n_splits,
                                                k_descale=kd, v_descale=vd, window_left=wl, **kw)


# ---- 1. parity with the float64 reference; 2c. paged == contiguous on the gathered cache, bit for bit
@pytest.mark.parametrize("i", ALL, ids=wr.IDS)
def test_parity_with_the_reference(i):
    c = wr.CASES[i]
    for fp8 in (False, True):
        ref = wr.reference(i, fp8)
        for n_splits in c["splits"]:
            where = f"{wr.case_id(c)} {'e4m3' if fp8 else 'bf16'} splits {n_splits}"
            _check(where, c["lens"], c["nq"], *_contiguous(i, fp8, n_splits), ref)
            for P in wr.PAGE_SIZES:
                _check(f"{where} page {P}", c["lens"], c["nq"], *_paged(i, fp8, P, n_splits), ref)


@pytest.mark.parametrize("i", ALL, ids=wr.IDS)
def test_paged_equals_contiguous_on_the_gathered_cache(i):
    c = wr.CASES[i]
    for fp8 in (False, True):
        for P in wr.PAGE_SIZES:
            Kp, Vp, table, cap = _pages(i, P, fp8)
            K, V = _gather(Kp, table, c["lens"], P), _gather(Vp, table, c["lens"], P)
            assert K.shape[2] == cap
            for n_splits in c["splits"]:
                _same_bits(_paged(i, fp8, P, n_splits), _contiguous(i, fp8, n_splits, K=K, V=V), (wr.case_id(c), fp8, P, n_splits))


# ---- 2a. no window, and a window that excludes no key of the capacity, are today's call
PLAIN_CASES = [k for k, c in enumerate(wr.CASES) if c["wl"] == 127]


@pytest.mark.parametrize("i", PLAIN_CASES, ids=[wr.IDS[k] for k in PLAIN_CASES])
def test_no_window_and_a_window_of_the_capacity_are_the_plain_call(i):
    fa, c = _fa(), wr.CASES[i]
    for fp8 in (False, True):
        Q, K, V, kd, vd, scale, lens, sink = _dev(i, fp8)
        for n_splits in c["splits"]:
            want = fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=True, sink=sink, n_splits=n_splits, k_descale=kd, v_descale=vd)
            for wl in (None, wr.N_CAP - 1, wr.N_CAP, INT_MAX):
                _same_bits(_contiguous(i, fp8, n_splits, wl=wl), want, (wr.case_id(c), fp8, n_splits, wl))
            for P in wr.PAGE_SIZES:
                Kp, Vp, table, cap = _pages(i, P, fp8)
                wantp = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, causal=True, sink=sink, n_splits=n_splits,
                                                          k_descale=kd, v_descale=vd)
                for wl in (None, cap - 1, cap, INT_MAX):
                    _same_bits(_paged(i, fp8, P, n_splits, wl=wl), wantp, (wr.case_id(c), fp8, P, n_splits, wl))
    # (and a window one key short of that does exclude one: the full sequence's last row loses key 0)
    got, want = _contiguous(i, False, 1, wl=wr.N_CAP - 2), _contiguous(i, False, 1, wl=None)
    full = c["lens"].index(wr.N_CAP)
    assert not torch.equal(got[1][full], want[1][full])


# ---- 2b. lo_b a multiple of 128, one query: the plain call on the cache rows from lo_b on
Q1_CASES = [k for k, c in enumerate(wr.CASES) if c["nq"] == 1]


@pytest.mark.parametrize("i", Q1_CASES, ids=[wr.IDS[k] for k in Q1_CASES])
def test_aligned_window_is_the_plain_call_on_the_rows_from_lo(i):
    fa, c = _fa(), wr.CASES[i]
    seen = 0
    for fp8 in (False, True):
        Q, K, V, kd, vd, scale, lens, sink = _dev(i, fp8)
        for n_splits in (1, 2, 5):
            O, L = _contiguous(i, fp8, n_splits)
            for b, n in enumerate(c["lens"]):
                lo = wr.lo_of(n, 1, c["wl"])
                if lo == 0 or lo % wr.KB:
                    continue
                seen += 1
                sub = torch.tensor([n - lo], dtype=torch.int32, device="cuda")
                want = fa.flash_attention_2_decode(Q[b:b + 1], K[b:b + 1, :, lo:].contiguous(), V[b:b + 1, :, lo:].contiguous(), sub, scale,
                                                   causal=True, sink=sink, n_splits=n_splits, k_descale=kd, v_descale=vd)
                _same_bits((O[b:b + 1], L[b:b + 1]), want, (wr.case_id(c), fp8, n_splits, b, lo))
    assert seen >= 6      # the length that puts lo_b at 256, both element sizes, three split counts


# ---- 3. garbage before the window (and past the length) changes nothing
def _filled(i, fp8, fill):
    """Host caches of CASES[i] with the rows below lo_b and the rows at and past the length set to `fill` (a float beside bf16
    caches, a byte beside e4m3 ones)."""
    c = wr.CASES[i]
    K, V = (wr.inputs_fp8(i) if fp8 else wr.inputs(i))[1:3]
    where = wr.below_window(K.shape, c["lens"], c["nq"], c["wl"]) | fr.past_lengths(K.shape, c["lens"])
    if fp8:
        return fr.filled(K, where, fill), fr.filled(V, where, fill)
    return tuple(torch.where(where, torch.tensor(fill, dtype=torch.bfloat16), t) for t in (K, V))


def _pools(i, fp8, P, K, V, garbage):
    """Pools and a table of host caches K, V (decode_paged_ref.build with the case's own seed: the same pages whatever they hold).
    garbage: what no key was copied to is NaN, unused entries are -1 / INT_MAX, and the entries of the pages wholly below lo_b are
    -1, INT_MAX, INT_MIN and n_pages in turn; otherwise zeros and entry 0 / the pages' own entries."""
    c = wr.CASES[i]
    img = (lambda t: t.to(torch.bfloat16)) if fp8 else (lambda t: t)
    Kp, Vp, table = pr.build(img(K), img(V), c["lens"], P, 87000 + 17 * i + P, fill=float("nan") if garbage else 0.0,
                             unused=pr.UNUSED if garbage else (0, 0))
    if garbage:
        bad = (-1, INT_MAX, INT_MIN, Kp.shape[0])
        for k, (b, p) in enumerate(wr.pages_below(c["lens"], c["nq"], c["wl"], P)):
            table[b, p] = bad[k % 4]
    if fp8:
        Kp, Vp = Kp.to(fr.E4M3), Vp.to(fr.E4M3)
    return Kp.cuda(), Vp.cuda(), table.cuda()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("i", ALL, ids=wr.IDS)
def test_garbage_before_the_window_changes_nothing(i, fp8):
    c = wr.CASES[i]
    assert wr.pages_below(c["lens"], c["nq"], c["wl"], 32)
    zero = _filled(i, fp8, 0x00 if fp8 else 0.0)
    fills = fr.GARBAGE_BYTES if fp8 else (float("nan"), 3e38)
    dirty = [_filled(i, fp8, f) for f in fills]
    for n_splits in (1, 2, 5):
        want = _contiguous(i, fp8, n_splits, K=zero[0].cuda(), V=zero[1].cuda())
        _check(f"{wr.case_id(c)} zeros splits {n_splits}", c["lens"], c["nq"], *want, wr.reference(i, fp8))
        for f, (K, V) in zip(fills, dirty):
            _same_bits(_contiguous(i, fp8, n_splits, K=K.cuda(), V=V.cuda()), want, (wr.case_id(c), n_splits, f))
    for P in wr.PAGE_SIZES:
        clean = _pools(i, fp8, P, *zero, garbage=False)
        # NaN rows below lo_b: the pages wholly below it are NaN throughout, and so is the straddling page below lo_b
        nasty = _pools(i, fp8, P, *dirty[0], garbage=True)
        assert not torch.equal(clean[2], nasty[2])
        for n_splits in (1, 2, 5):
            want = _paged(i, fp8, P, n_splits, pools=clean)
            _same_bits(want, _contiguous(i, fp8, n_splits, K=_gather(clean[0], clean[2], c["lens"], P), V=_gather(clean[1], clean[2], c["lens"], P)),
                       (wr.case_id(c), P, n_splits, "gathered"))
            _same_bits(_paged(i, fp8, P, n_splits, pools=nasty), want, (wr.case_id(c), P, n_splits, "garbage"))


# ---- 4. rows without a key, and the sink
@pytest.mark.parametrize("d", [64, 128])
def test_keyless_rows_and_a_sink_on_every_head(d):
    """A GPT-OSS-shaped layer: window_left = 127 (sliding_window = 128), grouped heads, a sink on EVERY head; and the same without
    one.  Sequences shorter than q_len have rows with pos < 0: O = 0 and L = sink[h], or -inf."""
    fa = _fa()
    i = next(k for k, c in enumerate(wr.CASES) if (c["hq"], c["hkv"], c["d"], c["nq"], c["wl"]) == (8, 2, d, 4, 127))
    c = wr.CASES[i]
    full = (torch.arange(c["hq"], dtype=torch.float32) * 0.75 - 1.5)
    keyless = torch.from_numpy(np.broadcast_to(_keyless(c["lens"], c["nq"]), (len(c["lens"]), c["hq"], c["nq"])).copy())
    assert keyless.any() and not keyless.all()
    for fp8 in (False, True):
        Q, K, V, kd, vd, scale, lens, _ = _dev(i, fp8)
        Kh, Vh = wr.dequantised(i) if fp8 else wr.inputs(i)[1:3]
        for sink in (full, None):
            ref = wr.reference64(wr.inputs(i)[0], Kh, Vh, c["lens"], scale, sink, 127)
            sd = None if sink is None else sink.cuda()
            runs = [(f"contiguous splits {s}", fa.flash_attention_2_decode(Q, K, V, lens, scale, sink=sd, n_splits=s, k_descale=kd, v_descale=vd,
                                                                           window_left=127)) for s in (0, 1, 2, 5)]
            Kp, Vp, table, _ = _pages(i, 32, fp8)
            runs += [(f"paged splits {s}", fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, sink=sd, n_splits=s, k_descale=kd,
                                                                             v_descale=vd, window_left=127)) for s in (1, 5)]
            for what, (O, L) in runs:
                _check(f"d{d} {'e4m3' if fp8 else 'bf16'} {'sink' if sink is not None else 'no sink'} {what}", c["lens"], c["nq"], O, L, ref)
                O, L = O.cpu(), L.cpu()
                assert (O[keyless] == 0).all()
                want = torch.full_like(L, -np.inf) if sink is None else sink[None, :, None].expand_as(L)
                assert torch.equal(L[keyless], want[keyless]), what
                assert torch.isfinite(L[~keyless]).all()


# ---- 5. writes
def _carved(n, dtype, pad):
    """A tensor of n elements inside a larger buffer filled with random bytes: (the buffer as bytes, a copy of it, the view)."""
    size = torch.empty((), dtype=dtype).element_size()
    big = torch.randint(0, 256, ((n + 2 * pad) * size,), dtype=torch.uint8, device="cuda")
    return big, big.clone(), big[pad * size:(pad + n) * size].view(dtype)


@pytest.mark.parametrize("n_splits", [1, 5])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("i", [k for k, c in enumerate(wr.CASES) if c["hq"] == 8 and c["nq"] == 4 and c["wl"] in (31, 200)],
                         ids=lambda k: wr.IDS[k])
def test_every_output_element_is_written_and_nothing_else(i, paged, n_splits):
    fa, c = _fa(), wr.CASES[i]
    Q, K, V, _, _, scale, lens, sink = _dev(i, False)
    B, hq, nq, d = Q.shape
    P = 96
    Kp, Vp, table, cap = _pages(i, P, False)
    cap = cap if paged else wr.N_CAP
    need = fa.decode_workspace(B, hq, c["hkv"], nq, cap, d, n_splits, device="cpu", q_len=nq, window_left=c["wl"]).numel()
    assert (need > 0) == (n_splits > 1)
    pad = 256
    bO, bO0, O = _carved(Q.numel(), torch.bfloat16, pad)
    bL, bL0, L = _carved(B * hq * nq, torch.float32, pad)
    bW, bW0, W = _carved(max(need, 256), torch.uint8, pad)
    # the outputs start dirty: a pattern no result holds, so an element left unwritten shows
    O.view(torch.int16).fill_(SENT16)
    L.view(torch.int32).fill_(SENT32)
    kw = dict(O=O.view(B, hq, nq, d), L=L.view(B, hq, nq), workspace=W)
    if paged:
        srcs = [t.clone() for t in (Kp, Vp, table)]
        _paged(i, False, P, n_splits, pools=srcs, **kw)
        orig = (Kp, Vp, table)
    else:
        srcs = [K.clone(), V.clone()]
        _contiguous(i, False, n_splits, K=srcs[0], V=srcs[1], **kw)
        orig = (K, V)
    torch.cuda.synchronize()
    assert not (O.view(torch.int16) == SENT16).any() and not (L.view(torch.int32) == SENT32).any()      # sequences without keys included
    for big, big0, n, size in ((bO, bO0, O.numel(), 2), (bL, bL0, L.numel(), 4), (bW, bW0, W.numel(), 1)):
        assert torch.equal(big[:pad * size], big0[:pad * size]) and torch.equal(big[(pad + n) * size:], big0[(pad + n) * size:])
    assert torch.equal(bW[pad + need:], bW0[pad + need:])      # nothing beyond the bytes the call asked for (none with one split)
    for got, want in zip(srcs, orig):      # the caches, the pools and the table are only read (compared as bytes: the pool holds NaNs)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    _check(f"{wr.case_id(c)} carved {'paged' if paged else 'contiguous'} splits {n_splits}", c["lens"], nq, O.view(B, hq, nq, d),
           L.view(B, hq, nq), wr.reference(i))


# ---- 6. one captured graph of append + windowed decode
def test_one_captured_graph_serves_a_growing_length_and_a_sliding_window():
    """Paged bf16, one token per step, window_left = 31, pages of 32 keys.  Captured once on one stream with a caller workspace, O, L
    and static source buffers; between the four replays the lengths are bumped IN PLACE.  Sequence 0 (63 keys at the first
    replay) grows into its third page at the third replay and its lo_b reaches 32 at the second: from then on its first page is
    behind the window, and its table entry is overwritten with -1 and its rows with NaN.  Sequence 1 (95 keys at the first replay,
    its first page already behind the window) sees its lo_b reach 64 at the second replay, where its second page falls behind,
    and grows into its fourth page at the third.  Every replay is checked against the float64 reference on a host copy of the
    logical caches, and is bit for bit the eager calls."""
    fa = _fa()
    hq, hkv, d, P, wl, B, max_pages = 8, 2, 128, 32, 31, 2, 4
    n_pages = 11
    g = torch.Generator().manual_seed(9100)
    rnd = lambda *shape: (torch.rand(*shape, generator=g) - 0.5).bfloat16()
    lens_host = [62, 94]                                       # before the first append
    logical_K, logical_V = rnd(B, hkv, max_pages * P, d), rnd(B, hkv, max_pages * P, d)
    table_host = torch.tensor([[7, 2, 9, 4], [5, 0, 3, 8]], dtype=torch.int32)
    Kp, Vp = (torch.full((n_pages, hkv, P, d), float("nan"), dtype=torch.bfloat16) for _ in range(2))
    for b in range(B):
        for p in range(pr.pages_for(lens_host[b], P)):
            rows = min(P, lens_host[b] - p * P)
            Kp[table_host[b, p], :, :rows] = logical_K[b, :, p * P:p * P + rows]
            Vp[table_host[b, p], :, :rows] = logical_V[b, :, p * P:p * P + rows]
    Kp, Vp, table = Kp.cuda(), Vp.cuda(), table_host.cuda()
    lens = torch.tensor(lens_host, dtype=torch.int32, device="cuda")
    Q = torch.empty(B, hq, 1, d, dtype=torch.bfloat16, device="cuda")
    kn, vn = (torch.empty(B, hkv, 1, d, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    O, L = torch.empty_like(Q), torch.empty(B, hq, 1, dtype=torch.float32, device="cuda")
    ws = fa.decode_workspace(B, hq, hkv, 1, max_pages * P, d, 2, q_len=1, window_left=wl)
    assert ws.numel() > 0
    sink = dr.sink_of(hq, 91).cuda()

    def step(Kp, Vp, O, L, ws):
        fa.kv_cache_append_paged(kn, vn, Kp, Vp, table, lens)
        return fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, sink=sink, n_splits=2, O=O, L=L, workspace=ws, window_left=wl)

    # the kernels' code objects load outside the capture, on scratch copies (the lengths are not bumped yet: row 61 / 93 of a copy)
    for t in (Q, kn, vn):
        t.zero_()
    step(Kp.clone(), Vp.clone(), torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))
    torch.cuda.synchronize()
    eager = [Kp.clone(), Vp.clone()]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(Kp, Vp, O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    # (the capture launched nothing: the pools are untouched)
    assert torch.equal(Kp.view(torch.int16), eager[0].view(torch.int16))
    freed = []
    for s in range(4):
        lens += 1                                              # 63 95 | 64 96 | 65 97 | 66 98
        lens_host = [n + 1 for n in lens_host]
        q, k, v = rnd(B, hq, 1, d), rnd(B, hkv, 1, d), rnd(B, hkv, 1, d)
        Q.copy_(q.cuda()), kn.copy_(k.cuda()), vn.copy_(v.cuda())
        for b, n in enumerate(lens_host):
            logical_K[b, :, n - 1], logical_V[b, :, n - 1] = k[b, :, 0], v[b, :, 0]
            for p in range(wr.lo_of(n, 1, wl) // P):           # the pages wholly behind the window: freed
                if (b, p) not in freed:
                    freed.append((b, p))
                    page = int(table_host[b, p])
                    for pools in ((Kp, Vp), eager):
                        for pool in pools:
                            pool[page] = float("nan")
                    table[b, p] = -1
        O.view(torch.int16).fill_(SENT16)
        L.view(torch.int32).fill_(SENT32)
        graph.replay()
        torch.cuda.synchronize()
        Oe, Le = step(*eager, torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))
        torch.cuda.synchronize()
        for got, want in zip((Kp, Vp), eager):
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("pool", s)
        _same_bits((O, L), (Oe, Le), ("replay", s))
        ref = wr.reference64(q, logical_K, logical_V, lens_host, 1.0 / d ** 0.5, sink.cpu(), wl)
        _check(f"replay {s} lens {lens_host} freed {freed}", lens_host, 1, O, L, ref)
    assert freed == [(1, 0), (0, 0), (1, 1)]
    assert lens_host == [66, 98]


# ---- 7. refusals
def test_refusals_write_nothing():
    fa = _fa()
    lib = fa._capi.lib()
    B, hq, hkv, P, max_pages, d, n_pages = 1, 8, 2, 64, 5, 128, 7
    ncap = max_pages * P
    Kp = torch.zeros(n_pages, hkv, P, d, dtype=torch.bfloat16, device="cuda")
    Kc = torch.zeros(B, hkv, ncap, d, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(B, max_pages, dtype=torch.int32, device="cuda")
    for nq, causal in ((9, 1), (1, 0), (9, 0)):      # 4 x 9 = 36 rows; a window without the causal mask; both
        Q = torch.zeros(B, hq, nq, d, dtype=torch.bfloat16, device="cuda")
        O = torch.full((B, hq, nq, d), SENT16, dtype=torch.int16, device="cuda")
        L = torch.full((B, hq, nq), SENT32, dtype=torch.int32, device="cuda")
        ws = torch.full((lib.fa2_decode_workspace_bytes(B, hq, hkv, nq, ncap, d, 2),), 0x5A, dtype=torch.uint8, device="cuda")
        for n_splits in (1, 2):
            tail = (ctypes.c_float(0.1), 0, 0, causal, n_splits, ws.data_ptr(), ws.numel(), None, 127)
            st = lib.fa2_forward_decode_window(Q.data_ptr(), Kc.data_ptr(), Kc.data_ptr(), None, None, None, None, O.data_ptr(), L.data_ptr(),
                                               B, hq, hkv, nq, ncap, d, *tail)
            assert st == -6, (nq, causal, n_splits)
            st = lib.fa2_forward_decode_paged_window(Q.data_ptr(), Kp.data_ptr(), Kp.data_ptr(), table.data_ptr(), None, None, None, None,
                                                     O.data_ptr(), L.data_ptr(), B, hq, hkv, nq, n_pages, P, max_pages, d, *tail)
            assert st == -6, (nq, causal, n_splits)
        torch.cuda.synchronize()
        assert (O == SENT16).all() and (L == SENT32).all() and (ws == 0x5A).all()
    Q = torch.zeros(B, hq, 1, d, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="window_left: 127 with causal=False"):
        fa.flash_attention_2_decode(Q, Kc, Kc, causal=False, window_left=127)
    with pytest.raises(ValueError, match="window_left: 127 with causal=False"):
        fa.flash_attention_2_decode_paged(Q, Kp, Kp, table, causal=False, window_left=127)
    with pytest.raises(ValueError, match="36 rows, decode takes at most 32"):
        fa.flash_attention_2_decode(torch.zeros(B, hq, 9, d, dtype=torch.bfloat16, device="cuda"), Kc, Kc, window_left=127)
