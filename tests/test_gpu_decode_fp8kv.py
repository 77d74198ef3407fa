"""GPU: decode attention over fp8 (OCP e4m3) KV caches, contiguous and paged (fa2_forward_decode_fp8kv and
fa2_forward_decode_paged_fp8kv through flash_attention_2_decode / flash_attention_2_decode_paged with torch.float8_e4m3fn caches and
per-head descales).

Inputs, references and gates are tests/decode_fp8kv_ref.py's: decode_ref's cases with the caches quantised per K/V head, the
float64 reference ON THE DEQUANTISED VALUES, decode_ref's own gates (O rel-L2 <= 5e-3; |dL| <= 1e-4 up to |L| = 25, <= 1e-3 above;
the -inf rows exact) and, PER ROW, |O_i - O_ref,i| <= KAPPA u sqrt(sum_j P_ij^2 |v_j|^2) + u |O_i| on the dequantised values
(tests/decode_rows_ref.py; the worst ratio is printed with its (sequence, head, token)).  Quantisation error is in no gate; tests/test_decode_fp8kv_reference.py certifies on the CPU that the
kernels' data flow on these values stays inside the gates.  Everything else is bit equality: paged against contiguous, garbage
against zeros, descales against a folded scale, a replayed graph against an eager call, and every e4m3 code against its value."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A      # bf16 / fp32 1.5e16: nothing these inputs produce
E4M3 = torch.float8_e4m3fn
PAGES = (32, 96, 256)


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _cuda(ts):
    return tuple(t.cuda() if isinstance(t, torch.Tensor) else t for t in ts)


@functools.lru_cache(maxsize=None)
def _case_dev(i):
    return _cuda(fr.inputs(i))


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _keyless(lens, nq, causal):
    return np.array([[[n == 0 or (causal and q + n - nq < 0) for q in range(nq)]] for n in lens])


def _check(where, lens, nq, causal, O, L, ref):
    O, L = O.float().cpu().numpy(), L.cpu().numpy()
    e = dr.errors(O, L, ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    assert (O[np.broadcast_to(_keyless(lens, nq, causal), L.shape)] == 0).all(), (where, "O of a row without a key")
    rows.check(where, O, ref)


# ---- 1. against the float64 reference on the dequantised caches
@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=[dr.case_id(c) for c in dr.CASES])
def test_against_the_float64_reference(i):
    fa, c = _fa(), dr.CASES[i]
    Q, K8, V8, kd, vd, scale, lens, sink = _case_dev(i)
    assert len(set(kd.tolist())) == c["hkv"] and len(set(vd.tolist())) == c["hkv"]      # a descale of its own per head
    ref = fr.reference(i)
    for n_splits in c["splits"]:
        O, L = fa.flash_attention_2_decode(Q, K8, V8, lens if c["seqlens"] else None, scale, causal=c["causal"], sink=sink,
                                           n_splits=n_splits, k_descale=kd, v_descale=vd)
        _check(f"{dr.case_id(c)} splits {n_splits}", c["lens"], c["nq"], c["causal"], O, L, ref)


# ---- 2. paged equals contiguous
@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("i", pr.BIT_CASES, ids=[dr.case_id(dr.CASES[i]) for i in pr.BIT_CASES])
def test_paged_equals_contiguous_on_the_gathered_cache(i, P):
    fa, c = _fa(), dr.CASES[i]
    Q, _, _, kd, vd, scale, _, sink = _case_dev(i)
    Kp, Vp, table, lens, cap, _ = fr.paged_inputs(i, P)
    K, V = fr.gather(Kp, table, lens, P).cuda(), fr.gather(Vp, table, lens, P).cuda()
    Kp, Vp, table = Kp.cuda(), Vp.cuda(), table.cuda()
    assert K.shape[2] == cap
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda") if c["seqlens"] else None
    for n_splits in pr.SPLITS:
        kw = dict(causal=c["causal"], sink=sink, n_splits=n_splits, k_descale=kd, v_descale=vd)
        got = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens_dev, scale, **kw)
        _same_bits(got, fa.flash_attention_2_decode(Q, K, V, lens_dev, scale, **kw), (dr.case_id(c), P, n_splits))
        assert not torch.isnan(got[0].float()).any()


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("P", PAGES)
def test_lengths_at_the_edges_of_a_page(P, d):
    fa, c = _fa(), pr.edge_case(P, d)
    Q, Kp, Vp, table, kd, vd, scale, lens, sink = fr.edge_inputs(P, d)
    K, V = fr.gather(Kp, table, lens.tolist(), P), fr.gather(Vp, table, lens.tolist(), P)
    ref = pr.reference64(Q, fr.dequantise(K, kd), fr.dequantise(V, vd), lens.tolist(), scale, True, sink)
    Q, Kp, Vp, table, kd, vd, lens, sink, K, V = _cuda((Q, Kp, Vp, table, kd, vd, lens, sink, K, V))
    for n_splits in pr.SPLITS:
        kw = dict(causal=True, sink=sink, n_splits=n_splits, k_descale=kd, v_descale=vd)
        got = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, **kw)
        _same_bits(got, fa.flash_attention_2_decode(Q, K, V, lens, scale, **kw), (P, d, n_splits))
        _check(f"edges d{d} page {P} splits {n_splits}", c["lens"], c["nq"], True, *got, ref)


# ---- 3. garbage
@pytest.mark.parametrize("i", pr.GARBAGE_CASES, ids=[dr.case_id(dr.CASES[i]) for i in pr.GARBAGE_CASES])
def test_garbage_past_the_lengths_changes_nothing(i):
    """Contiguous caches: the rows at and beyond each length hold 0x7F (NaN), 0xFF (NaN) or 0x7E (448) against zeros."""
    fa, c = _fa(), dr.CASES[i]
    Q, K8, V8, kd, vd, scale, lens, sink = _case_dev(i)
    past = fr.past_lengths(K8.shape, c["lens"]).cuda()
    assert past.any()

    def run(byte, n_splits):
        return fa.flash_attention_2_decode(Q, fr.filled(K8, past, byte), fr.filled(V8, past, byte), lens, scale, causal=c["causal"],
                                           sink=sink, n_splits=n_splits, k_descale=kd, v_descale=vd)

    for n_splits in (0, 1, 7):
        want = run(0, n_splits)
        assert not torch.isnan(want[0].float()).any()
        for byte in fr.GARBAGE_BYTES:
            _same_bits(run(byte, n_splits), want, (n_splits, hex(byte)))


@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("i", pr.GARBAGE_CASES, ids=[dr.case_id(dr.CASES[i]) for i in pr.GARBAGE_CASES])
def test_garbage_in_the_table_and_in_the_pool_changes_nothing(i, P):
    """Pools: the tail of each last page and every unused page hold 0x7F, 0xFF or 0x7E and the unused table entries -1 /
    0x7fffffff, against zeros in both."""
    fa, c = _fa(), dr.CASES[i]
    Q, _, _, kd, vd, scale, lens_dev, sink = _case_dev(i)
    Kp, Vp, table, lens, _, unused = _cuda(fr.paged_inputs(i, P))
    zero_table = table.clone()
    for b, n in enumerate(lens):
        zero_table[b, pr.pages_for(n, P):] = 0
    assert not torch.equal(zero_table, table) and unused.any()

    def run(byte, tbl, n_splits):
        return fa.flash_attention_2_decode_paged(Q, fr.filled(Kp, unused, byte), fr.filled(Vp, unused, byte), tbl, lens_dev, scale,
                                                 causal=c["causal"], sink=sink, n_splits=n_splits, k_descale=kd, v_descale=vd)

    for n_splits in (0, 1, 7):
        want = run(0, zero_table, n_splits)
        assert not torch.isnan(want[0].float()).any()
        _same_bits(run(0, table, n_splits), want, (n_splits, "table"))
        for byte in fr.GARBAGE_BYTES:
            _same_bits(run(byte, table, n_splits), want, (n_splits, hex(byte)))


# ---- 4. every e4m3 code is read as its value
def _codes(d):
    """uint8 [4, 1, 1, d]: row b holds the codes 64 b .. 64 b + 63 (repeated at d = 128), the two NaN codes replaced by 0."""
    codes = (64 * torch.arange(4)[:, None] + torch.arange(d)[None, :] % 64).to(torch.uint8)
    for nan in fr.NAN_CODES:
        codes[codes == nan] = 0
    assert len(set(codes.flatten().tolist())) == 254
    return codes.view(4, 1, 1, d)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("d", [64, 128])
def test_every_code_of_v_is_read_as_its_value(d, paged):
    """One key, P = 1: O is V's row.  Bit for bit V8.to(bfloat16), where the code 0x80 (-0) gives +0: the accumulator starts at +0
    and 0 + (-0) is +0."""
    fa, cap = _fa(), 64
    V8 = torch.zeros(4, 1, cap, d, dtype=torch.uint8)
    V8[:, :, :1] = _codes(d)
    V8 = V8.view(E4M3).cuda()
    K8 = torch.zeros_like(V8)
    Q = torch.ones(4, 1, 1, d, dtype=torch.bfloat16, device="cuda")
    lens = torch.ones(4, dtype=torch.int32, device="cuda")
    if paged:      # one page of 64 keys per sequence, in reverse order
        table = torch.tensor([[3], [2], [1], [0]], dtype=torch.int32, device="cuda")
        O, L = fa.flash_attention_2_decode_paged(Q, K8.flip(0).contiguous(), V8.flip(0).contiguous(), table, lens, n_splits=1)
    else:
        O, L = fa.flash_attention_2_decode(Q, K8, V8, lens, n_splits=1)
    want = V8[:, :, :1].to(torch.bfloat16)
    want = torch.where(want == 0, torch.zeros_like(want), want)      # -0 -> +0
    assert torch.equal(O.view(torch.int16), want.view(torch.int16)), (O.float() - want.float()).abs().max()
    assert torch.equal(L, torch.zeros_like(L))


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("d", [64, 128])
def test_every_code_of_k_is_read_as_its_value(d, paged):
    """One key, 32 query heads on one K/V head, softmax_scale 1, row j's query the one-hot e_(c0 + j): L of row j is the key's
    element c0 + j.  Adjacent e4m3 values differ by at least 2^-9, twenty times the gate on L."""
    fa, cap = _fa(), 64
    codes = _codes(d)
    K8 = torch.zeros(4, 1, cap, d, dtype=torch.uint8)
    K8[:, :, :1] = codes
    K8 = K8.view(E4M3).cuda()
    V8 = torch.zeros_like(K8)
    lens = torch.ones(4, dtype=torch.int32, device="cuda")
    table = torch.tensor([[3], [2], [1], [0]], dtype=torch.int32, device="cuda")
    values = codes.view(E4M3).double().view(4, d)
    for c0 in range(0, d, 32):
        Q = torch.zeros(4, 32, 1, d, dtype=torch.bfloat16)
        Q[:, torch.arange(32), 0, c0 + torch.arange(32)] = 1.0
        if paged:
            _, L = fa.flash_attention_2_decode_paged(Q.cuda(), K8.flip(0).contiguous(), V8, table, lens, 1.0, n_splits=1)
        else:
            _, L = fa.flash_attention_2_decode(Q.cuda(), K8, V8, lens, 1.0, n_splits=1)
        want = values[:, c0:c0 + 32]
        dl = (L.double().cpu().view(4, 32) - want).abs()
        small = want.abs() <= dr.L_LARGE
        print(f"d{d} columns {c0}..{c0 + 31}: max |dL| {float(dl[small].max()):.3e} (|L| <= 25) {float(dl[~small].max()):.3e} (above)")
        assert float(dl[small].max()) <= dr.L_ABS and float(dl[~small].max()) <= dr.L_ABS_LARGE, (d, c0)


# ---- 5. descales fold
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_power_of_two_descales_fold_into_the_scale_and_the_output(paged):
    """k_descale = 0.5 and v_descale = 4 on every head: the call without descales at softmax_scale / 2, its O times 4 (exact in bf16),
    the same L."""
    fa = _fa()
    i, P = pr.GARBAGE_CASES[0], 96
    c = dr.CASES[i]
    Q, K8, V8, _, _, scale, lens, sink = _case_dev(i)
    kd = torch.full((c["hkv"],), 0.5, device="cuda")
    vd = torch.full((c["hkv"],), 4.0, device="cuda")
    if paged:
        Kp, Vp, table, _, _, _ = _cuda(fr.paged_inputs(i, P))
        call = lambda s, **kw: fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, s, causal=c["causal"], sink=sink, **kw)
    else:
        call = lambda s, **kw: fa.flash_attention_2_decode(Q, K8, V8, lens, s, causal=c["causal"], sink=sink, **kw)
    for n_splits in (0, 1, 7):
        O, L = call(scale, n_splits=n_splits, k_descale=kd, v_descale=vd)
        O0, L0 = call(scale * 0.5, n_splits=n_splits)
        _same_bits((O, L), (O0 * 4, L0), n_splits)
        assert float(O.float().abs().max()) > 0
        _same_bits(call(scale, n_splits=n_splits, k_descale=kd), (O0, L0), (n_splits, "v_descale = None"))


# ---- 6. writes
def _carved(n, dtype, pad):
    """A tensor of n elements inside a larger buffer filled with the sentinel: (the buffer as integers, the view)."""
    it, sent = (torch.int16, SENT16) if dtype == torch.bfloat16 else (torch.int32, SENT32) if dtype == torch.float32 else (torch.uint8, 0x5A)
    big = torch.full((n + 2 * pad,), sent, dtype=it, device="cuda")
    return big, big[pad:pad + n].view(dtype)


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("n_splits", [1, 7])
@pytest.mark.parametrize("i", pr.GARBAGE_CASES[:2], ids=[dr.case_id(dr.CASES[i]) for i in pr.GARBAGE_CASES[:2]])
def test_every_output_element_is_written_and_nothing_else(i, n_splits, paged):
    fa, c, P = _fa(), dr.CASES[i], 96
    Q, K8, V8, kd, vd, scale, lens, sink = _case_dev(i)
    B, hq, nq, d = Q.shape
    if paged:
        Kp0, Vp0, table0, _, cap, _ = _cuda(fr.paged_inputs(i, P))
        ins = [Kp0.clone(), Vp0.clone(), table0.clone()]
        run = lambda **kw: fa.flash_attention_2_decode_paged(Q, *ins, lens, scale, causal=c["causal"], sink=sink, n_splits=n_splits,
                                                             k_descale=kd, v_descale=vd, **kw)
        before = (Kp0, Vp0, table0)
    else:
        cap = K8.shape[2]
        ins = [K8.clone(), V8.clone()]
        run = lambda **kw: fa.flash_attention_2_decode(Q, *ins, lens, scale, causal=c["causal"], sink=sink, n_splits=n_splits,
                                                       k_descale=kd, v_descale=vd, **kw)
        before = (K8, V8)
    need = fa._capi.lib().fa2_decode_workspace_bytes(B, hq, c["hkv"], nq, cap, d, n_splits)
    assert (need > 0) == (n_splits > 1)
    pad = 256
    bO, O = _carved(Q.numel(), torch.bfloat16, pad)
    bL, L = _carved(B * hq * nq, torch.float32, pad)
    bW, W = _carved(max(need, 256), torch.uint8, pad)
    run(O=O.view(B, hq, nq, d), L=L.view(B, hq, nq), workspace=W)
    torch.cuda.synchronize()
    assert not (O.view(torch.int16) == SENT16).any() and not (L.view(torch.int32) == SENT32).any()      # sequences without keys included
    for big, n, sent in ((bO, O.numel(), SENT16), (bL, L.numel(), SENT32), (bW, W.numel(), 0x5A)):
        assert (big[:pad] == sent).all() and (big[pad + n:] == sent).all()
    if need:
        assert (bW[pad + need:] == 0x5A).all()
    else:
        assert (W == 0x5A).all()      # one split touches no workspace
    for t, t0 in zip(ins, before):      # the caches (pools, table) are only read
        assert torch.equal(t.view(torch.uint8) if t.dtype == E4M3 else t, t0.view(torch.uint8) if t0.dtype == E4M3 else t0)
    _same_bits(run(), (O.view(B, hq, nq, d), L.view(B, hq, nq)), "a second run")
    ref = fr.reference(i)
    _check(f"{dr.case_id(c)} carved, splits {n_splits}", c["lens"], nq, c["causal"], O.view(B, hq, nq, d), L.view(B, hq, nq), ref)


# ---- 7. one captured graph
def test_one_captured_graph_serves_changing_lengths_table_and_descales():
    """The paged fp8 call captured once with a caller workspace, O and L; between replays seqlens_k, a table entry (a sequence grows
    into a new page) and both descale tensors change IN PLACE, and each replay is bit for bit an eager call on the new values."""
    fa = _fa()
    i, P = pr.GARBAGE_CASES[0], 64
    c = dr.CASES[i]
    Q, _, _, kd0, vd0, scale, _, sink = _case_dev(i)
    Kp, Vp, table0, lens0, cap, unused = _cuda(fr.paged_inputs(i, P))
    g = torch.Generator().manual_seed(78)      # every page holds numbers: a page a sequence grows into must not be NaN below its length
    fresh = lambda t: torch.where(unused, torch.randint(0, 0x78, t.shape, generator=g, dtype=torch.uint8).cuda(), t.view(torch.uint8)).view(E4M3)
    Kp, Vp = fresh(Kp), fresh(Vp)
    B, hq, nq, d = Q.shape
    table, lens = table0.clone(), torch.tensor(lens0, dtype=torch.int32, device="cuda")
    kd, vd = kd0.clone(), vd0.clone()
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device="cuda")
    ws = fa.decode_workspace(B, hq, c["hkv"], nq, cap, d, 0)
    assert ws.numel() > 0
    kw = dict(causal=True, sink=sink, n_splits=0, k_descale=kd, v_descale=vd)
    call = lambda: fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, O=O, L=L, workspace=ws, **kw)
    call()      # (the first launch of a kernel sets its LDS limit: not inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    used = {int(table0[b, p]) for b, n in enumerate(lens0) for p in range(pr.pages_for(n, P))}
    spare = sorted(set(range(Kp.shape[0])) - used)
    grow = next(b for b, n in enumerate(lens0) if 0 < n < cap - P and n % P)      # a sequence with a partly filled last page
    seen = []
    for step in range(3):
        new_table, new_lens = table0.cpu().clone(), list(lens0)
        if step >= 1:      # the sequence grows into a new page
            new_lens[grow] = pr.pages_for(lens0[grow], P) * P + 3
            new_table[grow, pr.pages_for(lens0[grow], P)] = spare[0]
        if step == 2:      # ... and the cache is rescaled
            kd.copy_(kd0 * 1.5)
            vd.copy_(vd0 * 0.75)
        table.copy_(new_table.cuda())
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32).cuda())
        O.view(torch.int16).fill_(SENT16)
        L.view(torch.int32).fill_(SENT32)
        graph.replay()
        torch.cuda.synchronize()
        _same_bits((O, L), fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, **kw), ("replay", step))
        assert not torch.isnan(O.float()).any()
        seen.append((O.clone(), L.clone()))
    for a, b in ((0, 1), (1, 2)):      # every change reached the kernel
        assert not torch.equal(seen[a][0], seen[b][0]) and not torch.equal(seen[a][1], seen[b][1])


# ---- 8. refusals
def test_more_than_32_rows_is_refused_and_writes_nothing():
    fa = _fa()
    lib = fa._capi.lib()
    B, hq, hkv, nq, cap, d = 1, 8, 2, 9, 320, 128      # 4 x 9 = 36 rows
    Q = torch.zeros(B, hq, nq, d, dtype=torch.bfloat16, device="cuda")
    K8 = torch.zeros(B, hkv, cap, d, dtype=torch.uint8, device="cuda").view(E4M3)
    O = torch.full((B, hq, nq, d), SENT16, dtype=torch.int16, device="cuda")
    L = torch.full((B, hq, nq), SENT32, dtype=torch.int32, device="cuda")
    ws = torch.full((lib.fa2_decode_workspace_bytes(B, hq, hkv, nq, cap, d, 2),), 0x5A, dtype=torch.uint8, device="cuda")
    for n_splits in (1, 2):
        st = lib.fa2_forward_decode_fp8kv(Q.data_ptr(), K8.data_ptr(), K8.data_ptr(), None, None, None, None, O.data_ptr(), L.data_ptr(),
                                          B, hq, hkv, nq, cap, d, ctypes.c_float(0.1), 0, 2, 1, n_splits, ws.data_ptr(), ws.numel(), None)
        assert st == -6
    torch.cuda.synchronize()
    assert (O == SENT16).all() and (L == SENT32).all() and (ws == 0x5A).all()
    with pytest.raises(ValueError, match="36 rows, decode takes at most 32"):
        fa.flash_attention_2_decode(Q, K8, K8)


def test_an_fp8_k_beside_a_bf16_v_is_refused():
    fa = _fa()
    Q = torch.zeros(1, 8, 1, 128, dtype=torch.bfloat16, device="cuda")
    V = torch.zeros(1, 2, 320, 128, dtype=torch.bfloat16, device="cuda")
    K8 = torch.zeros(1, 2, 320, 128, dtype=torch.uint8, device="cuda").view(E4M3)
    with pytest.raises(ValueError, match="V_cache: dtype torch.bfloat16 beside K_cache torch.float8_e4m3fn"):
        fa.flash_attention_2_decode(Q, K8, V)
    with pytest.raises(ValueError, match="k_descale: a descale belongs to torch.float8_e4m3fn caches"):
        fa.flash_attention_2_decode(Q, V, V, k_descale=torch.ones(2, device="cuda"))
