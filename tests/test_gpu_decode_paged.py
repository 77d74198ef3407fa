"""GPU: paged decode attention (fa2_forward_decode_paged through cuda_flashattention_amd.flash_attention_2_decode_paged): Q [B, H_q,
N_q, d] against page pools [n_pages, H_kv, page_size, d] and a block table in device memory.

THE GATE IS BIT EQUALITY with flash_attention_2_decode on the GATHERED contiguous cache of capacity max_pages * page_size and the
same n_splits: the 32-key tiles, their order and every sum are the same in both kernels, only where a tile's rows are found
differs, so O and L are compared as integers and need no tolerance.  Beside it decode_ref's gates against the float64 reference
(tests/test_decode_paged_reference.py certifies on the CPU that the reference alone stays inside them), O == 0 on every row
without a visible key, and PER ROW |O_i - O_ref,i| <= KAPPA u sqrt(sum_j P_ij^2 |v_j|^2) + u |O_i| (tests/decode_rows_ref.py; the
worst ratio is printed with its (sequence, head, token)).

Pools and tables are tests/decode_paged_ref.py's: pages assigned by a seeded permutation, the pool NaN wherever no key was copied
(the tail of each last page, every spare page), unused table entries -1 and 0x7fffffff.  Page sizes 32, 64, 96, 128, 256; splits 0
(the default), 1, 2, 7, 64; caches of at most 2592 keys, B = 9.  No test feeds an out-of-range table entry that is IN USE: that
clamp (min(max(entry, 0), n_pages - 1) in load_tile of fa2_decode.hip) is checked by reading the code."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A      # bf16 / fp32 1.5e16: nothing these inputs produce


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _cuda(ts):
    return tuple(t.cuda() if isinstance(t, torch.Tensor) else t for t in ts)


@functools.lru_cache(maxsize=None)
def _case_dev(i):
    return _cuda(dr.inputs(i))


@functools.lru_cache(maxsize=None)
def _pages_dev(i, P, fill="nan", zero_unused=False):
    Kp, Vp, table, lens, cap = pr.paged_inputs(i, P, fill, zero_unused)
    return Kp.cuda(), Vp.cuda(), table.cuda(), lens, cap


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _keyless(lens, nq, causal):
    """[B, 1, nq] bool: the rows that see no key."""
    return np.array([[[n == 0 or (causal and q + n - nq < 0) for q in range(nq)]] for n in lens])


def _check(where, lens, nq, causal, O, L, ref):
    O, L = O.float().cpu().numpy(), L.cpu().numpy()
    e = dr.errors(O, L, ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    assert (O[np.broadcast_to(_keyless(lens, nq, causal), L.shape)] == 0).all(), (where, "O of a row without a key")
    rows.check(where, O, ref)


# ---- 1. bit for bit against the contiguous kernel
@pytest.mark.parametrize("P", pr.PAGE_SIZES)
@pytest.mark.parametrize("i", pr.BIT_CASES, ids=[dr.case_id(dr.CASES[i]) for i in pr.BIT_CASES])
def test_paged_equals_contiguous_on_the_gathered_cache(i, P):
    fa, c = _fa(), dr.CASES[i]
    Q, _, _, scale, _, sink = _case_dev(i)
    Kp, Vp, table, lens, cap = _pages_dev(i, P)
    lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda") if c["seqlens"] else None
    K, V = pr.gather(Kp, table, lens, P), pr.gather(Vp, table, lens, P)
    assert K.shape[2] == cap == table.shape[1] * P
    ref = pr.paged_reference(i, P)
    for n_splits in pr.SPLITS:
        where = f"{dr.case_id(c)} page {P} splits {n_splits}"
        got = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens_dev, scale, causal=c["causal"], sink=sink, n_splits=n_splits)
        want = fa.flash_attention_2_decode(Q, K, V, lens_dev, scale, causal=c["causal"], sink=sink, n_splits=n_splits)
        _same_bits(got, want, where)
        _check(where, lens, c["nq"], c["causal"], *got, ref)


# ---- 2. page edges
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("P", pr.PAGE_SIZES)
def test_lengths_at_the_edges_of_a_page(P, d):
    fa, c = _fa(), pr.edge_case(P, d)
    Q, Kp, Vp, table, scale, lens, sink = _cuda(pr.edge_inputs(P, d))
    K, V = _cuda(pr.edge_gathered(P, d))
    ref = pr.edge_reference(P, d)
    for n_splits in pr.SPLITS:
        where = f"edges d{d} page {P} splits {n_splits}"
        got = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, causal=True, sink=sink, n_splits=n_splits)
        want = fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=True, sink=sink, n_splits=n_splits)
        _same_bits(got, want, where)
        _check(where, c["lens"], c["nq"], True, *got, ref)


# ---- 3. garbage
@pytest.mark.parametrize("P", [32, 96, 256])
@pytest.mark.parametrize("i", pr.GARBAGE_CASES, ids=[dr.case_id(dr.CASES[i]) for i in pr.GARBAGE_CASES])
def test_garbage_in_the_table_and_in_the_pool_changes_nothing(i, P):
    """Unused table entries -1 / 0x7fffffff against zeros; the pool's unused rows and pages NaN against 3e38 against 0: the same bits."""
    fa, c = _fa(), dr.CASES[i]
    Q, _, _, scale, lens_dev, sink = _case_dev(i)

    def run(n_splits, fill, zero_unused):
        Kp, Vp, table, _, _ = _pages_dev(i, P, fill, zero_unused)
        return fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens_dev, scale, causal=c["causal"], sink=sink, n_splits=n_splits)

    for n_splits in (0, 1, 7):
        want = run(n_splits, "zero", True)
        _same_bits(run(n_splits, "zero", False), want, (n_splits, "table"))
        for fill in ("nan", "3e38"):
            _same_bits(run(n_splits, fill, False), want, (n_splits, fill))


# ---- 4. shared pages
@pytest.mark.parametrize("d", [64, 128])
def test_shared_and_repeated_pages(d):
    """Two sequences whose first two entries are the same pages (a shared prefix), one sequence that uses a page twice."""
    fa = _fa()
    hq, hkv, nq, P, n_pages = 8, 2, 4, 64, 9
    g = torch.Generator().manual_seed(4400 + d)
    Q = (torch.rand(3, hq, nq, d, generator=g) - 0.5).bfloat16().cuda()
    Kp, Vp = ((torch.rand(n_pages, hkv, P, d, generator=g) - 0.5).bfloat16().cuda() for _ in range(2))
    table = torch.tensor([[7, 2, 5, 0], [7, 2, 1, 8], [4, 6, 4, 3]], dtype=torch.int32).cuda()
    lens = [200, 256, 192]
    lens_dev = torch.tensor(lens, dtype=torch.int32).cuda()
    K, V = pr.gather(Kp, table, lens, P), pr.gather(Vp, table, lens, P)
    assert torch.equal(K[0, :, :128], K[1, :, :128]) and torch.equal(K[2, :, :64], K[2, :, 128:192])
    ref = pr.reference64(Q.cpu(), K.cpu(), V.cpu(), lens, 1.0 / d ** 0.5, True, None)
    for n_splits in (0, 1, 2):
        got = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens_dev, causal=True, n_splits=n_splits)
        _same_bits(got, fa.flash_attention_2_decode(Q, K, V, lens_dev, causal=True, n_splits=n_splits), (d, n_splits))
        _check(f"shared pages d{d} splits {n_splits}", lens, nq, True, *got, ref)


# ---- 5. writes
def _carved(n, dtype, pad):
    """A tensor of n elements inside a larger buffer filled with the sentinel: (the buffer as integers, the view)."""
    it, sent = (torch.int16, SENT16) if dtype == torch.bfloat16 else (torch.int32, SENT32) if dtype == torch.float32 else (torch.uint8, 0x5A)
    big = torch.full((n + 2 * pad,), sent, dtype=it, device="cuda")
    return big, big[pad:pad + n].view(dtype)


@pytest.mark.parametrize("n_splits", [1, 7])
@pytest.mark.parametrize("i", pr.GARBAGE_CASES[:2], ids=[dr.case_id(dr.CASES[i]) for i in pr.GARBAGE_CASES[:2]])
def test_every_output_element_is_written_and_nothing_else(i, n_splits):
    fa, c, P = _fa(), dr.CASES[i], 96
    Q, _, _, scale, lens_dev, sink = _case_dev(i)
    Kp0, Vp0, table0, lens, cap = _pages_dev(i, P)
    Kp, Vp, table = Kp0.clone(), Vp0.clone(), table0.clone()
    B, hq, nq, d = Q.shape
    need = fa._capi.lib().fa2_decode_workspace_bytes(B, hq, c["hkv"], nq, cap, d, n_splits)
    assert (need > 0) == (n_splits > 1)
    pad = 256
    bO, O = _carved(Q.numel(), torch.bfloat16, pad)
    bL, L = _carved(B * hq * nq, torch.float32, pad)
    bW, W = _carved(max(need, 256), torch.uint8, pad)
    fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens_dev, scale, causal=c["causal"], sink=sink, n_splits=n_splits,
                                      O=O.view(B, hq, nq, d), L=L.view(B, hq, nq), workspace=W)
    torch.cuda.synchronize()
    assert not (O.view(torch.int16) == SENT16).any() and not (L.view(torch.int32) == SENT32).any()      # sequences without keys included
    for big, n, sent in ((bO, O.numel(), SENT16), (bL, L.numel(), SENT32), (bW, W.numel(), 0x5A)):
        assert (big[:pad] == sent).all() and (big[pad + n:] == sent).all()
    if need:
        assert (bW[pad + need:] == 0x5A).all()
    else:
        assert (W == 0x5A).all()      # one split touches no workspace
    # the pool and the table are only read (compared as integers: the pool is full of NaNs)
    assert torch.equal(Kp.view(torch.int16), Kp0.view(torch.int16)) and torch.equal(Vp.view(torch.int16), Vp0.view(torch.int16))
    assert torch.equal(table, table0)
    _check(f"{dr.case_id(c)} carved, page {P} splits {n_splits}", lens, nq, c["causal"], O.view(B, hq, nq, d), L.view(B, hq, nq),
           pr.paged_reference(i, P))


# ---- 6. one captured graph
def test_one_captured_graph_serves_a_changing_table():
    """One call captured with a caller workspace, O and L; between replays seqlens_k and block_table change IN PLACE -- a sequence
    grows into a new page, two sequences swap their pages -- and each replay is bit for bit an eager call on the new values.  One
    stream, no parallel branches."""
    fa = _fa()
    i, P = pr.GARBAGE_CASES[0], 64
    c = dr.CASES[i]
    Q, _, _, scale, _, sink = _case_dev(i)
    Kp0, Vp0, table0, lens0, cap = _pages_dev(i, P)
    # every page holds data here: a page a sequence grows into, or gets in a swap, must not be NaN below its length
    g = torch.Generator().manual_seed(77)
    fresh = lambda t: torch.where(torch.isnan(t.float()), (torch.rand(t.shape, generator=g) - 0.5).cuda(), t.float()).bfloat16()
    Kp, Vp = fresh(Kp0), fresh(Vp0)
    B, hq, nq, d = Q.shape
    table, lens = table0.clone(), torch.tensor(lens0, dtype=torch.int32, device="cuda")
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device="cuda")
    ws = fa.decode_workspace(B, hq, c["hkv"], nq, cap, d, 0)
    assert ws.numel() > 0
    call = lambda: fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, causal=True, sink=sink, n_splits=0, O=O, L=L,
                                                     workspace=ws)
    call()      # (the first launch of a kernel sets its LDS limit: not inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    spare = sorted(set(range(Kp.shape[0])) - {int(table0[b, p]) for b, n in enumerate(lens0) for p in range(pr.pages_for(n, P))})
    grow = next(b for b, n in enumerate(lens0) if 0 < n < cap - P and n % P)      # a sequence with a partly filled last page
    a, b2 = [b for b, n in enumerate(lens0) if n > P][:2]                          # two sequences with more than a page
    for step in range(2):
        new_table, new_lens = table0.cpu().clone(), list(lens0)
        if step == 0:      # a sequence grows into a new page
            new_lens[grow] = pr.pages_for(lens0[grow], P) * P + 3
            new_table[grow, pr.pages_for(lens0[grow], P)] = spare[0]
        else:              # two sequences swap their pages (and their lengths with them)
            new_table[[a, b2]] = new_table[[b2, a]]
            new_lens[a], new_lens[b2] = new_lens[b2], new_lens[a]
        table.copy_(new_table.cuda())
        lens.copy_(torch.tensor(new_lens, dtype=torch.int32).cuda())
        O.view(torch.int16).fill_(SENT16)
        L.view(torch.int32).fill_(SENT32)
        graph.replay()
        torch.cuda.synchronize()
        want = fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, scale, causal=True, sink=sink, n_splits=0)
        _same_bits((O, L), want, ("replay", step))
        K, V = pr.gather(Kp, table, new_lens, P), pr.gather(Vp, table, new_lens, P)
        _same_bits((O, L), fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=True, sink=sink, n_splits=0), ("contiguous", step))
        assert not torch.isnan(O.float()).any()


# ---- 7. more than 32 rows
def test_more_than_32_rows_is_refused_and_writes_nothing():
    fa = _fa()
    lib = fa._capi.lib()
    B, hq, hkv, nq, P, max_pages, d = 1, 8, 2, 9, 64, 5, 128      # 4 x 9 = 36 rows
    n_pages = 7
    Q = torch.zeros(B, hq, nq, d, dtype=torch.bfloat16, device="cuda")
    Kp = torch.zeros(n_pages, hkv, P, d, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(B, max_pages, dtype=torch.int32, device="cuda")
    O = torch.full((B, hq, nq, d), SENT16, dtype=torch.int16, device="cuda")
    L = torch.full((B, hq, nq), SENT32, dtype=torch.int32, device="cuda")
    ws = torch.full((lib.fa2_decode_workspace_bytes(B, hq, hkv, nq, max_pages * P, d, 2),), 0x5A, dtype=torch.uint8, device="cuda")
    for n_splits in (1, 2):
        st = lib.fa2_forward_decode_paged(Q.data_ptr(), Kp.data_ptr(), Kp.data_ptr(), table.data_ptr(), None, None, O.data_ptr(), L.data_ptr(),
                                          B, hq, hkv, nq, n_pages, P, max_pages, d, ctypes.c_float(0.1), 0, 1, n_splits, ws.data_ptr(),
                                          ws.numel(), None)
        assert st == -6
    torch.cuda.synchronize()
    assert (O == SENT16).all() and (L == SENT32).all() and (ws == 0x5A).all()
    with pytest.raises(ValueError, match="36 rows, decode takes at most 32"):
        fa.flash_attention_2_decode_paged(Q, Kp, Kp, table)
