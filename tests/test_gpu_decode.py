"""GPU: split-KV decode attention over a KV cache with per-sequence lengths (fa2_forward_decode through
cuda_flashattention_amd.flash_attention_2_decode): Q [B, H_q, N_q, d] against caches [B, H_kv, N_cap, d], lengths in device memory.

CASES, inputs, the float64 reference and the gates are tests/decode_ref.py's (tests/test_decode_reference.py certifies on the CPU
that an emulation of the kernels' data flow meets the gates on every case here).  The sizes the kernel has: a wave's MFMA tile is
TILE = 32 keys, the key block KB = 128 keys is one round of the four waves and the grain of a split's first key; the lengths of
one batch are {0, 1, 2, KB - 1, KB, KB + 1, 300, 1100, 2500} -- or the tile's edges {TILE - 1, TILE, TILE + 1, ...} -- in caches of
2560 rows and of exactly the longest length; N_q 1 and 4 with and without the mask (sequences shorter than N_q have rows without
a key); 3 heads on 3, 8 on 2, 8 on 1 (N_q = 4: M = 32 rows) and 32 on 1; both head dims; 0 (the default), 1, 2, 7 and 64 splits (at
64 most splits of most sequences are empty); sinks on a subset, two heads of them -inf; seqlens_k = None; and the peaked, spikes,
scale-one and low-level regimes of tests/regimes.py at 300 and 1100 keys (a late large key inside a later split, L < -88).

GATES: O rel-L2 <= 5e-3 over the whole tensor; max |dL| <= 1e-4 over rows with finite |L_ref| <= 25, <= 1e-3 above; the rows with
L = -inf are exactly the reference's, O is exactly 0 on them and on every row without a visible key; no NaN, no Inf; and PER ROW |O_i - O_ref,i| <= KAPPA u sqrt(sum_j P_ij^2 |v_j|^2) + u |O_i| (tests/decode_rows_ref.py: the tensor gate
alone lets a fault on the long sequences' P V side pass), the worst ratio printed with its (sequence, head, token)."""
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


@functools.lru_cache(maxsize=None)
def _dev(i):
    return tuple(None if t is None else (t.cuda() if isinstance(t, torch.Tensor) else t) for t in dr.inputs(i))


def _keyless(c):
    """[B, 1, nq] bool: the rows that see no key."""
    return np.array([[[n == 0 or (c["causal"] and q + n - c["nq"] < 0) for q in range(c["nq"])]] for n in c["lens"]])


def _check(where, c, O, L, ref, extra=None):
    O, L = O.float().cpu().numpy(), L.cpu().numpy()
    e = dr.errors(O, L, ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    keyless = np.broadcast_to(_keyless(c), L.shape)
    assert (O[keyless] == 0).all(), (where, "O of a row without a key")
    rows.check(where, O, ref, extra=extra)


@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=[dr.case_id(c) for c in dr.CASES])
def test_decode_against_reference(i):
    fa, c = _fa(), dr.CASES[i]
    Q, K, V, scale, lens, sink = _dev(i)
    ref = dr.reference(i)
    for n_splits in c["splits"]:
        O, L = fa.flash_attention_2_decode(Q, K, V, lens if c["seqlens"] else None, scale, causal=c["causal"], sink=sink,
                                           n_splits=n_splits)
        _check(f"{dr.case_id(c)} splits {n_splits}", c, O, L, ref)


def _first(**want):
    return next(i for i, c in enumerate(dr.CASES) if all(c[k] == v for k, v in want.items()))


GARBAGE_CASES = [_first(hq=8, hkv=2, d=128, nq=4, causal=True, regime=None, seqlens=True),
                 _first(hq=8, hkv=1, d=64, nq=4, causal=False, regime=None, seqlens=True),
                 _first(hq=3, hkv=3, d=128, nq=1, causal=True, regime=None, seqlens=True)]


@pytest.mark.parametrize("i", GARBAGE_CASES, ids=[dr.case_id(dr.CASES[i]) for i in GARBAGE_CASES])
def test_garbage_past_the_length_changes_nothing(i):
    """Cache rows >= len_b filled with NaN, and with 3e38: O and L are bit for bit those of the run with zeros there."""
    fa, c = _fa(), dr.CASES[i]
    Q, K, V, scale, lens, sink = _dev(i)

    def run(fill, n_splits):
        k, v = K.clone(), V.clone()
        for b, n in enumerate(c["lens"]):
            k[b, :, n:] = fill
            v[b, :, n:] = fill
        return fa.flash_attention_2_decode(Q, k, v, lens, scale, causal=c["causal"], sink=sink, n_splits=n_splits)

    for n_splits in (0, 1, 7):
        want = run(0.0, n_splits)
        for fill in (float("nan"), 3e38):
            got = run(fill, n_splits)
            assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (fill, n_splits, "O")
            assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (fill, n_splits, "L")


def _carved(n, dtype, pad):
    """A tensor of n elements inside a larger buffer filled with the sentinel: (the buffer as integers, the view)."""
    it, sent = (torch.int16, SENT16) if dtype == torch.bfloat16 else (torch.int32, SENT32) if dtype == torch.float32 else (torch.uint8, 0x5A)
    big = torch.full((n + 2 * pad,), sent, dtype=it, device="cuda")
    return big, big[pad:pad + n].view(dtype)


@pytest.mark.parametrize("n_splits", [1, 7])
@pytest.mark.parametrize("i", GARBAGE_CASES[:2], ids=[dr.case_id(dr.CASES[i]) for i in GARBAGE_CASES[:2]])
def test_every_output_element_is_written_and_nothing_else(i, n_splits):
    fa, c = _fa(), dr.CASES[i]
    Q, K, V, scale, lens, sink = _dev(i)
    B, hq, nq, d = Q.shape
    need = fa._capi.lib().fa2_decode_workspace_bytes(B, hq, c["hkv"], nq, c["ncap"], d, n_splits)
    assert (need > 0) == (n_splits > 1)
    pad = 256
    bO, O = _carved(Q.numel(), torch.bfloat16, pad)
    bL, L = _carved(B * hq * nq, torch.float32, pad)
    bW, W = _carved(max(need, 256), torch.uint8, pad)
    fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=c["causal"], sink=sink, n_splits=n_splits, O=O.view(B, hq, nq, d),
                                L=L.view(B, hq, nq), workspace=W)
    torch.cuda.synchronize()
    assert not (O.view(torch.int16) == SENT16).any() and not (L.view(torch.int32) == SENT32).any()      # sequences without keys included
    for big, n, sent in ((bO, O.numel(), SENT16), (bL, L.numel(), SENT32), (bW, W.numel(), 0x5A)):
        assert (big[:pad] == sent).all() and (big[pad + n:] == sent).all()
    if need:
        assert (bW[pad + need:] == 0x5A).all()
    else:
        assert (W == 0x5A).all()      # one split touches no workspace
    _check(f"{dr.case_id(c)} carved, splits {n_splits}", c, O.view(B, hq, nq, d), L.view(B, hq, nq), dr.reference(i))


def test_two_runs_agree_bit_for_bit():
    fa = _fa()
    for i in GARBAGE_CASES:
        c = dr.CASES[i]
        Q, K, V, scale, lens, sink = _dev(i)
        for n_splits in (0, 1, 64):
            a = fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=c["causal"], sink=sink, n_splits=n_splits)
            b = fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=c["causal"], sink=sink, n_splits=n_splits)
            assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_one_captured_graph_serves_changing_lengths():
    """One call captured with a caller workspace and a seqlens_k tensor; seqlens_k and Q change in place; the replay is bit for
    bit an eager call on the new values.  One stream, no parallel branches."""
    fa = _fa()
    i = GARBAGE_CASES[0]
    c = dr.CASES[i]
    Q0, K, V, scale, lens0, sink = _dev(i)
    B, hq, nq, d = Q0.shape
    Q, lens = Q0.clone(), lens0.clone()
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device="cuda")
    ws = fa.decode_workspace(B, hq, c["hkv"], nq, c["ncap"], d, 0)
    assert ws.numel() > 0
    call = lambda: fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=True, sink=sink, n_splits=0, O=O, L=L, workspace=ws)
    call()      # (the first launch of a kernel sets its LDS limit: not inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.Generator().manual_seed(5)
    for step in range(2):
        new_lens = torch.tensor([min(n + 1 + 40 * step, c["ncap"]) for n in c["lens"]][::-1], dtype=torch.int32)
        lens.copy_(new_lens.cuda())
        Q.copy_(((torch.rand(Q.shape, generator=g) - 0.5)).bfloat16().cuda())
        O.view(torch.int16).fill_(SENT16)
        L.view(torch.int32).fill_(SENT32)
        graph.replay()
        torch.cuda.synchronize()
        want = fa.flash_attention_2_decode(Q, K, V, lens, scale, causal=True, sink=sink, n_splits=0)
        assert torch.equal(O.view(torch.int16), want[0].view(torch.int16)) and torch.equal(L.view(torch.int32), want[1].view(torch.int32))


@pytest.mark.parametrize("d", [64, 128])
def test_a_cache_in_two_allocations_is_two_calls_and_a_merge(d):
    """Keys [0, cut) in one allocation and [cut, ...) in another: the first call without the mask and the sink, the last with
    both, merge_states_forward over the pair -- against the reference over the whole cache, the same gates."""
    fa = _fa()
    hq, hkv, nq, cut, ncap = 8, 2, 4, 777, 2560
    lens = (1100, 900, 2500, cut + nq)
    c = dict(hq=hq, hkv=hkv, d=d, nq=nq, causal=True, lens=lens, ncap=ncap)
    g = torch.Generator().manual_seed(8800 + d)
    mk = lambda h, n: (torch.rand(len(lens), h, n, d, generator=g) - 0.5).bfloat16()
    Q, K, V = mk(hq, nq), mk(hkv, ncap), mk(hkv, ncap)
    sink = dr.sink_of(hq, 3)
    scale = 1.0 / d ** 0.5
    from sink_ref import ref_attention_sink
    rO, rL = np.zeros(tuple(Q.shape)), np.zeros(tuple(Q.shape[:3]))
    for b, n in enumerate(lens):
        k, v = (np.repeat(t[b, :, :n].double().numpy(), hq // hkv, axis=0) for t in (K, V))
        rO[b], rL[b] = ref_attention_sink(Q[b].double().numpy(), k, v, np.zeros((hq, nq, d)), scale, True, sink.double().numpy())[:2]
    ref = rows.Ref(rO, rL, rows.quad64(Q, K, V, lens, scale, True, sink))
    # the two partial O's are rounded to bf16 before the merge weighs them: u (w_a |O_a,i| + w_b |O_b,i|) on top of the row gate,
    # from the reference partials (the first without the mask and the sink, the last with both) and their weights exp(L_part - L)
    parts = [pr.reference64(Q, K[:, :, :cut], V[:, :, :cut], [min(n, cut) for n in lens], scale, False, None),
             pr.reference64(Q, K[:, :, cut:], V[:, :, cut:], [n - cut for n in lens], scale, True, sink)]
    extra = rows.merged_extra(parts, rL)
    Qd, sd = Q.cuda(), sink.cuda()
    first = (K[:, :, :cut].contiguous().cuda(), V[:, :, :cut].contiguous().cuda())
    last = (K[:, :, cut:].contiguous().cuda(), V[:, :, cut:].contiguous().cuda())
    la = torch.tensor([min(n, cut) for n in lens], dtype=torch.int32).cuda()
    lb = torch.tensor([n - cut for n in lens], dtype=torch.int32).cuda()
    for n_splits in (0, 1, 7):
        a = fa.flash_attention_2_decode(Qd, *first, la, scale, causal=False, n_splits=n_splits)
        b = fa.flash_attention_2_decode(Qd, *last, lb, scale, causal=True, sink=sd, n_splits=n_splits)
        O, L = fa.merge_states_forward([a[0], b[0]], [a[1], b[1]])
        _check(f"two allocations d{d} splits {n_splits}", c, O, L, ref, extra=extra)


def test_more_than_32_rows_is_refused_and_writes_nothing():
    fa = _fa()
    lib = fa._capi.lib()
    B, hq, hkv, nq, ncap, d = 1, 8, 2, 9, 300, 128      # 4 x 9 = 36 rows
    Q = torch.zeros(B, hq, nq, d, dtype=torch.bfloat16, device="cuda")
    K = torch.zeros(B, hkv, ncap, d, dtype=torch.bfloat16, device="cuda")
    O = torch.full((B, hq, nq, d), SENT16, dtype=torch.int16, device="cuda")
    L = torch.full((B, hq, nq), SENT32, dtype=torch.int32, device="cuda")
    ws = torch.full((lib.fa2_decode_workspace_bytes(B, hq, hkv, nq, ncap, d, 2),), 0x5A, dtype=torch.uint8, device="cuda")
    for n_splits in (1, 2):
        st = lib.fa2_forward_decode(Q.data_ptr(), K.data_ptr(), K.data_ptr(), None, None, O.data_ptr(), L.data_ptr(), B, hq, hkv, nq, ncap, d,
                                    ctypes.c_float(0.1), 0, 1, n_splits, ws.data_ptr(), ws.numel(), None)
        assert st == -6
    torch.cuda.synchronize()
    assert (O == SENT16).all() and (L == SENT32).all() and (ws == 0x5A).all()
