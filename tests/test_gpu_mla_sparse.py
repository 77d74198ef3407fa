"""GPU: the sparse MLA decode (fa2_forward_mla_decode_sparse / _paged, include/fa2_mla_sparse_mi355x.h) against tests/mla_ref's
float64 reference on the live rows compacted, in list order with duplicates kept, into a dense cache per (sequence, token).  Gates
are the MLA family's, unchanged: decode_rows_ref.check per row of O, decode_ref's L_ABS / L_ABS_LARGE on L, the -inf rows exactly
the reference's with O exactly 0; the rest are bit equalities.  Index rows are seeded and unsorted: positions in [0, cap), some
past the length, -1 in the middle and at the end, INT_MIN, INT_MAX, a duplicated live position."""
import functools

import numpy as np
import pytest
import torch

import decode_ref as dr
import decode_rows_ref as rows
import mla_ref

pytestmark = pytest.mark.gpu

N_CAP, SCALE = 384, 0.0913
LENS = (0, 1, 31, 33, 128, 300, N_CAP)
B = len(LENS)
SHAPES = ((16, 1, 32), (40, 1, 96), (5, 3, 33), (16, 2, 100))      # (H, q_len, topk)
SPLITS = (0, 1, 2, 5)
I32 = (-2 ** 31, 2 ** 31 - 1)


def _fa():
    import cuda_flashattention_amd as fa
    return fa


@functools.lru_cache(maxsize=None)
def _inputs(H, nq, topk):
    """Host Q, cache (tests/test_gpu_mla_decode.py's distributions; the last two sequences share their first 96 rows) and indices
    [B, nq, topk].  Token nq - 1 of sequence 2 names nothing live, of sequence 5 live positions in its first 32 slots only, and
    slot 1 of every row repeats slot 0."""
    g = torch.Generator().manual_seed(576 + 7 * H + nq)
    Q = ((torch.rand(B, H, nq, 576, generator=g) - 0.5) * 12).bfloat16()
    C = (torch.rand(B, N_CAP, 576, generator=g) - 0.5).bfloat16()
    C[B - 1, :96] = C[B - 2, :96]
    idx = torch.randint(0, N_CAP, (B, nq, topk), generator=g, dtype=torch.int32)
    for b, n in enumerate(LENS):      # mostly live positions where there are any, then the dead kinds
        idx[b] = torch.where(torch.rand(nq, topk, generator=g) < 0.6, idx[b] % max(n, 1), idx[b])
    idx[:, :, 3::7], idx[:, :, -2:], idx[:, :, 5], idx[:, :, 9] = -1, -1, I32[0], I32[1]
    idx[:, :, 1] = idx[:, :, 0]
    idx[2, nq - 1] = torch.where((idx[2, nq - 1] >= 0) & (idx[2, nq - 1] < LENS[2]), idx[2, nq - 1] + LENS[2], idx[2, nq - 1])
    idx[5, nq - 1, 32:] = -1
    return Q, C, idx


def _live(idx, nq, causal):
    n, i = torch.tensor(LENS)[:, None, None], torch.arange(nq)[None, :, None]
    return (idx >= 0) & (idx < n) & ((idx <= i + n - nq) | (not causal))


@functools.lru_cache(maxsize=None)
def _reference(H, nq, topk, causal):
    Q, C, idx = _inputs(H, nq, topk)
    live = _live(idx, nq, causal)
    dense, counts = torch.zeros(B * nq, topk, 576, dtype=torch.bfloat16), live.sum(-1).reshape(-1)
    for k in range(B * nq):
        dense[k, :counts[k]] = C[k // nq, idx[k // nq, k % nq][live[k // nq, k % nq]].long()]
    chunk = -(-(-(-topk // 2)) // 32) * 32
    assert counts[2 * nq + nq - 1] == 0 and LENS[2] > 0, "a row without a live entry in a sequence with keys"
    assert counts[5 * nq + nq - 1] > 0 and not live[5, nq - 1, chunk:].any(), "a row whose live entries sit in split 0 of 2"
    assert live[B - 1, nq - 1, 0] and idx[B - 1, nq - 1, 0] == idx[B - 1, nq - 1, 1], "a duplicated live position"
    return mla_ref.reference64(Q.permute(0, 2, 1, 3).reshape(B * nq, H, 1, 576), dense, counts.tolist(), SCALE, False)


def _dev(H, nq, topk):
    return tuple(t.cuda() for t in _inputs(H, nq, topk)) + (torch.tensor(LENS, dtype=torch.int32, device="cuda"),)


def _pool(C, P, fill=0.0, unused=None, live=None, idx=None):
    """mla_ref.paged's pool and table with the last two sequences sharing their first page; `unused`: what the table entries that
    no live index goes through are overwritten with."""
    pool, table = mla_ref.paged(C, LENS, P, 31 + P, fill)
    table[B - 1, 0] = table[B - 2, 0]
    if unused is not None:
        used = torch.zeros_like(table, dtype=torch.bool)
        for b in range(B):
            used[b, (idx[b][live[b]].long() // P).unique()] = True
        table[~used] = torch.tensor(unused, dtype=torch.int32).repeat(table.numel())[:int((~used).sum())]
    return pool.cuda(), table.cuda()


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
@pytest.mark.parametrize("H,nq,topk", SHAPES)
def test_parity_with_float64_and_paged_equals_contiguous(H, nq, topk, causal):
    fa = _fa()
    Q, C, idx, lens = _dev(H, nq, topk)
    ref = _reference(H, nq, topk, causal)
    pools = {P: _pool(_inputs(H, nq, topk)[1], P) for P in (32, 96)}
    for ns in SPLITS:
        got = fa.flash_attention_2_mla_decode_sparse(Q, C, idx, lens, softmax_scale=SCALE, causal=causal, n_splits=ns)
        O = got[0].float().cpu().permute(0, 2, 1, 3).reshape(B * nq, H, 1, 512).numpy()
        e = dr.errors(O, got[1].cpu().permute(0, 2, 1).reshape(B * nq, H, 1).numpy(), ref)
        print(f"H {H} nq {nq} topk {topk} causal {causal} splits {ns}: dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
        assert e[1] <= dr.L_ABS and e[2] <= dr.L_ABS_LARGE and e[3], (ns, e)
        rows.check((H, nq, topk, causal, ns), O, ref)
        for P, (pool, table) in pools.items():
            paged = fa.flash_attention_2_mla_decode_sparse_paged(Q, pool, table, idx, lens, softmax_scale=SCALE, causal=causal, n_splits=ns)
            _same_bits(paged, got, (H, nq, topk, causal, ns, P))


@pytest.mark.parametrize("H", (16, 40))
def test_identity_indices_reproduce_the_dense_kernel(H):
    fa = _fa()
    Q, C, _, lens = _dev(H, 1, 32)
    idx = torch.arange(N_CAP, dtype=torch.int32, device="cuda").repeat(B, 1, 1)
    _same_bits(fa.flash_attention_2_mla_decode_sparse(Q, C, idx, lens, softmax_scale=SCALE, n_splits=1),
               fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, n_splits=1), H)


def test_garbage_changes_no_bit():
    fa = _fa()
    H, nq, topk = SHAPES[3]
    Q, _, idx, lens = _dev(H, nq, topk)
    host, hidx = _inputs(H, nq, topk)[1:]
    live = _live(hidx, nq, True)
    named = torch.zeros(B, N_CAP, dtype=torch.bool)
    for b in range(B):
        named[b, hidx[b][live[b]].long()] = True
    named[B - 2, :96] |= named[B - 1, :96]      # the page the last two sequences share
    named[B - 1, :96] = named[B - 2, :96]
    for ns in (1, 5):
        want = fa.flash_attention_2_mla_decode_sparse(Q, torch.where(named[..., None], host, 0.0).cuda(), idx, lens, softmax_scale=SCALE, n_splits=ns)
        ws = fa.mla_sparse_workspace(B, H, nq, topk, ns).fill_(255) if ns > 1 else None      # a dirty workspace: NaNs
        for f in (float("nan"), 3e38):
            C = torch.where(named[..., None], host, torch.tensor(f, dtype=torch.bfloat16))
            _same_bits(fa.flash_attention_2_mla_decode_sparse(Q, C.cuda(), idx, lens, softmax_scale=SCALE, n_splits=ns, workspace=ws), want, (ns, f))
            for P in (32, 96):
                pool, table = _pool(C, P, f, (-1, I32[1], I32[0], B * (N_CAP // P) + 3), live, hidx)
                _same_bits(fa.flash_attention_2_mla_decode_sparse_paged(Q, pool, table, idx, lens, softmax_scale=SCALE, n_splits=ns), want, (ns, f, P))


def test_one_captured_graph_serves_changing_indices_and_lengths():
    fa = _fa()
    H, nq, topk = SHAPES[3]
    Q, C, idx, lens = _dev(H, nq, topk)
    O, L = torch.empty(B, H, nq, 512, dtype=torch.bfloat16, device="cuda"), torch.empty(B, H, nq, dtype=torch.float32, device="cuda")
    ws = fa.mla_sparse_workspace(B, H, nq, topk, 2)
    run = lambda O, L, ws: fa.flash_attention_2_mla_decode_sparse(Q, C, idx, lens, softmax_scale=SCALE, n_splits=2, O=O, L=L, workspace=ws)
    run(torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))      # the code objects load outside the capture
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    for step in range(3):
        lens.copy_(torch.tensor([min(n + 17 * step + 1, N_CAP) for n in LENS], dtype=torch.int32))      # in place
        idx.copy_(idx.flip(-1) + step)
        O.zero_(), L.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same_bits((O, L), run(torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws)), ("replay", step))
