"""GPU: the MLA latent-cache append (fa2_mla_kv_append / _paged through mla_kv_cache_append / _paged) against a model written
here from the contract's words, BIT FOR BIT -- the contract is an exact fp32 expression with one rounding, so there is no
tolerance: row[:512] = qk_norm_ref.rms_rows (its butterfly runs to 64 lanes at d = 512), row[512:] and Q_out[..., 512:] =
rope_ref.rotate_bf16 at table row pos, Q_out[..., :512] the bytes of q_nope, and the write-or-drop rule spelled out below.
One batch of capacity 96 carries the lengths AFTER the append (n_new, 35, 64, 96, 97, n_new - 1, 99 + n_new): a first row, a
page edge, the last row, one token past the capacity, one token before row 0, every token dropped.  The sources are strided
slices of fused projection outputs; the cache is pre-filled with a sentinel and Q_out with NaN."""
import pytest
import torch

import qk_norm_ref as nr
import rope_ref as rr

pytestmark = pytest.mark.gpu

CAP, P, SENTINEL, SCALE = 96, 32, -1234.0, 0.1


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _lens(n_new):
    return (n_new, 35, 64, 96, 97, n_new - 1, 99 + n_new)


def _sources(B, H, n_new, seed):
    """The fused host tensors the views are cut from: kv [B, n_new, 1536 + 576], q [B, n_new, H, 192], nope [H, B n_new, 512], in
    (-3, 3), the token (1, 0) all zero."""
    g = torch.Generator().manual_seed(seed)
    kv, q, nope = (((torch.rand(s, generator=g) - 0.5) * 6).bfloat16() for s in ((B, n_new, 2112), (B, n_new, max(H, 1), 192), (max(H, 1), B * n_new, 512)))
    kv[1, 0], q[1, 0], nope[:, n_new] = 0, 0, 0
    return kv, q, nope


def _views(kv, q, nope, H):
    """(q_nope [B, H, n_new, 512], q_pe [B, H, n_new, 64], kv_new [B, n_new, 576]) as views; H = 0: no queries."""
    B, n_new = kv.shape[:2]
    if not H:
        return None, None, kv[..., 1536:]
    return nope.view(H, B, n_new, 512).permute(1, 0, 2, 3), q[..., 128:].permute(0, 2, 1, 3), kv[..., 1536:]


def _table(B, bad):
    """[B, CAP / P] distinct pages of a pool of B CAP / P + 3; bad: one entry -1 and one >= n_pages on pages tokens fall in."""
    mp = CAP // P
    table = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(5))[:B * mp].to(torch.int32).view(B, mp)
    if bad:
        table[1, 1], table[3, 2] = -1, B * mp + 8      # rows 32 .. 34 of sequence 1, rows 93 .. 95 of sequence 3
    return table


def _model(cache, table, views, lens, w, cos, sin, il):
    """The contract on host tensors, IN PLACE on the cache [B, CAP, 576] (table None) or the pool; returns Q_out or None."""
    q_nope, q_pe, kv = views
    B, n_new = kv.shape[:2]
    latent = nr.rms_rows(kv[..., :512], w, nr.EPS)
    Q_out = None if q_nope is None else torch.zeros(B, q_nope.shape[1], n_new, 576, dtype=torch.bfloat16)
    for b in range(B):
        for t in range(n_new):
            pos = lens[b] - n_new + t
            if not 0 <= pos < CAP:
                continue                                  # dropped: no cache row, Q_out stays +0.0
            if Q_out is not None:
                Q_out[b, :, t] = torch.cat((q_nope[b, :, t], rr.rotate_bf16(q_pe[b, :, t], cos[pos], sin[pos], il)), dim=-1)
            row = torch.cat((latent[b, t], rr.rotate_bf16(kv[b, t, 512:], cos[pos], sin[pos], il)))
            if table is None:
                cache[b, pos] = row
            elif 0 <= int(table[b, pos // P]) < cache.shape[0]:      # a bad entry drops the cache row only
                cache[int(table[b, pos // P]), pos % P] = row
    return Q_out


def _same(got, want, where):
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), where


@pytest.mark.parametrize("H,n_new", ((0, 3), (5, 1), (16, 3)))
@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_cache_and_q_out_equal_the_model_bit_for_bit(paged, interleaved, H, n_new):
    fa = _fa()
    lens = _lens(n_new)
    B = len(lens)
    host = _sources(B, H, n_new, 100 * H + n_new)
    w, (cos, sin) = nr.weights(512, nr.WEIGHT_SEED)[1], rr.random_tables(CAP, 64, 9)
    table = _table(B, bad=True) if paged else None
    cache = torch.full((B * (CAP // P) + 3, P, 576) if paged else (B, CAP, 576), SENTINEL, dtype=torch.bfloat16)
    dev_cache, dev_lens = cache.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    want = _model(cache, table, _views(*host, H), lens, w, cos, sin, interleaved)
    q_nope, q_pe, kv = _views(*(x.cuda() for x in host), H)
    Q_out = torch.full((B, H, n_new, 576), float("nan"), dtype=torch.bfloat16, device="cuda") if H else None
    if paged:
        got = fa.mla_kv_cache_append_paged(q_nope, q_pe, kv, dev_cache, table.cuda(), cos.cuda(), sin.cuda(), w.cuda(), nr.EPS, dev_lens,
                                           interleaved=interleaved, Q_out=Q_out)
    else:
        got = fa.mla_kv_cache_append(q_nope, q_pe, kv, dev_cache, cos.cuda(), sin.cuda(), w.cuda(), nr.EPS, dev_lens,
                                     interleaved=interleaved, Q_out=Q_out)
    _same(dev_cache, cache, "cache")      # unwritten rows keep the sentinel
    assert (got is None and want is None) if not H else got is Q_out
    if H:
        _same(Q_out, want, "Q_out")       # every row written: no NaN is left
        assert (want[4, :, n_new - 1] == 0).all() and (want[0] != 0).any()


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_one_captured_graph_of_append_and_decode_serves_every_step(paged):
    fa = _fa()
    H, n_new, B = 16, 2, 3
    w, (cos, sin) = nr.weights(512, nr.WEIGHT_SEED)[1], rr.random_tables(CAP, 64, 9)
    table = _table(B, bad=False) if paged else None
    cache = ((torch.rand((B * (CAP // P) + 3, P, 576) if paged else (B, CAP, 576), generator=torch.Generator().manual_seed(3)) - 0.5)).bfloat16()
    dev = [x.cuda() for x in _sources(B, H, n_new, 0)]
    dev_cache, lens, dtable = cache.cuda(), torch.zeros(B, dtype=torch.int32, device="cuda"), None if table is None else table.cuda()
    tabs = (cos.cuda(), sin.cuda(), w.cuda(), nr.EPS)
    Q_out = torch.empty(B, H, n_new, 576, dtype=torch.bfloat16, device="cuda")
    O, L = torch.empty(B, H, n_new, 512, dtype=torch.bfloat16, device="cuda"), torch.empty(B, H, n_new, dtype=torch.float32, device="cuda")

    def decode(Q, C, O, L):
        if paged:
            return fa.flash_attention_2_mla_decode_paged(Q, C, dtable, lens, softmax_scale=SCALE, n_splits=1, O=O, L=L)
        return fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, n_splits=1, O=O, L=L)

    def step(C, Q_out, O, L):
        q_nope, q_pe, kv = _views(*dev, H)
        if paged:
            fa.mla_kv_cache_append_paged(q_nope, q_pe, kv, C, dtable, *tabs, lens, Q_out=Q_out)
        else:
            fa.mla_kv_cache_append(q_nope, q_pe, kv, C, *tabs, lens, Q_out=Q_out)
        decode(Q_out, C, O, L)

    step(dev_cache.clone(), torch.empty_like(Q_out), torch.empty_like(O), torch.empty_like(L))      # the code objects load outside the capture
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(dev_cache, Q_out, O, L)
    torch.cuda.current_stream().wait_stream(side)
    dev_cache.copy_(cache)                # whatever the capture ran or did not run, the steps start from the model's cache
    for s, now in enumerate(((2, 35, 64), (4, 37, 97))):
        host = _sources(B, H, n_new, 40 + s)
        for d, h in zip(dev, host):
            d.copy_(h)                    # in place: the graph's views see the new step
        lens.copy_(torch.tensor(now, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want_q = _model(cache, table, _views(*host, H), now, w, cos, sin, False)
        want = decode(want_q.cuda(), cache.cuda(), torch.empty_like(O), torch.empty_like(L))
        assert torch.equal(O.view(torch.int16), want[0].view(torch.int16)) and torch.equal(L.view(torch.int32), want[1].view(torch.int32)), s
