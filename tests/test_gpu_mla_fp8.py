"""GPU: the MLA decode and append over e4m3 latent caches (include/fa2_mla_fp8_mi355x.h), which a torch.uint8 cache of 640-byte
rows routes.  The uniform MLA case, latent columns quantised at 1.25 x 2^-10 (nothing saturates, the dequantised values are exact
in fp32): the decode against float64 ON THE DEQUANTISED CACHE -- quantisation error is in no gate -- under the family's gates
unchanged (the path adds one fp32 multiply-add per score and one multiply per output element: 2^-24 against gates at 2^-9); the
append against the bf16 append on the same inputs, bit for bit."""
import functools

import pytest
import torch

import decode_ref as dr
import decode_rows_ref as rows
import kv_append_ref as ka
import mla_ref as mr

pytestmark = pytest.mark.gpu

CAP, SCALE, DESCALE = 384, 0.0913, 1.25 * 2.0 ** -10
LENS = (0, 1, 31, 32, 33, 127, 128, 129, 300, CAP)
B = len(LENS)
A_CAP, A_P, A_H, SENTINEL, BYTE = 96, 32, 5, -1234.0, 0xA5      # the append's capacity, page, heads and what unwritten rows hold


def _fa():
    import cuda_flashattention_amd as fa
    return fa


@functools.lru_cache(maxsize=None)
def _inputs(H, nq):
    """Q [B, H, nq, 576] bf16, the cache [B, 384, 640] uint8 and its dequantised fp32 rows; the last two sequences start alike."""
    g = torch.Generator().manual_seed(640 + 7 * H + nq)
    Q = ((torch.rand(B, H, nq, 576, generator=g) - 0.5) * 12).bfloat16()
    C = (torch.rand(B, CAP, 576, generator=g) - 0.5).bfloat16()
    C[B - 1, :96] = C[B - 2, :96]
    codes = ka.quantise(C[:, None, :, :512], torch.tensor([DESCALE]))[:, 0]
    packed = torch.cat((codes.view(torch.uint8), C[..., 512:].contiguous().view(torch.uint8)), dim=-1)
    return Q, packed, torch.cat((codes.float() * DESCALE, C[..., 512:].float()), dim=-1)


@functools.lru_cache(maxsize=None)
def _reference(H, nq, causal):
    """The MLA decode's float64 reference (a decode_rows_ref.Ref with quad64), on the DEQUANTISED rows."""
    Q, _, deq = _inputs(H, nq)
    return mr.reference64(Q, deq, LENS, SCALE, causal)


def _paged(cache, P, fill):
    """(pool, table) on the device: shuffled pages of P rows, `fill` bytes past the lengths and in the spare pages; the last two
    sequences share their first page; fill != 0: the table slots no length reaches hold entries outside the pool."""
    mp = CAP // P
    table = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(P))[:B * mp].to(torch.int32).view(B, mp)
    table[B - 1, 0] = table[B - 2, 0]
    pool = torch.full((B * mp + 3, P, 640), fill, dtype=torch.uint8)
    for b, n in enumerate(LENS):
        for p in range(-(-n // P)):
            pool[table[b, p], :min(P, n - p * P)] = cache[b, p * P:min((p + 1) * P, n)]
        if fill:
            table[b, -(-n // P):] = (-7, 1 << 20, 2 ** 31 - 1)[b % 3]
    return pool.cuda(), table.cuda()


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), where


def _decode_args(n_splits, causal):
    kw = dict(softmax_scale=SCALE, causal=causal, n_splits=n_splits, latent_descale=torch.tensor([DESCALE], device="cuda"))
    return torch.tensor(LENS, dtype=torch.int32, device="cuda"), kw


@pytest.mark.parametrize("n_splits", (0, 1, 2, 5))
@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
@pytest.mark.parametrize("H,nq", ((16, 2), (5, 3), (40, 1)))      # a full block with a causal edge; padding rows and rho % q_len; two row blocks
def test_decode_on_the_dequantised_cache_within_the_row_gates(H, nq, causal, n_splits):
    fa, (Q, cache, _), (lens, kw) = _fa(), _inputs(H, nq), _decode_args(n_splits, causal)
    ref, where = _reference(H, nq, causal), f"mla e4m3 H {H} nq {nq} causal {causal} splits {n_splits}"
    got = fa.flash_attention_2_mla_decode(Q.cuda(), cache.cuda(), lens, **kw)
    e = dr.errors(got[0].float().cpu().numpy(), got[1].cpu().numpy(), ref)
    print(where, f"dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert e[1] <= dr.L_ABS and e[2] <= dr.L_ABS_LARGE and e[3], (where, e)      # e[3]: the -inf rows are the reference's, O = 0 on them
    rows.check(where, got[0], ref)
    for P in (32, 96):
        _same_bits(fa.flash_attention_2_mla_decode_paged(Q.cuda(), *_paged(cache, P, 0), lens, **kw), got, (where, "pages of", P))


@pytest.mark.parametrize("n_splits", (1, 5))
def test_garbage_past_the_lengths_changes_no_bit(n_splits):
    """0xFF is the e4m3 NaN code and 0xFFFF a bf16 NaN; the paged call also gets out-of-range entries in its unused table slots."""
    fa, (Q, cache, _), (lens, kw) = _fa(), _inputs(5, 3), _decode_args(n_splits, True)
    clean, dirty = cache.clone(), cache.clone()
    for b, n in enumerate(LENS):
        clean[b, n:], dirty[b, n:] = 0, 0xFF
    want = fa.flash_attention_2_mla_decode(Q.cuda(), clean.cuda(), lens, **kw)
    assert torch.isfinite(want[0].float()).all() and (want[0] != 0).any()
    _same_bits(fa.flash_attention_2_mla_decode(Q.cuda(), dirty.cuda(), lens, **kw), want, "contiguous")
    _same_bits(fa.flash_attention_2_mla_decode_paged(Q.cuda(), *_paged(cache, 32, 0xFF), lens, **kw), want, "paged")


def _append_inputs(n_new, seed, lens):
    """Device arguments of the appends around the cache: strided q_nope, q_pe, kv_new views; tables, weight, eps and the lengths."""
    g, n = torch.Generator().manual_seed(seed), len(lens)
    kv, q, nope = (((torch.rand(s, generator=g) - 0.5) * 6).bfloat16().cuda() for s in ((n, n_new, 2112), (n, n_new, A_H, 192), (A_H, n * n_new, 512)))
    cos, sin, w = (torch.rand(s, generator=g).cuda() for s in ((A_CAP, 32), (A_CAP, 32), (512,)))
    return (nope.view(A_H, n, n_new, 512).permute(1, 0, 2, 3), q[..., 128:].permute(0, 2, 1, 3), kv[..., 1536:]), (cos, sin, w + 0.5, 1e-6, lens)


def _append(views, cache, table, tabs, **kw):
    fa = _fa()
    return fa.mla_kv_cache_append(*views, cache, *tabs, **kw) if table is None else fa.mla_kv_cache_append_paged(*views, cache, table, *tabs, **kw)


@pytest.mark.parametrize("n_new", (1, 3))
@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_append_stores_the_quantised_bf16_append(paged, interleaved, n_new):
    lens = (n_new, 35, 64, 96, 97, n_new - 1, 99 + n_new)      # a first row, a page edge, the last row, tokens dropped on both sides, all dropped
    views, tabs = _append_inputs(n_new, 31 * n_new + paged, torch.tensor(lens, dtype=torch.int32, device="cuda"))
    n, mp, table = len(lens), A_CAP // A_P, None
    if paged:
        table = torch.randperm(n * mp + 3, generator=torch.Generator().manual_seed(5))[:n * mp].to(torch.int32).view(n, mp)
        table[1, 1], table[3, 2] = -1, n * mp + 8      # rows 32 .. 34 of sequence 1, rows 93 .. 95 of sequence 3: dropped
        table = table.cuda()
    shape = (n * mp + 3, A_P) if paged else (n, A_CAP)
    wide, narrow = torch.full(shape + (576,), SENTINEL, dtype=torch.bfloat16, device="cuda"), torch.full(shape + (640,), BYTE, dtype=torch.uint8, device="cuda")
    descale = torch.tensor([0.0123], device="cuda")
    Q_wide = _append(views, wide, table, tabs, interleaved=interleaved)
    Q_narrow = _append(views, narrow, table, tabs, interleaved=interleaved, latent_descale=descale)
    assert torch.equal(Q_narrow.view(torch.int16), Q_wide.view(torch.int16))
    written = (wide != SENTINEL).any(dim=-1).cpu()
    assert written.sum() == sum(0 <= x - n_new + t < A_CAP for x in lens for t in range(n_new)) - (2 * n_new if paged else 0)
    wide, narrow = wide.cpu()[written], narrow.cpu()
    assert (narrow[~written] == BYTE).all()
    assert torch.equal(narrow[written][:, :512], ka.quantise(wide[None, None, :, :512], descale.cpu())[0, 0].view(torch.uint8))
    assert torch.equal(narrow[written][:, 512:], wide[:, 512:].contiguous().view(torch.uint8))


def test_one_captured_graph_serves_changing_lengths_and_a_changed_descale():
    """What fails if the descale is read on the host: it is written in place between replays, like seqlens_k."""
    fa, n, n_new = _fa(), 3, 2
    lens, descale = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.tensor([DESCALE], device="cuda")
    views, tabs = _append_inputs(n_new, 7, lens)
    cache = _inputs(5, 3)[1][:n, :A_CAP].contiguous().cuda()      # rows the decode may read
    ws = fa.mla_decode_workspace(n, A_H, n_new, A_CAP, 2)

    def step(C, Q_out, O, L):
        fa.mla_kv_cache_append(*views, C, *tabs, Q_out=Q_out, latent_descale=descale)
        return C, *fa.flash_attention_2_mla_decode(Q_out, C, lens, softmax_scale=SCALE, n_splits=2, O=O, L=L, workspace=ws, latent_descale=descale)

    def fresh():      # Q_out, O, L
        return tuple(torch.empty(n, A_H, n_new, *w, dtype=t, device="cuda") for w, t in (((576,), torch.bfloat16), ((512,), torch.bfloat16), ((), torch.float32)))

    step(cache.clone(), *fresh())      # the code objects load outside the capture
    torch.cuda.synchronize()
    out, graph, side = fresh(), torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(cache, *out)
    torch.cuda.current_stream().wait_stream(side)
    for now, d in (((2, 35, 64), DESCALE), ((4, 37, 97), DESCALE), ((6, 39, 96), 3.0 * DESCALE)):
        lens.copy_(torch.tensor(now, dtype=torch.int32))
        descale.fill_(d)
        C, O, L = step(cache.clone(), *fresh())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cache, C), now
        _same_bits(out[1:], (O, L), now)
