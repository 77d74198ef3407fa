"""GPU: MLA decode attention (fa2_forward_mla_decode / _paged through flash_attention_2_mla_decode / _paged) against a float64
reference on the bf16 inputs.  One batch carries the lengths 0, 1, 31, 32, 33, 127, 128, 129, 300 and the capacity (384) side by
side; (H, N_q) = (16, 1) a part-filled row block, (16, 2) a full one with a causal edge, (5, 3) padding rows with row % N_q,
(40, 1) two row blocks with the second part-filled.  n_splits 2 and 5 leave empty splits on the short sequences.
Gates: O per row, tests/decode_rows_ref.py's KAPPA u quad + u |O_ref| unchanged (P is rounded once per (row, key), one output
rounding; the three extra fp32 adds of the S partials are at the 2^-24 level); L decode_ref's 1e-4 (|L| <= 25) / 1e-3; the
-inf rows exactly the reference's with O exactly 0; and bit equalities without a tolerance."""
import functools

import numpy as np
import pytest
import torch

import decode_ref as dr
import decode_rows_ref as rows

pytestmark = pytest.mark.gpu

N_CAP, SCALE = 384, 0.0913      # 12 pages of 32 keys, 4 of 96; the scale is the default of no width
LENS = (0, 1, 31, 32, 33, 127, 128, 129, 300, N_CAP)
SHAPES = ((16, 1), (16, 2), (5, 3), (40, 1))
SPLITS = (0, 1, 2, 5)
B = len(LENS)


def _fa():
    import cuda_flashattention_amd as fa
    return fa


@functools.lru_cache(maxsize=None)
def _inputs(H, nq):
    """Host Q [B, H, nq, 576] (scores of standard deviation 2: no flat softmax) and the latent cache [B, N_CAP, 576], finite
    everywhere; the last two sequences start with the same 96 rows (the page they share)."""
    g = torch.Generator().manual_seed(576 + 7 * H + nq)
    Q = ((torch.rand(B, H, nq, 576, generator=g) - 0.5) * 12).bfloat16()
    C = (torch.rand(B, N_CAP, 576, generator=g) - 0.5).bfloat16()
    C[B - 1, :96] = C[B - 2, :96]
    return Q, C


@functools.lru_cache(maxsize=None)
def _reference(H, nq, causal):
    Q, C = _inputs(H, nq)
    O, L = np.zeros((B, H, nq, 512)), np.full((B, H, nq), -np.inf)
    for b, n in enumerate(LENS):
        s = SCALE * (Q[b].double() @ C[b, :n].double().T)                              # [H, nq, n]
        if causal:
            s = s.masked_fill(torch.arange(n)[None, :] > torch.arange(nq)[:, None] + n - nq, -np.inf)
        Lb = torch.logsumexp(s, dim=-1) if n else torch.full((H, nq), -np.inf)
        P = torch.exp(s - Lb.masked_fill(Lb == -np.inf, 0.0)[..., None])
        O[b], L[b] = (P @ C[b, :n, :512].double()).numpy(), Lb.numpy()
    return rows.Ref(O, L, rows.quad64(Q, C[:, None], C[:, None, :, :512], LENS, SCALE, causal, None))


@functools.lru_cache(maxsize=None)
def _dev(H, nq):
    Q, C = _inputs(H, nq)
    return Q.cuda(), C.cuda(), torch.tensor(LENS, dtype=torch.int32, device="cuda")


def _pool(C, P, unused=None, fill=0.0):
    """A pool [n_pages, P, 576] and a shuffled table of the host cache C: page p of sequence b holds rows p P ..+P up to the length,
    `fill` past it and in the pages nothing was copied to; the last two sequences share their first page; the entries beyond
    ceil(len / P) are `unused` (None: valid pages)."""
    mp = N_CAP // P
    g = torch.Generator().manual_seed(31 + P)
    table = torch.randperm(B * mp + 3, generator=g)[:B * mp].to(torch.int32).view(B, mp)
    table[B - 1, 0] = table[B - 2, 0]
    pool = torch.full((B * mp + 3, P, 576), fill, dtype=torch.bfloat16)
    for b, n in enumerate(LENS):
        for p in range(mp):
            if p * P < n:
                pool[table[b, p], :min(P, n - p * P)] = C[b, p * P:min((p + 1) * P, n)]
            elif unused is not None:
                table[b, p] = unused[(b + p) % len(unused)]
    return pool.cuda(), table.cuda()


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _check(where, O, L, ref):
    O = O.float().cpu().numpy()
    e = dr.errors(O, L.cpu().numpy(), ref)
    print(where, f"dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert e[1] <= dr.L_ABS and e[2] <= dr.L_ABS_LARGE and e[3], (where, e)
    rows.check(where, O, ref)


@pytest.mark.parametrize("causal", (True, False), ids=("causal", "full"))
@pytest.mark.parametrize("H,nq", SHAPES)
def test_parity_with_the_reference_and_paged_equals_contiguous(H, nq, causal):
    fa = _fa()
    Q, C, lens = _dev(H, nq)
    ref = _reference(H, nq, causal)
    pools = {P: _pool(_inputs(H, nq)[1], P) for P in (32, 96)}
    for ns in SPLITS:
        got = fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, causal=causal, n_splits=ns)
        _check(f"H {H} nq {nq} causal {causal} splits {ns}", *got, ref)
        for P, (pool, table) in pools.items():
            paged = fa.flash_attention_2_mla_decode_paged(Q, pool, table, lens, softmax_scale=SCALE, causal=causal, n_splits=ns)
            _same_bits(paged, got, (H, nq, causal, ns, P))
    full = fa.flash_attention_2_mla_decode(Q[-1:], C[-1:], None, softmax_scale=SCALE, causal=causal, n_splits=2)      # seqlens_k = None
    _same_bits(full, fa.flash_attention_2_mla_decode(Q[-1:], C[-1:], lens[-1:], softmax_scale=SCALE, causal=causal, n_splits=2), "no lengths")


@pytest.mark.parametrize("H,nq", ((16, 2), (40, 1)))
def test_garbage_past_the_lengths_changes_no_bit(H, nq):
    fa = _fa()
    Q, _, lens = _dev(H, nq)
    past = (torch.arange(N_CAP)[None, :] >= torch.tensor(LENS)[:, None])[..., None]
    zeros, nans, huge = (torch.where(past, torch.tensor(f, dtype=torch.bfloat16), _inputs(H, nq)[1]) for f in (0.0, float("nan"), 3e38))
    for ns in (1, 2, 5):
        want = fa.flash_attention_2_mla_decode(Q, zeros.cuda(), lens, softmax_scale=SCALE, n_splits=ns)
        _check(f"H {H} nq {nq} zeros splits {ns}", *want, _reference(H, nq, True))
        for f, host in ((float("nan"), nans), (3e38, huge)):
            _same_bits(fa.flash_attention_2_mla_decode(Q, host.cuda(), lens, softmax_scale=SCALE, n_splits=ns), want, (ns, f))
            for P in (32, 96):
                pool, table = _pool(host, P, unused=(-1, 2 ** 31 - 1, -2 ** 31, B * (N_CAP // P) + 3), fill=f)
                _same_bits(fa.flash_attention_2_mla_decode_paged(Q, pool, table, lens, softmax_scale=SCALE, n_splits=ns), want, (ns, f, P))


def test_one_captured_graph_serves_changing_lengths():
    fa = _fa()
    H, nq = 16, 2
    Q, C, _ = _dev(H, nq)
    lens = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    O, L = torch.empty(B, H, nq, 512, dtype=torch.bfloat16, device="cuda"), torch.empty(B, H, nq, dtype=torch.float32, device="cuda")
    ws = fa.mla_decode_workspace(B, H, nq, N_CAP, 2)
    run = lambda O, L, ws: fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, n_splits=2, O=O, L=L, workspace=ws)
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
        O.zero_(), L.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same_bits((O, L), run(torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws)), ("replay", step))


def test_a_dirty_workspace_changes_no_bit():
    fa = _fa()
    Q, C, lens = _dev(40, 1)
    want = fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, n_splits=5)
    for _ in range(2):
        ws = fa.mla_decode_workspace(B, 40, 1, N_CAP, 5).view(torch.float32).fill_(float("nan")).view(torch.uint8)
        _same_bits(fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, n_splits=5, workspace=ws), want, "dirty workspace")
