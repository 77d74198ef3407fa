"""GPU: the MLA decode and the MLA latent-cache append where no test had taken them (tests/mla_ref.py has the inputs, the float64
reference and the append's model; tests/test_mla_rows_reference.py certifies on the CPU that the kernel's emulated data flow uses
at most 0.75 of every gate on every input of this file).

THE REGIMES.  `peaked`, `spikes`, `scale-one` and `low-level` at (H, q_len) = (11, 3): lengths 300 and 1100 side by side in caches
of 1120 rows whose tails hold finite garbage, both masks, contiguous and behind pages of 32, 1, 7 and 0 splits.  The MLA kernel
had only seen a near-flat softmax: no running maximum that jumps by 100, no split whose weight underflows beside another, no L
below -88.
THE SHAPES, on tests/test_gpu_mla_decode.py's uniform inputs and lengths: (11, 3) -- M = 33, head 10's tokens straddle the row
block's edge, so the causal mask needs rho % q_len and not the row within the block --, (2, 17) (M = 34) and (128, 1), the model's
own four row blocks; both masks, splits 0, 1, 2 and 5, contiguous and pages of 32.
THE CLAMPS the header promises: seqlens_k below 0 and above the capacity; table entries IN USE outside [0, n_pages).
PAST 4 GiB: a pool whose last pages start beyond byte 2^32, a contiguous cache whose last two sequences do, and both appends
writing rows there.
THE APPEND'S SHAPES: a pass of eight heads plus one (H = 9) and sixteen passes (H = 128).

GATES, all against the float64 reference: tests/decode_rows_ref.py's row gate on every row of O, decode_ref's L gates, the keyless
rows exactly; paged equals contiguous bit for bit; the append equals its model bit for bit."""
import numpy as np
import pytest
import torch

import decode_ref as dr
import decode_rows_ref as rows
import mla_ref as mr
import qk_norm_ref as nr
import rope_ref as rr

pytestmark = pytest.mark.gpu

MASKS = ((True, "causal"), (False, "full"))
BIG_PAGES = 116600            # pages of 32 keys: 4.30 GB; page 116509 is the first to start beyond byte 2^32
FIRST_FAR_PAGE = -(-2 ** 32 // (mr.PAGE * mr.D * 2))
FAR_CAP, FAR_B = mr.FAR_CAP, mr.FAR_B
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _check(where, O, L, ref):
    O = O.float().cpu().numpy()
    e = dr.errors(O, L.cpu().numpy(), ref)
    print(where, f"dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert e[1] <= dr.L_ABS and e[2] <= dr.L_ABS_LARGE and e[3], (where, e)
    return rows.check(where, O, ref)


def _both(where, Q, C, pool, table, lens, scale, causal, n_splits, ref):
    """The contiguous call inside every gate, the paged call its bits; returns the row ratio and the result."""
    fa = _fa()
    got = fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=scale, causal=causal, n_splits=n_splits)
    top = _check(where, *got, ref)
    _same_bits(fa.flash_attention_2_mla_decode_paged(Q, pool, table, lens, softmax_scale=scale, causal=causal, n_splits=n_splits), got, (where, "paged"))
    return top, got


# ------------------------------------------------------------------------------------------------ the regimes
@pytest.mark.parametrize("regime", mr.REGIMES)
def test_the_regimes(regime):
    Q, C, scale, lens = mr.regime_inputs(regime)
    pool, table = (t.cuda() for t in mr.paged(C, mr.LENS, mr.PAGE, 576 + mr.REGIMES.index(regime)))
    Qd, Cd, ld = Q.cuda(), C.cuda(), lens.cuda()
    top = 0.0
    for causal, name in MASKS:
        ref = mr.regime_reference(regime, causal)
        for n_splits in mr.SPLITS:
            top = max(top, _both(f"mla {regime} {name} splits {n_splits}", Qd, Cd, pool, table, ld, scale, causal, n_splits, ref)[0])
    print(f"ROWS-GPU mla {regime}: largest row ratio {top:.3f}")


# ------------------------------------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("H,nq", mr.NEW_SHAPES)
def test_the_shapes(H, nq):
    Q, C = mr.uniform_inputs(H, nq)
    pool, table = (t.cuda() for t in mr.paged(C, mr.UNIFORM_LENS, mr.PAGE, 31 + H))
    Qd, Cd, ld = Q.cuda(), C.cuda(), torch.tensor(mr.UNIFORM_LENS, dtype=torch.int32, device="cuda")
    top = 0.0
    for causal, name in MASKS:
        ref = mr.uniform_reference(H, nq, causal)
        for n_splits in mr.UNIFORM_SPLITS:
            top = max(top, _both(f"mla H {H} nq {nq} {name} splits {n_splits}", Qd, Cd, pool, table, ld, mr.UNIFORM_SCALE, causal, n_splits, ref)[0])
    print(f"ROWS-GPU mla uniform H {H} nq {nq}: largest row ratio {top:.3f}")


# ------------------------------------------------------------------------------------------------ the clamps
def test_seqlens_are_clamped_on_the_device():
    fa = _fa()
    H, nq = mr.NEW_SHAPES[0]
    Q, C = (t[:4] for t in mr.uniform_inputs(H, nq))
    cap = mr.UNIFORM_CAP
    pool, table = (t.cuda() for t in mr.paged(C, (cap,) * 4, mr.PAGE, 9))      # every page holds rows: the clamped call reads them all
    Qd, Cd = Q.cuda(), C.cuda()
    stored, clamped = (-5, INT_MIN, cap + 7, INT_MAX), (0, 0, cap, cap)
    bad, good = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (stored, clamped))
    for causal, name in MASKS:
        ref = mr.reference64(Q, C, clamped, mr.UNIFORM_SCALE, causal)
        for n_splits in (0, 1, 5):
            kw = dict(softmax_scale=mr.UNIFORM_SCALE, causal=causal, n_splits=n_splits)
            want = fa.flash_attention_2_mla_decode(Qd, Cd, good, **kw)
            _check(f"mla clamped lengths {name} splits {n_splits}", *want, ref)
            _same_bits(fa.flash_attention_2_mla_decode(Qd, Cd, bad, **kw), want, (name, n_splits))
            _same_bits(fa.flash_attention_2_mla_decode_paged(Qd, pool, table, bad, **kw), want, (name, n_splits, "paged"))
    assert (want[0][:2] == 0).all() and torch.isneginf(want[1][:2]).all()


def test_table_entries_in_use_are_clamped():
    """Sequence 9 (384 keys) keeps its rows 96 ..+32 in page 0 and sequence 8 (300 keys) its rows 64 ..+32 in the last page; the
    table that says -1 (INT_MIN) and n_pages + 5 (INT_MAX) there gives the bits of the table that says 0 and n_pages - 1."""
    fa = _fa()
    H, nq = mr.NEW_SHAPES[0]
    Q, C = mr.uniform_inputs(H, nq)
    B, P, mp = len(mr.UNIFORM_LENS), mr.PAGE, mr.UNIFORM_CAP // mr.PAGE
    n_pages = B * mp + 3
    table = (torch.randperm(n_pages - 2, generator=torch.Generator().manual_seed(17)) + 1)[:B * mp].to(torch.int32).view(B, mp)
    table[9, 3], table[8, 2] = 0, n_pages - 1
    pool = torch.zeros(n_pages, P, mr.D, dtype=torch.bfloat16)
    for b, n in enumerate(mr.UNIFORM_LENS):
        for p in range(mp):
            if p * P < n:
                pool[table[b, p], :min(P, n - p * P)] = C[b, p * P:min((p + 1) * P, n)]
    assert (pool[0] != 0).any() and (pool[n_pages - 1] != 0).any()
    Qd, Cd, pool, ld = Q.cuda(), C.cuda(), pool.cuda(), torch.tensor(mr.UNIFORM_LENS, dtype=torch.int32, device="cuda")
    for causal, name in MASKS:
        ref = mr.uniform_reference(H, nq, causal)
        for n_splits in (1, 5):
            kw = dict(softmax_scale=mr.UNIFORM_SCALE, causal=causal, n_splits=n_splits)
            want = fa.flash_attention_2_mla_decode_paged(Qd, pool, table.cuda(), ld, **kw)
            _check(f"mla clamped table {name} splits {n_splits}", *want, ref)
            _same_bits(want, fa.flash_attention_2_mla_decode(Qd, Cd, ld, **kw), (name, n_splits, "contiguous"))
            for low, high in ((-1, n_pages + 5), (INT_MIN, INT_MAX)):
                bad = table.clone()
                bad[9, 3], bad[8, 2] = low, high
                _same_bits(fa.flash_attention_2_mla_decode_paged(Qd, pool, bad.cuda(), ld, **kw), want, (name, n_splits, low, high))


# ------------------------------------------------------------------------------------------------ past 4 GiB
def test_a_pool_past_4_gib():
    """The pages in use are the pool's last ones (every one starts beyond byte 2^32) and page 0; the rest is never written."""
    fa = _fa()
    H, nq = mr.NEW_SHAPES[0]
    Q, C = mr.uniform_inputs(H, nq)
    B, P, mp = len(mr.UNIFORM_LENS), mr.PAGE, mr.UNIFORM_CAP // mr.PAGE
    assert (FIRST_FAR_PAGE - 1) * P * mr.D * 2 < 2 ** 32 <= FIRST_FAR_PAGE * P * mr.D * 2 and BIG_PAGES * P * mr.D * 2 > 4.29e9
    pool = torch.empty(BIG_PAGES, P, mr.D, dtype=torch.bfloat16, device="cuda")
    table = torch.full((B, mp), 5, dtype=torch.int32)
    page, Cd = BIG_PAGES, C.cuda()
    for b, n in enumerate(mr.UNIFORM_LENS):
        for p in range(mp):
            if p * P < n:
                page -= 1
                table[b, p] = page
                pool[page, :min(P, n - p * P)] = Cd[b, p * P:min((p + 1) * P, n)]
    assert page >= FIRST_FAR_PAGE
    table[9, 0] = 0
    pool[0] = Cd[9, :P]
    Qd, ld, table = Q.cuda(), torch.tensor(mr.UNIFORM_LENS, dtype=torch.int32, device="cuda"), table.cuda()
    for causal, name in MASKS:
        for n_splits in (1, 5):
            kw = dict(softmax_scale=mr.UNIFORM_SCALE, causal=causal, n_splits=n_splits)
            got = fa.flash_attention_2_mla_decode_paged(Qd, pool, table, ld, **kw)
            _check(f"mla pool past 4 GiB {name} splits {n_splits}", *got, mr.uniform_reference(H, nq, causal))
            _same_bits(got, fa.flash_attention_2_mla_decode(Qd, Cd, ld, **kw), (name, n_splits))


def test_a_contiguous_cache_past_4_gib():
    fa = _fa()
    Q, C = mr.far_inputs()
    assert (FAR_B - 2) * FAR_CAP * mr.D * 2 > 2 ** 32 and FAR_CAP * mr.D * 2 <= INT_MAX
    cache = torch.empty(FAR_B, FAR_CAP, mr.D, dtype=torch.bfloat16, device="cuda")
    cache[FAR_B - 2:, :mr.UNIFORM_CAP] = C.cuda()
    Qd = ((torch.rand(FAR_B, 1, 1, mr.D, generator=torch.Generator().manual_seed(3)) - 0.5) * 12).bfloat16()
    Qd[FAR_B - 2:] = Q
    Qd, ld = Qd.cuda(), torch.tensor((0,) * (FAR_B - 2) + mr.FAR_LENS, dtype=torch.int32, device="cuda")
    for causal, name in MASKS:
        for n_splits in (0, 1, 5):
            O, L = fa.flash_attention_2_mla_decode(Qd, cache, ld, softmax_scale=mr.UNIFORM_SCALE, causal=causal, n_splits=n_splits)
            assert (O[:FAR_B - 2].view(torch.int16) == 0).all() and torch.isneginf(L[:FAR_B - 2]).all(), (name, n_splits)
            _check(f"mla cache past 4 GiB {name} splits {n_splits}", O[FAR_B - 2:], L[FAR_B - 2:], mr.far_reference(causal))


def _all_sentinel(t):
    want = torch.tensor(mr.APPEND_SENTINEL, dtype=torch.bfloat16).view(torch.int16).item()
    return all(bool((c.view(torch.int16) == want).all()) for c in t.chunk(8))


def _append(paged, views, cache, table, tabs, lens, interleaved, Q_out):
    fa = _fa()
    if paged:
        return fa.mla_kv_cache_append_paged(*views, cache, table, *tabs, lens, interleaved=interleaved, Q_out=Q_out)
    return fa.mla_kv_cache_append(*views, cache, *tabs, lens, interleaved=interleaved, Q_out=Q_out)


def _same(got, want, where):
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), where


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_the_append_writes_past_4_gib(paged):
    """Contiguous: 1024 sequences of 4096 rows (4.83 GB), only the last two own tokens -- rows 4094 and 4095 of sequence 1022 and
    rows 35 and 36 of sequence 1023.  Paged: three sequences whose nine pages are the last nine of a pool of 4.30 GB."""
    H, n_new = 2, 2
    if paged:
        B, mp, cap = 3, 3, 96
        lens = (n_new, 35, 96)
        small = torch.arange(B * mp, dtype=torch.int32).view(B, mp)
        table = (BIG_PAGES - 1 - small).cuda()
        assert BIG_PAGES - B * mp >= FIRST_FAR_PAGE
        shape, keep = (BIG_PAGES, mr.PAGE, mr.D), B
    else:
        B, cap = 1024, 4096
        lens = (0,) * (B - 2) + (cap, 37)
        small = table = None
        assert (B - 2) * cap * mr.D * 2 > 2 ** 32
        shape, keep = (B, cap, mr.D), 2
    host = mr.append_sources(B, H, n_new, 4096 + paged)
    w, (cos, sin) = nr.weights(512, nr.WEIGHT_SEED)[1], rr.random_tables(cap, 64, 9)
    # the model, on the sequences that own tokens alone
    model = torch.full((B * mp, mr.PAGE, mr.D) if paged else (keep, cap, mr.D), mr.APPEND_SENTINEL, dtype=torch.bfloat16)
    want = mr.append_model(model, small, tuple(v[B - keep:] for v in mr.append_views(*host)), lens[B - keep:], w, cos, sin, paged)
    assert (model != mr.APPEND_SENTINEL).any(dim=-1).sum() == 2 * n_new + (n_new if paged else 0)
    cache = torch.full(shape, mr.APPEND_SENTINEL, dtype=torch.bfloat16, device="cuda")
    Q_out = torch.full((B, H, n_new, mr.D), float("nan"), dtype=torch.bfloat16, device="cuda")
    views = mr.append_views(*(x.cuda() for x in host))
    _append(paged, views, cache, table, (cos.cuda(), sin.cuda(), w.cuda(), nr.EPS), torch.tensor(lens, dtype=torch.int32, device="cuda"), paged, Q_out)
    _same(Q_out[B - keep:], want, "Q_out")
    assert (Q_out[:B - keep].view(torch.int16) == 0).all()      # a dropped position: +0.0
    if paged:
        _same(cache[BIG_PAGES - B * mp:].flip(0), model, "the last pages")
        assert _all_sentinel(cache[:BIG_PAGES - B * mp])
    else:
        _same(cache[B - 2:], model, "the last two sequences")
        assert _all_sentinel(cache[:B - 2])


# ------------------------------------------------------------------------------------------------ the append's shapes
APPEND_CAP = 96


@pytest.mark.parametrize("H,n_new", ((9, 2), (128, 1)))
@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "interleaved"))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_the_append_at_a_pass_plus_one_head_and_at_sixteen_passes(paged, interleaved, H, n_new):
    """tests/test_gpu_mla_append.py's batch (a first row, a page edge, the last row, one token past the capacity, one before row
    0, every token dropped; a -1 and a >= n_pages table entry on pages tokens fall in) at H = 9 and H = 128."""
    lens = (n_new, 35, 64, 96, 97, n_new - 1, 99 + n_new)
    B, mp = len(lens), APPEND_CAP // mr.PAGE
    host = mr.append_sources(B, H, n_new, 100 * H + n_new)
    w, (cos, sin) = nr.weights(512, nr.WEIGHT_SEED)[1], rr.random_tables(APPEND_CAP, 64, 9)
    table = None
    if paged:
        table = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(5))[:B * mp].to(torch.int32).view(B, mp)
        table[1, 1], table[3, 2] = -1, B * mp + 8      # rows 32 .. 34 of sequence 1, rows 93 .. 95 of sequence 3
    cache = torch.full((B * mp + 3, mr.PAGE, mr.D) if paged else (B, APPEND_CAP, mr.D), mr.APPEND_SENTINEL, dtype=torch.bfloat16)
    dev_cache = cache.cuda()
    want = mr.append_model(cache, table, mr.append_views(*host), lens, w, cos, sin, interleaved)
    Q_out = torch.full((B, H, n_new, mr.D), float("nan"), dtype=torch.bfloat16, device="cuda")
    got = _append(paged, mr.append_views(*(x.cuda() for x in host)), dev_cache, None if table is None else table.cuda(),
                  (cos.cuda(), sin.cuda(), w.cuda(), nr.EPS), torch.tensor(lens, dtype=torch.int32, device="cuda"), interleaved, Q_out)
    assert got is Q_out
    _same(dev_cache, cache, "cache")      # unwritten rows keep the sentinel
    _same(Q_out, want, "Q_out")           # every row written: no NaN is left
    assert (want[4, :, n_new - 1] == 0).all() and (want[0, H - 1] != 0).any() and (cache != mr.APPEND_SENTINEL).any()
