"""GPU: the KV-cache append (fa2_kv_append, fa2_kv_append_paged through kv_cache_append / kv_cache_append_paged), contiguous and
paged, bf16 and e4m3.

B = 3, H_kv = 2, d in 64, 128; a contiguous cache of 96 rows, or pages of 32 and of 96 keys, three table entries per sequence, in
a shuffled pool of 8 pages.  Every cache and pool is a VIEW into a larger allocation with a guard band before and after, the whole
allocation prefilled with random bytes; the source is a strided view of a fused [B, n_new, H_q + 2 H_kv, d] tensor.  Every check
compares the WHOLE allocation, guards included, with tests/kv_append_ref.py applied to a host copy: written rows bit for bit,
everything else untouched.  The tolerance is zero everywhere: a bf16 append copies bits, and the e4m3 bytes follow from IEEE
division, the clamp and round-to-nearest-even (for a NaN source only NaN-ness is compared: 0x7F and 0xFF are both NaN).
Then: append + decode gives the decode's bits on a cache written by the framework expression, and one captured graph of
append + decode serves three steps while lengths, source and a table entry change in place."""
import math

import pytest
import torch

import kv_append_ref as ar

pytestmark = pytest.mark.gpu

B, HQ, HKV, N_PAGES, MAX_PAGES, CAP = 3, 4, 2, 8, 3, 96
GUARD = 1024                                   # bytes before and after every cache (a multiple of 16: the view stays aligned)
UNUSED = (-1, 0x7FFFFFFF)                      # what table entries no written row needs hold
KINDS = ("contiguous", "P32", "P96")
E4M3 = ar.E4M3
KD, VD = (0.3, 0.7), (1.3, 0.9)                # a descale of its own per head and per tensor, none a power of two


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _capacity(kind):
    return CAP if kind == "contiguous" else MAX_PAGES * int(kind[1:])


class Alloc:
    """A cache inside a larger allocation: GUARD random bytes, the cache (random bytes too), GUARD random bytes."""

    def __init__(self, shape, dtype, seed):
        self.shape, self.dtype = shape, dtype
        self.n = math.prod(shape) * (1 if dtype == E4M3 else 2)
        self.host = torch.randint(0, 256, (self.n + 2 * GUARD,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        self.dev = self.host.cuda()

    def view(self, buf):
        return buf[GUARD:GUARD + self.n].view(self.dtype).view(self.shape)


def _source(n_new, d, seed, special=False):
    """(the fused [B, n_new, H_q + 2 H_kv, d] host tensor, its K and V views [B, H_kv, n_new, d]).  special: the first 32 elements of
    token 0's K rows and of the last token's V rows are kv_append_ref.special_values()."""
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(B, n_new, HQ + 2 * HKV, d, generator=g) - 0.5) * 6).bfloat16()
    if special:
        s = ar.special_values()
        x[:, 0, HQ:HQ + HKV, :s.numel()] = s
        x[:, n_new - 1, HQ + HKV:, :s.numel()] = s
    return x, *_views(x)


def _views(x):
    return x[:, :, HQ:HQ + HKV].permute(0, 2, 1, 3), x[:, :, HQ + HKV:].permute(0, 2, 1, 3)


def _table(lens, n_new, P, seed, bad=()):
    """A block table for one call: every logical page a written row needs gets a pool page of its own from a seeded
    permutation (so pages written by the call belong to one sequence each), every other entry is UNUSED; then bad: (b, p, value)."""
    perm = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.tensor([[UNUSED[(b * MAX_PAGES + p) % 2] for p in range(MAX_PAGES)] for b in range(B)], dtype=torch.int32)
    for b in range(B):
        for t in range(n_new):
            pos = ar.position(lens[b], n_new, t, MAX_PAGES * P)
            if pos is not None and int(table[b, pos // P]) in UNUSED:
                table[b, pos // P] = perm.pop()
    for b, p, value in bad:
        table[b, p] = value
    return table


def _same(got, want, nan, where):
    """The whole allocation: equal bytes; where the source was NaN (e4m3 only) a NaN code."""
    got = got.cpu()
    if nan is not None and nan.any():
        assert ((got[nan] & 0x7F) == 0x7F).all(), (where, "a NaN source must store a NaN code", got[nan].tolist()[:8])
        got = torch.where(nan, want, got)
    diff = (got != want).nonzero().flatten()
    if diff.numel():
        print(where, f"{diff.numel()} bytes differ; first at", [(int(i), int(got[i]), int(want[i])) for i in diff[:8]],
              f"(cache bytes are [{GUARD}, {got.numel() - GUARD}))")
    assert diff.numel() == 0, where


def _run(kind, d, fp8, n_new, lens, seed, descales=True, special=False, bad=(), expect=None):
    """One call against the reference on the whole allocations.  expect: how many (sequence, token) pairs the call writes."""
    fa = _fa()
    dtype = E4M3 if fp8 else torch.bfloat16
    P = None if kind == "contiguous" else int(kind[1:])
    shape = (B, HKV, CAP, d) if P is None else (N_PAGES, HKV, P, d)
    x, kn, vn = _source(n_new, d, seed, special)
    K, V = Alloc(shape, dtype, seed + 1), Alloc(shape, dtype, seed + 2)
    kd, vd = (torch.tensor(KD), torch.tensor(VD)) if fp8 and descales else (None, None)
    table = None if P is None else _table(lens, n_new, P, seed + 3, bad)
    # the reference, on host copies, and where a NaN source lands
    want = [a.host.clone() for a in (K, V)]
    nan = [torch.zeros_like(a.host) for a in (K, V)]
    flags = [torch.isnan(t).to(torch.bfloat16) for t in (kn, vn)]
    if P is None:
        written = ar.append(kn, vn, K.view(want[0]), V.view(want[1]), lens, kd, vd)
        ar.append(*flags, K.view(nan[0]), V.view(nan[1]), lens)
    else:
        written = ar.append_paged(kn, vn, K.view(want[0]), V.view(want[1]), table, lens, kd, vd)
        ar.append_paged(*flags, K.view(nan[0]), V.view(nan[1]), table, lens)
    if expect is not None:
        assert len(written) == expect, (written, expect)
    # the call
    xd = x.cuda()
    knd, vnd = _views(xd)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kw = dict(k_descale=None if kd is None else kd.cuda(), v_descale=None if vd is None else vd.cuda())
    if P is None:
        out = fa.kv_cache_append(knd, vnd, K.view(K.dev), V.view(V.dev), lens_d, **kw)
    else:
        out = fa.kv_cache_append_paged(knd, vnd, K.view(K.dev), V.view(V.dev), table.cuda(), lens_d, **kw)
    torch.cuda.synchronize()
    assert out is None
    where = (kind, d, "e4m3" if fp8 else "bf16", n_new, lens)
    for a, w, m, name in zip((K, V), want, nan, "KV"):
        _same(a.dev, w, (m != 0) if fp8 else None, where + (name,))
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16)), "the source is only read"
    return written


# ---- 1. bf16: the source bits, at row 0, mid-cache and ending at the last row
@pytest.mark.parametrize("n_new", (1, 3))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_bf16_rows_land_where_the_lengths_say(kind, d, n_new):
    cap = _capacity(kind)
    _run(kind, d, False, n_new, [n_new, cap // 2 + 2, cap], 1000 + d + n_new, expect=B * n_new)


@pytest.mark.parametrize("d", (64, 128))
def test_bf16_tokens_cross_a_page(d):
    written = _run("P32", d, False, 3, [34, 66, 3], 1100 + d, expect=9)
    assert len({page for b, _, page, _ in written if b == 0}) == 2      # rows 31 | 32, 33: two pages


# ---- 2. drops
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_tokens_outside_the_capacity_are_dropped(kind, d, fp8):
    cap = _capacity(kind)
    # length 1: two tokens dropped, one on row 0; length capacity + 2: one on the last row; length 0: none
    written = _run(kind, d, fp8, 3, [1, cap + 2, 0], 1200 + d, expect=2)
    assert sorted((b, t) for b, t, *_ in written) == [(0, 2), (1, 0)]
    _run(kind, d, fp8, 3, [-5, ar.INT_MAX, ar.INT_MIN], 1300 + d, expect=0)
    _run(kind, d, fp8, 3, [0, ar.INT_MAX - 1, ar.INT_MIN + 1], 1400 + d, expect=0)


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("values", ((-1, N_PAGES), (N_PAGES, -1), (ar.INT_MIN, ar.INT_MAX)))
def test_a_table_entry_outside_the_pool_drops_its_tokens_only(values, fp8):
    """Rows 31 | 32, 33 of every sequence: sequence 1's second page and sequence 2's first page have no valid entry."""
    written = _run("P32", 128, fp8, 3, [34, 34, 34], 1500, bad=((1, 1, values[0]), (2, 0, values[1])), expect=3 + 1 + 2)
    assert sorted((b, t) for b, t, *_ in written) == [(0, 0), (0, 1), (0, 2), (1, 0), (2, 1), (2, 2)]


# ---- 3. e4m3: the bytes of (x.float() / descale).clamp(-448, 448).to(torch.float8_e4m3fn)
@pytest.mark.parametrize("descales", (True, False), ids=("descales", "none"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_e4m3_bytes_equal_the_torch_expression(kind, d, descales):
    cap = _capacity(kind)
    _run(kind, d, True, 3, [3, cap // 2 + 2, cap], 1600 + d, descales=descales, special=True, expect=9)


def test_e4m3_special_values_on_the_device_are_the_tables():
    """The contract's byte table through the kernel itself (descale None): one row holding exactly those values."""
    fa = _fa()
    vals = torch.tensor([x for x, _ in ar.BYTE_TABLE]).bfloat16()      # (rounding to bf16 moves no entry across a byte: checked next)
    want = [b for _, b in ar.BYTE_TABLE]
    host = ar.quantise(vals.view(1, 1, 1, -1)).view(torch.uint8).flatten().tolist()
    assert all((h in ar.NAN_CODES) if w is None else h == w for h, w in zip(host, want))
    src = torch.zeros(1, 1, 1, 64, dtype=torch.bfloat16)
    src[0, 0, 0, :vals.numel()] = vals
    K = torch.full((1, 1, 32, 64), 1.0).to(E4M3).cuda()
    V = K.clone()
    fa.kv_cache_append(src.cuda(), src.cuda().clone(), K, V, torch.tensor([1], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for cache in (K, V):
        got = cache.view(torch.uint8)[0, 0, 0, :vals.numel()].tolist()
        for g, w in zip(got, want):
            assert (g in ar.NAN_CODES) if w is None else g == w, (got, want)
        assert (cache.view(torch.uint8)[0, 0, 1:] == 0x38).all()      # 1.0


# ---- 4. append then decode
def _history(kind, d, fp8, lens0, seed):
    """Caches holding lens0 tokens of history written by the framework expression (host tensors), with descales and a table."""
    P = None if kind == "contiguous" else int(kind[1:])
    cap = _capacity(kind)
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.rand(B, HKV, cap, d, generator=g) - 0.5).bfloat16()
    kd, vd = (torch.tensor(KD) / 100, torch.tensor(VD) / 100) if fp8 else (None, None)
    K, V = (ar.quantise(mk(), ds) if fp8 else mk() for ds in (kd, vd))
    if P is None:
        return K, V, None, kd, vd
    perm = torch.randperm(B * MAX_PAGES, generator=g).view(B, MAX_PAGES)      # a pool of B max_pages pages here: every page in use
    paged = lambda t: t.view(torch.uint8 if fp8 else torch.int16).view(B, HKV, MAX_PAGES, P, d).permute(0, 2, 1, 3, 4) \
        .reshape(B * MAX_PAGES, HKV, P, d)[torch.argsort(perm.flatten())].contiguous().view(t.dtype)
    return paged(K), paged(V), perm.int(), kd, vd


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", ("contiguous", "P32"))
def test_append_then_decode_equals_decode_on_a_framework_written_cache(kind, fp8):
    fa, d, n_new = _fa(), 128, 3
    lens = [5 + n_new, 40 + n_new, 93 + n_new]
    K, V, table, kd, vd = _history(kind, d, fp8, lens, 1700)
    x, kn, vn = _source(n_new, d, 1701)
    x = (x.float() / 6).bfloat16()
    kn, vn = _views(x)
    Kw, Vw = K.clone(), V.clone()                               # the framework's write: the reference model on the host
    if table is None:
        ar.append(kn, vn, Kw, Vw, lens, kd, vd)
    else:
        ar.append_paged(kn, vn, Kw, Vw, table, lens, kd, vd)
    xd = x.cuda()
    knd, vnd = _views(xd)
    Q = xd[:, :, :HQ].permute(0, 2, 1, 3).contiguous()          # the step's queries: the fused tensor's first H_q heads
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    Kd, Vd = K.cuda(), V.cuda()
    kw = dict(k_descale=None if kd is None else kd.cuda(), v_descale=None if vd is None else vd.cuda())
    if table is None:
        fa.kv_cache_append(knd, vnd, Kd, Vd, lens_d, **kw)
        got = fa.flash_attention_2_decode(Q, Kd, Vd, lens_d, **kw)
        want = fa.flash_attention_2_decode(Q, Kw.cuda(), Vw.cuda(), lens_d, **kw)
    else:
        fa.kv_cache_append_paged(knd, vnd, Kd, Vd, table.cuda(), lens_d, **kw)
        got = fa.flash_attention_2_decode_paged(Q, Kd, Vd, table.cuda(), lens_d, **kw)
        want = fa.flash_attention_2_decode_paged(Q, Kw.cuda(), Vw.cuda(), table.cuda(), lens_d, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert not torch.isnan(got[0].float()).any() and torch.isfinite(got[1]).all()
    assert not torch.equal(Kd.cpu().view(torch.uint8), K.view(torch.uint8))      # (the append did write)


# ---- 5. one captured graph of append + decode
def test_one_captured_graph_of_append_and_decode_serves_three_steps():
    """Paged e4m3, one token per step.  Captured once on one stream with a caller workspace, O, L and a static source buffer; between
    replays the lengths are bumped, the source is overwritten and a table entry is assigned as a sequence crosses into a new page,
    all IN PLACE.  Every replay leaves the pools, O and L bit for bit what the same two eager calls leave on a copy."""
    fa, d, P, n_new = _fa(), 128, 32, 1
    g = torch.Generator().manual_seed(1800)
    pools = [torch.randint(0, 0x78, (N_PAGES, HKV, P, d), generator=g, dtype=torch.uint8).cuda().view(E4M3) for _ in range(2)]
    table = torch.tensor([[5, -1, -1], [2, -1, -1], [7, -1, -1]], dtype=torch.int32, device="cuda")
    lens = torch.tensor([30, 31, 5], dtype=torch.int32, device="cuda")
    kd, vd = (torch.tensor(KD) / 100).cuda(), (torch.tensor(VD) / 100).cuda()
    x = torch.zeros(B, n_new, HQ + 2 * HKV, d, dtype=torch.bfloat16, device="cuda")
    kn, vn = _views(x)
    q_view = x[:, :, :HQ].permute(0, 2, 1, 3)
    Q = torch.empty(B, HQ, n_new, d, dtype=torch.bfloat16, device="cuda")
    O, L = torch.empty_like(Q), torch.empty(B, HQ, n_new, dtype=torch.float32, device="cuda")
    ws = fa.decode_workspace(B, HQ, HKV, n_new, MAX_PAGES * P, d, 2)
    assert ws.numel() > 0

    def step(Kp, Vp, O, L, ws):
        fa.kv_cache_append_paged(kn, vn, Kp, Vp, table, lens, kd, vd)
        return fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, n_splits=2, O=O, L=L, workspace=ws, k_descale=kd, v_descale=vd)

    step(*pools, O, L, ws)      # (code objects load outside the capture)
    torch.cuda.synchronize()
    eager = [p.clone() for p in pools]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(*pools, O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    assign = {1: (1, 1, 0), 2: (0, 1, 3)}      # before step s: sequence b's logical page p becomes pool page v
    for s in range(3):
        lens += n_new                           # 31 32 6 | 32 33 7 | 33 34 8: sequence 1 reaches row 32 at step 1, sequence 0 at step 2
        if s in assign:
            b, p, v = assign[s]
            table[b, p] = v
        x.copy_(((torch.rand(x.shape, generator=g) - 0.5) * 2).bfloat16().cuda())
        Q.copy_(q_view)
        O.view(torch.int16).fill_(0x5A5A)
        L.view(torch.int32).fill_(0x5A5A5A5A)
        graph.replay()
        torch.cuda.synchronize()
        Oe, Le = step(*eager, torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))
        torch.cuda.synchronize()
        for got, want in zip(pools, eager):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), ("pool", s)
        assert torch.equal(O.view(torch.int16), Oe.view(torch.int16)) and torch.equal(L.view(torch.int32), Le.view(torch.int32)), s
        assert not torch.isnan(O.float()).any()
    # the rows the three steps wrote are the quantised sources' (the last step's are still in the buffer)
    row = ar.quantise(kn.cpu(), kd.cpu()).view(torch.uint8)
    assert torch.equal(pools[0].cpu().view(torch.uint8)[3, :, 0], row[0, :, 0])      # sequence 0: row 32 = row 0 of pool page 3
