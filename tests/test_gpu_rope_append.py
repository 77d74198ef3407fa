"""GPU: the rotary-embedding KV-cache append (fa2_rope_kv_append, fa2_rope_kv_append_paged through rope_kv_cache_append /
rope_kv_cache_append_paged), contiguous and paged, bf16 and e4m3, both pair forms, full and partial rot_dim.

B = 3, H_q = 4, H_kv = 2, d in 64, 128; a contiguous cache of 96 rows, or pages of 32 keys, three table entries per sequence, in a
shuffled pool of 8 pages.  The source is ONE fused [B, n_new, H_q + 2 H_kv, d] tensor whose Q, K and V slices are passed as views.
Every cache, pool and Q_out is a VIEW between 1024-byte guard bands in an allocation of random bytes, and every check compares
the WHOLE allocation with tests/rope_ref.py applied to a host copy.  The tolerance is ZERO everywhere: the contract is IEEE
operations only (include/fa2_rope_mi355x.h, ARITHMETIC), and no source here holds a NaN.  The cos/sin tables are seeded random
fp32 in (-1, 1) with a distinct value per (table, position, column) -- not a real rotation --, so a wrong row, a wrong column,
swapped tables, a wrong sign or a wrong partner each changes bits."""
import math

import pytest
import torch

import kv_append_ref as ar
import rope_ref as rr

pytestmark = pytest.mark.gpu

B, HQ, HKV, N_PAGES, MAX_PAGES, CAP, PAGE = 3, 4, 2, 8, 3, 96, 32
GUARD = 1024                                   # bytes before and after every cache and Q_out (a multiple of 16: the view stays aligned)
UNUSED = (-1, 0x7FFFFFFF)                      # what table entries no written row needs hold
KINDS = ("contiguous", "P32")
E4M3 = ar.E4M3
KD, VD = (0.3, 0.7), (1.3, 0.9)                # a descale of its own per head and per tensor, none a power of two
FORMS = ((False, "half"), (True, "pairs"))


def _fa():
    import cuda_flashattention_amd as fa
    return fa


class Alloc:
    """A tensor inside a larger allocation: GUARD random bytes, the tensor (random bytes too), GUARD random bytes."""

    def __init__(self, shape, dtype, seed):
        self.shape, self.dtype = shape, dtype
        self.n = math.prod(shape) * (1 if dtype == E4M3 else 2)
        self.host = torch.randint(0, 256, (self.n + 2 * GUARD,), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        self.dev = self.host.cuda()

    def view(self, buf):
        return buf[GUARD:GUARD + self.n].view(self.dtype).view(self.shape)


def _views(x):
    """Q, K, V [B, H, n_new, d] views of the fused [B, n_new, H_q + 2 H_kv, d] tensor."""
    return tuple(t.permute(0, 2, 1, 3) for t in (x[:, :, :HQ], x[:, :, HQ:HQ + HKV], x[:, :, HQ + HKV:]))


def _source(n_new, d, seed, scale=6.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, n_new, HQ + 2 * HKV, d, generator=g) - 0.5) * scale).bfloat16()


def _table(lens, n_new, seed, bad=()):
    """A block table for one call: every logical page a written row needs gets a pool page of its own from a seeded
    permutation (so pages written by the call belong to one sequence each), every other entry is UNUSED; then bad: (b, p, value)."""
    perm = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.tensor([[UNUSED[(b * MAX_PAGES + p) % 2] for p in range(MAX_PAGES)] for b in range(B)], dtype=torch.int32)
    for b in range(B):
        for t in range(n_new):
            pos = ar.position(lens[b], n_new, t, MAX_PAGES * PAGE)
            if pos is not None and int(table[b, pos // PAGE]) in UNUSED:
                table[b, pos // PAGE] = perm.pop()
    for b, p, value in bad:
        table[b, p] = value
    return table


def _same(got, want, where):
    """The whole allocation, guards included: equal bytes."""
    got = got.cpu()
    diff = (got != want).nonzero().flatten()
    if diff.numel():
        print(where, f"{diff.numel()} bytes differ; first at", [(int(i), int(got[i]), int(want[i])) for i in diff[:8]],
              f"(the tensor's bytes are [{GUARD}, {got.numel() - GUARD}))")
    assert diff.numel() == 0, where


def _run(kind, d, fp8, n_new, lens, rot, interleaved, seed, bad=(), with_q=True, x=None, tables=None, expect=None):
    """One call against the model on the whole allocations of K, V and Q_out.  Returns what the later checks look at."""
    fa = _fa()
    dtype = E4M3 if fp8 else torch.bfloat16
    paged = kind != "contiguous"
    shape = (N_PAGES, HKV, PAGE, d) if paged else (B, HKV, CAP, d)
    x = _source(n_new, d, seed) if x is None else x
    q, kn, vn = _views(x)
    cos, sin = rr.random_tables(CAP, rot, seed + 5) if tables is None else tables
    K, V, Qo = Alloc(shape, dtype, seed + 1), Alloc(shape, dtype, seed + 2), Alloc((B, HQ, n_new, d), torch.bfloat16, seed + 4)
    kd, vd = (torch.tensor(KD), torch.tensor(VD)) if fp8 else (None, None)
    table = _table(lens, n_new, seed + 3, bad) if paged else None
    # the model, on host copies
    want = [a.host.clone() for a in (K, V, Qo)]
    if paged:
        q_ref, written = rr.rope_append_paged(q if with_q else None, kn, vn, K.view(want[0]), V.view(want[1]), table, cos, sin, lens,
                                              interleaved, kd, vd)
    else:
        q_ref, written = rr.rope_append(q if with_q else None, kn, vn, K.view(want[0]), V.view(want[1]), cos, sin, lens, interleaved, kd, vd)
    if with_q:
        Qo.view(want[2]).view(torch.int16).copy_(q_ref.view(torch.int16))
    if expect is not None:
        assert len(written) == expect, (written, expect)
    # the call
    xd = x.cuda()
    qd, knd, vnd = _views(xd)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kw = dict(interleaved=interleaved, k_descale=None if kd is None else kd.cuda(), v_descale=None if vd is None else vd.cuda(),
              Q_out=Qo.view(Qo.dev) if with_q else None)
    if paged:
        out = fa.rope_kv_cache_append_paged(qd if with_q else None, knd, vnd, K.view(K.dev), V.view(V.dev), table.cuda(), cos.cuda(),
                                            sin.cuda(), lens_d, **kw)
    else:
        out = fa.rope_kv_cache_append(qd if with_q else None, knd, vnd, K.view(K.dev), V.view(V.dev), cos.cuda(), sin.cuda(), lens_d, **kw)
    torch.cuda.synchronize()
    assert (out.data_ptr() == Qo.view(Qo.dev).data_ptr()) if with_q else out is None
    where = (kind, d, "e4m3" if fp8 else "bf16", n_new, lens, rot, "pairs" if interleaved else "half")
    for a, w, name in zip((K, V, Qo), want, ("K", "V", "Q_out")):
        _same(a.dev, w, where + (name,))
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16)), "the source is only read"
    return dict(written=written, q_out=Qo.view(Qo.dev).cpu(), q_ref=q_ref, K=K, V=V, table=table, cos=cos, sin=sin, x=x)


# ---- 1. every shape of the rotation: token groups, rot_dim, pair form, cache dtype, layout
@pytest.mark.parametrize("n_new", (1, 3, 19))
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_rotated_rows_land_where_the_lengths_say(kind, d, fp8, n_new):
    """n_new = 19: three token groups at d = 128 (8 + 8 + 3) and two at d = 64 (16 + 3), the last one ragged.  The lengths put
    tokens on row 0, mid-cache (rows 31 .. 49: across a page) and ending on the last row."""
    for rot in (d, d // 2, 16):
        for interleaved, _ in FORMS:
            r = _run(kind, d, fp8, n_new, [n_new, CAP // 2 + 2, CAP], rot, interleaved, 2000 + d + 7 * n_new + rot, expect=B * n_new)
            assert not (r["q_out"].view(torch.int16) == 0).all(dim=-1).any()


# ---- 2. the products are not contracted
@pytest.mark.parametrize("interleaved,form", FORMS, ids=[f for _, f in FORMS])
def test_contraction_witnesses_keep_the_contracts_bits(interleaved, form):
    """A one-token source and table rows built from the CPU search's witnesses (rope_ref.witnesses): elements whose bf16 result
    differs between fl(fl(x1*c) - fl(x2*s)) and a fused multiply-add of either product.  Sequence 0 holds 64 witnesses of
    fma(x1, c, -fl(x2*s)), sequence 1 64 of fma(-x2, s, fl(x1*c)), sequence 2 32 of each; every head, Q and K, carries them."""
    d, half = 128, 64
    w = rr.witnesses()
    assert all(w[k][0].numel() >= 64 for k in w), {k: w[k][0].numel() for k in w}
    first, second = ([t[:64] for t in w[k]] for k in ("fma_first", "fma_second"))
    rows = [first, second, [torch.cat([a[32:64], b[32:64]]) for a, b in zip(first, second)]]
    lens = [1, CAP // 2 + 2, CAP]
    x = _source(1, d, 2100)
    cos, sin = rr.random_tables(CAP, d, 2101)
    for b, (x1, x2, c, s) in enumerate(rows):
        if interleaved:
            x[b, 0, :, 0::2], x[b, 0, :, 1::2] = x1, x2
        else:
            x[b, 0, :, :half], x[b, 0, :, half:] = x1, x2
        cos[lens[b] - 1], sin[lens[b] - 1] = c, s
    r = _run("contiguous", d, False, 1, lens, d, interleaved, 2102, x=x, tables=(cos, sin), expect=B)
    # (the whole-allocation comparison above is the check; this spells out what it covered)
    y1 = (lambda t: t[..., 0::2]) if interleaved else (lambda t: t[..., :half])
    for b, (x1, x2, c, s) in enumerate(rows):
        contract = (x1.float() * c - x2.float() * s).bfloat16()
        kb = r["K"].view(r["K"].dev).cpu()[b, :, lens[b] - 1]
        for got in (y1(r["q_out"][b, :, 0]), y1(kb)):
            assert torch.equal(got.view(torch.int16), contract.view(torch.int16).expand_as(got))


# ---- 3. drops
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_tokens_outside_the_capacity_drop_k_and_v_and_zero_their_queries(kind, d, fp8):
    # length 1: two tokens dropped, one on row 0; length capacity + 2: one on the last row; length 0: none
    r = _run(kind, d, fp8, 3, [1, CAP + 2, 0], d // 2, False, 2200 + d, expect=2)
    assert sorted((b, t) for b, t, *_ in r["written"]) == [(0, 2), (1, 0)]
    zero = (r["q_out"].view(torch.int16) == 0).all(dim=-1)                 # [B, H_q, n_new]: +0.0 throughout, bit for bit
    assert zero.tolist() == [[[True, True, False]] * HQ, [[False, True, True]] * HQ, [[True, True, True]] * HQ]
    r = _run(kind, d, fp8, 3, [-5, ar.INT_MAX, ar.INT_MIN], d, True, 2300 + d, expect=0)
    assert (r["q_out"].view(torch.int16) == 0).all()
    r = _run(kind, d, fp8, 3, [0, ar.INT_MAX - 1, ar.INT_MIN + 1], 16, False, 2400 + d, expect=0)
    assert (r["q_out"].view(torch.int16) == 0).all()


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("values", ((-1, N_PAGES), (ar.INT_MIN, ar.INT_MAX)))
def test_a_table_entry_outside_the_pool_drops_k_and_v_only(values, fp8):
    """Rows 31 | 32, 33 of every sequence: sequence 1's second page and sequence 2's first page have no valid entry.  Their
    queries are rotated all the same: Q depends on the position alone."""
    r = _run("P32", 128, fp8, 3, [34, 34, 34], 64, False, 2500, bad=((1, 1, values[0]), (2, 0, values[1])), expect=3 + 1 + 2)
    assert sorted((b, t) for b, t, *_ in r["written"]) == [(0, 0), (0, 1), (0, 2), (1, 0), (2, 1), (2, 2)]
    assert not (r["q_out"].view(torch.int16) == 0).all(dim=-1).any()
    assert torch.equal(r["q_out"].view(torch.int16), rr.rope(_views(r["x"])[0], r["cos"], r["sin"], [34, 34, 34], CAP, False).view(torch.int16))


# ---- 4. the fused call is {rotate to bf16, kv_cache_append}, on the device
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_fused_call_equals_rotated_upload_then_the_existing_append(kind, fp8):
    fa, d, n_new, rot, interleaved = _fa(), 128, 19, 64, False
    lens = [n_new, CAP // 2 + 2, CAP]
    r = _run(kind, d, fp8, n_new, lens, rot, interleaved, 2600)
    _, kn, vn = _views(r["x"])
    k_rot = rr.rope(kn, r["cos"], r["sin"], lens, CAP, interleaved).cuda()                     # the model's rotated bf16 K, uploaded
    K2, V2 = Alloc(r["K"].shape, r["K"].dtype, 2601), Alloc(r["V"].shape, r["V"].dtype, 2602)      # the same bytes as the fused call's
    assert torch.equal(K2.host, r["K"].host) and torch.equal(V2.host, r["V"].host)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    kw = dict(k_descale=torch.tensor(KD).cuda(), v_descale=torch.tensor(VD).cuda()) if fp8 else {}
    if kind == "contiguous":
        fa.kv_cache_append(k_rot, vn.contiguous().cuda(), K2.view(K2.dev), V2.view(V2.dev), lens_d, **kw)
    else:
        fa.kv_cache_append_paged(k_rot, vn.contiguous().cuda(), K2.view(K2.dev), V2.view(V2.dev), r["table"].cuda(), lens_d, **kw)
    torch.cuda.synchronize()
    assert torch.equal(K2.dev, r["K"].dev) and torch.equal(V2.dev, r["V"].dev)


# ---- 5. K/V only
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_a_call_without_queries_writes_the_caches_alone(kind, fp8):
    _run(kind, 64, fp8, 3, [3, CAP // 2 + 2, CAP], 32, True, 2700, with_q=False, expect=9)
    _run(kind, 128, fp8, 19, [19, CAP // 2 + 2, CAP], 128, False, 2710, with_q=False, expect=57)


# ---- 6. fused call then decode
def _history(kind, d, fp8, seed):
    """Caches full of history written by the framework expression (host tensors), with descales and a table."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (torch.rand(B, HKV, CAP, d, generator=g) - 0.5).bfloat16()
    kd, vd = (torch.tensor(KD) / 100, torch.tensor(VD) / 100) if fp8 else (None, None)
    K, V = (ar.quantise(mk(), ds) if fp8 else mk() for ds in (kd, vd))
    if kind == "contiguous":
        return K, V, None, kd, vd
    perm = torch.randperm(B * MAX_PAGES, generator=g).view(B, MAX_PAGES)      # a pool of B max_pages pages here: every page in use
    paged = lambda t: t.view(torch.uint8 if fp8 else torch.int16).view(B, HKV, MAX_PAGES, PAGE, d).permute(0, 2, 1, 3, 4) \
        .reshape(B * MAX_PAGES, HKV, PAGE, d)[torch.argsort(perm.flatten())].contiguous().view(t.dtype)
    return paged(K), paged(V), perm.int(), kd, vd


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_fused_call_then_decode_equals_decode_on_model_written_cache_and_queries(kind, fp8):
    fa, d, n_new, rot, interleaved = _fa(), 128, 3, 64, False
    lens = [5 + n_new, 40 + n_new, 93 + n_new]
    K, V, table, kd, vd = _history(kind, d, fp8, 2800)
    x = _source(n_new, d, 2801, scale=1.0)
    q, kn, vn = _views(x)
    cos, sin = rr.random_tables(CAP, rot, 2802)
    Kw, Vw = K.clone(), V.clone()                               # the model's write and the model's queries
    if table is None:
        q_ref, _ = rr.rope_append(q, kn, vn, Kw, Vw, cos, sin, lens, interleaved, kd, vd)
    else:
        q_ref, _ = rr.rope_append_paged(q, kn, vn, Kw, Vw, table, cos, sin, lens, interleaved, kd, vd)
    qd, knd, vnd = _views(x.cuda())
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    Kd, Vd = K.cuda(), V.cuda()
    kw = dict(k_descale=None if kd is None else kd.cuda(), v_descale=None if vd is None else vd.cuda())
    if table is None:
        Q = fa.rope_kv_cache_append(qd, knd, vnd, Kd, Vd, cos.cuda(), sin.cuda(), lens_d, interleaved=interleaved, **kw)
        got = fa.flash_attention_2_decode(Q, Kd, Vd, lens_d, **kw)
        want = fa.flash_attention_2_decode(q_ref.cuda(), Kw.cuda(), Vw.cuda(), lens_d, **kw)
    else:
        Q = fa.rope_kv_cache_append_paged(qd, knd, vnd, Kd, Vd, table.cuda(), cos.cuda(), sin.cuda(), lens_d, interleaved=interleaved, **kw)
        got = fa.flash_attention_2_decode_paged(Q, Kd, Vd, table.cuda(), lens_d, **kw)
        want = fa.flash_attention_2_decode_paged(q_ref.cuda(), Kw.cuda(), Vw.cuda(), table.cuda(), lens_d, **kw)
    torch.cuda.synchronize()
    assert Q.is_contiguous() and tuple(Q.shape) == (B, HQ, n_new, d)
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert not torch.isnan(got[0].float()).any() and torch.isfinite(got[1]).all()
    assert not torch.equal(Kd.cpu().view(torch.uint8), K.view(torch.uint8))      # (the call did write)


# ---- 7. one captured graph of fused call + decode
def test_one_captured_graph_of_fused_call_and_decode_serves_three_steps():
    """Paged e4m3, one token per step.  Captured once on one stream with a caller workspace, Q_out, O, L and a static source
    buffer; between replays the lengths are bumped, the source is overwritten and a table entry is assigned as a sequence crosses
    into a new page, all IN PLACE, and Q_out is refilled with a pattern.  Every replay leaves the pools, Q_out, O and L bit for
    bit what the same two eager calls leave on a copy."""
    fa, d, n_new, rot = _fa(), 128, 1, 64
    g = torch.Generator().manual_seed(2900)
    pools = [torch.randint(0, 0x78, (N_PAGES, HKV, PAGE, d), generator=g, dtype=torch.uint8).cuda().view(E4M3) for _ in range(2)]
    table = torch.tensor([[5, -1, -1], [2, -1, -1], [7, -1, -1]], dtype=torch.int32, device="cuda")
    lens = torch.tensor([30, 31, 5], dtype=torch.int32, device="cuda")
    kd, vd = (torch.tensor(KD) / 100).cuda(), (torch.tensor(VD) / 100).cuda()
    cos, sin = (t.cuda() for t in rr.random_tables(CAP, rot, 2901))
    x = torch.zeros(B, n_new, HQ + 2 * HKV, d, dtype=torch.bfloat16, device="cuda")
    q_view, kn, vn = _views(x)
    Q = torch.empty(B, HQ, n_new, d, dtype=torch.bfloat16, device="cuda")
    O, L = torch.empty_like(Q), torch.empty(B, HQ, n_new, dtype=torch.float32, device="cuda")
    ws = fa.decode_workspace(B, HQ, HKV, n_new, MAX_PAGES * PAGE, d, 2)
    assert ws.numel() > 0

    def step(Kp, Vp, Q, O, L, ws):
        out = fa.rope_kv_cache_append_paged(q_view, kn, vn, Kp, Vp, table, cos, sin, lens, k_descale=kd, v_descale=vd, Q_out=Q)
        assert out is Q                                             # (nothing allocated: the capture holds no allocation of the call's)
        return fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, n_splits=2, O=O, L=L, workspace=ws, k_descale=kd, v_descale=vd)

    step(*pools, Q, O, L, ws)      # (code objects load outside the capture)
    torch.cuda.synchronize()
    eager = [p.clone() for p in pools]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(*pools, Q, O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    assign = {1: (1, 1, 0), 2: (0, 1, 3)}      # before step s: sequence b's logical page p becomes pool page v
    for s in range(3):
        lens += n_new                           # 31 32 6 | 32 33 7 | 33 34 8: sequence 1 reaches row 32 at step 1, sequence 0 at step 2
        if s in assign:
            b, p, v = assign[s]
            table[b, p] = v
        x.copy_(((torch.rand(x.shape, generator=g) - 0.5) * 2).bfloat16().cuda())
        Q.view(torch.int16).fill_(0x5A5A)
        O.view(torch.int16).fill_(0x5A5A)
        L.view(torch.int32).fill_(0x5A5A5A5A)
        graph.replay()
        torch.cuda.synchronize()
        Qe = torch.empty_like(Q)
        Oe, Le = step(*eager, Qe, torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))
        torch.cuda.synchronize()
        for got, want in zip(pools, eager):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), ("pool", s)
        assert torch.equal(Q.view(torch.int16), Qe.view(torch.int16)), ("Q_out", s)
        assert torch.equal(O.view(torch.int16), Oe.view(torch.int16)) and torch.equal(L.view(torch.int32), Le.view(torch.int32)), s
        assert not torch.isnan(O.float()).any()
    # the last step's rows are the model's: sequence 0 wrote row 32 = row 0 of pool page 3, its queries sit in Q
    host_lens = lens.cpu().tolist()
    k_rot = rr.rope(kn.cpu(), cos.cpu(), sin.cpu(), host_lens, MAX_PAGES * PAGE, False)
    row = ar.quantise(k_rot, kd.cpu()).view(torch.uint8)
    assert torch.equal(pools[0].cpu().view(torch.uint8)[3, :, 0], row[0, :, 0])
    assert torch.equal(Q.cpu().view(torch.int16), rr.rope(q_view.cpu(), cos.cpu(), sin.cpu(), host_lens, MAX_PAGES * PAGE, False).view(torch.int16))
