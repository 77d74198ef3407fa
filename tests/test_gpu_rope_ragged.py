"""GPU: the ragged rotary-embedding KV-cache append (fa2_rope_kv_append_ragged, _paged through rope_kv_cache_append_ragged /
_paged and kv_cache_append_ragged / _paged), contiguous and paged, bf16 and e4m3, both pair forms, full and partial rot_dim.

H_q = 4, H_kv = 2, d in 64, 128, T = 28 packed tokens; a contiguous cache of 96 rows, or pages of 32 keys, three table entries
per sequence, in a shuffled pool of 16 pages.  The source is ONE fused [T, H_q + 2 H_kv, d] tensor whose Q, K and V slices are
passed as views.  Every cache, pool and Q_out is a VIEW between 1024-byte guard bands in an allocation of random bytes, and every
check compares the WHOLE allocation with tests/rope_ragged_ref.py applied to a host copy.  The tolerance is ZERO everywhere: the
contract is IEEE operations only (include/fa2_rope_mi355x.h, ARITHMETIC), and no source here holds a NaN.  The cos/sin tables are
rope_ref.random_tables: a distinct value per (table, position, column).  The inputs (rope_ragged_ref.PLACEMENT, DROPS, HOSTILE,
MANY) are the ones tests/test_rope_ragged_reference.py shows five wrong models to fail on."""
import pytest
import torch

import extend_ragged_ref as xr
import kv_append_ref as ar
import rope_ragged_ref as gr
import rope_ref as rr
from test_gpu_rope_append import GUARD, Alloc, _same

pytestmark = pytest.mark.gpu

HQ, HKV, CAP, PAGE, MAX_PAGES, N_PAGES, T = gr.HQ, gr.HKV, gr.CAP, gr.PAGE, gr.MAX_PAGES, gr.N_PAGES, gr.T
KINDS = ("contiguous", "P32")
E4M3 = ar.E4M3
KD, VD = (0.3, 0.7), (1.3, 0.9)                # a descale of its own per head and per tensor, none a power of two
FORMS = ((False, "half"), (True, "pairs"))
assert GUARD == 1024


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _run(kind, d, fp8, case, rot, interleaved, seed, bad=(), with_q=True, plan=None, plain=False, model_cu=None, expect=None):
    """One call against the model on the whole allocations of K, V and Q_out.  rot = 0: no tables.  plan: what to pass in place
    of cu_seqlens_q (an ExtendRaggedPlan); model_cu: the cu the model runs on (None with a wrong plan: the model is 'nothing
    changes').  plain: through kv_cache_append_ragged[_paged].  Returns what the later checks look at."""
    fa = _fa()
    cu, lens = list(case["cu"]), list(case["lens"])
    B = len(lens)
    dtype = E4M3 if fp8 else torch.bfloat16
    paged = kind != "contiguous"
    shape = (N_PAGES, HKV, PAGE, d) if paged else (B, HKV, CAP, d)
    x = gr.source(d, seed)
    q, kn, vn = gr.views(x)
    cos, sin = rr.random_tables(CAP, rot, seed + 5) if rot else (None, None)
    K, V, Qo = Alloc(shape, dtype, seed + 1), Alloc(shape, dtype, seed + 2), Alloc((T, HQ, d), torch.bfloat16, seed + 4)
    kd, vd = (torch.tensor(KD), torch.tensor(VD)) if fp8 else (None, None)
    table = gr.table_for(cu, lens, seed + 3, bad=bad) if paged else None
    # the model, on host copies
    want = [a.host.clone() for a in (K, V, Qo)]
    q_ref, written = None, None
    if model_cu != "untouched":
        q_ref, written = gr.ragged_append(q if with_q else None, kn, vn, K.view(want[0]), V.view(want[1]), table, cos, sin,
                                          cu if model_cu is None else model_cu, lens, interleaved, kd, vd)
        if with_q:
            Qo.view(want[2]).view(torch.int16).copy_(q_ref.view(torch.int16))
        if expect is not None:
            assert sum(len(w) for w in written) == expect, (written, expect)
    # the call
    xd = x.cuda()
    qd, knd, vnd = gr.views(xd)
    lens_d = _dev_i32(lens)
    how = _dev_i32(cu) if plan is None else plan
    kw = dict(k_descale=None if kd is None else kd.cuda(), v_descale=None if vd is None else vd.cuda())
    tbl = (table.cuda(),) if paged else ()
    if plain:
        f = fa.kv_cache_append_ragged_paged if paged else fa.kv_cache_append_ragged
        out = f(knd, vnd, K.view(K.dev), V.view(V.dev), *tbl, how, lens_d, **kw)
    else:
        f = fa.rope_kv_cache_append_ragged_paged if paged else fa.rope_kv_cache_append_ragged
        out = f(qd if with_q else None, knd, vnd, K.view(K.dev), V.view(V.dev), *tbl, None if cos is None else cos.cuda(),
                None if sin is None else sin.cuda(), how, lens_d, interleaved=interleaved, Q_out=Qo.view(Qo.dev) if with_q else None, **kw)
    torch.cuda.synchronize()
    assert (out.data_ptr() == Qo.view(Qo.dev).data_ptr()) if with_q and not plain else out is None
    where = (kind, d, "e4m3" if fp8 else "bf16", tuple(cu[:6]), rot, "pairs" if interleaved else "half")
    for a, w, name in zip((K, V, Qo), want, ("K", "V", "Q_out")):
        _same(a.dev, w, where + (name,))
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16)), "the source is only read"
    return dict(written=written, q_out=Qo.view(Qo.dev).cpu(), q_ref=q_ref, K=K, V=V, table=table, cos=cos, sin=sin, x=x, lens=lens, cu=cu)


def _zero_rows(q_out):
    return (q_out.view(torch.int16) == 0).all(dim=-1).all(dim=-1).tolist()      # [T]: +0.0 throughout in every head


# ---- 1. placement (and 7: bit for bit the siblings)
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_rows_land_where_the_plan_and_the_lengths_say(kind, d, fp8):
    """q = 0, 1, 19, 5 behind an un-owned token 0, tokens 26, 27 un-owned; the group of tokens 0..7 holds an un-owned token and two
    sequences.  Row 0, rows 31..49 across a page, a sequence ending on the last row."""
    for rot in (d, d // 2, 16):
        for interleaved, _ in FORMS:
            r = _run(kind, d, fp8, gr.PLACEMENT, rot, interleaved, 3000 + d + rot, expect=25)
            assert _zero_rows(r["q_out"]) == [True] + [False] * 25 + [True, True]


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_bit_for_bit_the_uniform_call_on_each_sequence_alone(kind, fp8):
    """Case 1's caches and the Q_out rows of owned tokens equal what rope_kv_cache_append / _paged writes when called on each
    sequence alone with B = 1 and n_new = q_b -- on the device, both sides the product's."""
    fa = _fa()
    for d, rot, interleaved in ((128, 64, False), (64, 64, True)):
        seed = 3100 + d
        r = _run(kind, d, fp8, gr.PLACEMENT, rot, interleaved, seed)
        K2, V2 = Alloc(r["K"].shape, r["K"].dtype, seed + 1), Alloc(r["V"].shape, r["V"].dtype, seed + 2)      # the same bytes as the ragged call's
        assert torch.equal(K2.host, r["K"].host)
        xd = r["x"].cuda()
        qd, knd, vnd = gr.views(xd)
        kw = dict(k_descale=torch.tensor(KD).cuda(), v_descale=torch.tensor(VD).cuda()) if fp8 else {}
        cu = r["cu"]
        for b in range(len(r["lens"])):
            s, n = cu[b], cu[b + 1] - cu[b]
            if not n:
                continue
            one = lambda t: t[s:s + n].permute(1, 0, 2)[None]      # [1, H, q_b, d] views of the same tokens
            lens_d = _dev_i32(r["lens"][b:b + 1])
            if kind == "contiguous":
                q1 = fa.rope_kv_cache_append(one(qd), one(knd), one(vnd), K2.view(K2.dev)[b:b + 1], V2.view(V2.dev)[b:b + 1],
                                             r["cos"].cuda(), r["sin"].cuda(), lens_d, interleaved=interleaved, **kw)
            else:
                q1 = fa.rope_kv_cache_append_paged(one(qd), one(knd), one(vnd), K2.view(K2.dev), V2.view(V2.dev), r["table"][b:b + 1].cuda(),
                                                   r["cos"].cuda(), r["sin"].cuda(), lens_d, interleaved=interleaved, **kw)
            torch.cuda.synchronize()
            assert torch.equal(q1[0].permute(1, 0, 2).cpu().view(torch.int16), r["q_out"][s:s + n].view(torch.int16)), (d, b)
        assert torch.equal(K2.dev, r["K"].dev) and torch.equal(V2.dev, r["V"].dev), d


# ---- 2. drops
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
def test_dropped_tokens_write_no_key_and_a_zero_query(kind, d, fp8):
    """lens = (5, 0, 10, 99): a negative position, nine leading tokens before row 0, positions past the capacity with 94 and 95
    written.  Dropped rows are +0.0 in Q_out; the guards and the rest of the cache are untouched (the whole-allocation check)."""
    r = _run(kind, d, fp8, gr.DROPS, d // 2, False, 3200 + d, expect=10 + 2)
    assert _zero_rows(r["q_out"]) == [True, True] + [True] * 9 + [False] * 10 + [False, False, True, True, True] + [True, True]
    r = _run(kind, d, fp8, dict(cu=gr.DROPS["cu"], lens=(ar.INT_MIN, ar.INT_MAX, ar.INT_MIN + 1, ar.INT_MAX - 1)), d, True, 3250 + d, expect=0)
    assert all(_zero_rows(r["q_out"]))


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("values", ((-1, N_PAGES), (ar.INT_MIN, ar.INT_MAX)))
def test_a_table_entry_outside_the_pool_drops_k_and_v_only(values, fp8):
    """PLACEMENT with sequence 2's second page (rows 32..49) and sequence 3's third page (rows 91..95) behind bad entries: those
    tokens' K and V are dropped, their queries are rotated all the same."""
    r = _run("P32", 128, fp8, gr.PLACEMENT, 64, False, 3300, bad=((2, 1, values[0]), (3, 2, values[1])), expect=1 + 1)
    assert _zero_rows(r["q_out"]) == [True] + [False] * 25 + [True, True]


# ---- 3. a hostile cu goes through the plan kernel
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_a_hostile_cu_is_the_model_on_the_sanitised_pairs(kind, fp8):
    assert xr.sanitised(gr.HOSTILE["cu"], T) == [(5, 0), (5, 23), (28, 0), (28, 0)]
    for d in (64, 128):
        r = _run(kind, d, fp8, gr.HOSTILE, d, False, 3400 + d, expect=23)
        assert _zero_rows(r["q_out"]) == [True] * 5 + [False] * 23


# ---- 4. a wrong plan: no byte of any allocation changes
@pytest.mark.parametrize("with_q", (True, False), ids=("q", "kv-only"))
@pytest.mark.parametrize("kind", KINDS)
def test_a_plan_for_another_batch_changes_nothing(kind, with_q):
    fa = _fa()
    cu = list(gr.PLACEMENT["cu"])
    G = HQ // HKV
    good = fa.extend_ragged_plan(_dev_i32(cu), HQ, HKV, T)
    other_B = fa.extend_ragged_plan(_dev_i32(cu[:4]), HQ, HKV, T)            # built for B = 3
    other_T = fa.extend_ragged_plan(_dev_i32(cu), HQ, HKV, T - 1)            # built for T = 27
    other_G = fa.extend_ragged_plan(_dev_i32(cu), HKV, HKV, T)               # built for G = 1
    torch.cuda.synchronize()
    size = good.tensor.numel()
    wrong = [fa.ExtendRaggedPlan(torch.cat([p.tensor, torch.zeros(size, dtype=torch.int32, device="cuda")])[:size].contiguous(), len(cu) - 1,
                                 HQ, HKV, T) for p in (other_B, other_T)]
    wrong.append(fa.ExtendRaggedPlan(torch.zeros(size, dtype=torch.int32, device="cuda"), len(cu) - 1, HQ, HKV, T))      # never built
    if with_q:
        wrong.append(fa.ExtendRaggedPlan(other_G.tensor, len(cu) - 1, HQ, HKV, T))
    for i, plan in enumerate(wrong):
        assert plan.tensor.data_ptr() % 16 == 0
        for fp8 in (False, True):
            _run(kind, 128, fp8, gr.PLACEMENT, 64, False, 3500 + i, with_q=with_q, plan=plan, model_cu="untouched")
    # (the same call with the right plan does write; a K/V-only call takes a plan built for any G)
    _run(kind, 128, False, gr.PLACEMENT, 64, False, 3550, with_q=with_q, plan=good, expect=25)
    if not with_q:
        _run(kind, 128, False, gr.PLACEMENT, 64, False, 3551, with_q=False, plan=fa.ExtendRaggedPlan(other_G.tensor, len(cu) - 1, HKV, HKV, T), expect=25)


# ---- 5. many sequences: six search steps, runs of equal starts
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_thirty_seven_sequences_mostly_empty(kind, fp8):
    for d in (64, 128):
        r = _run(kind, d, fp8, gr.MANY, d // 2, True, 3600 + d, expect=23)
        assert _zero_rows(r["q_out"]) == [True, True] + [False] * 23 + [True] * 3


# ---- 6. the plain ragged append
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_the_plain_ragged_append_is_kv_cache_append_per_sequence(kind, fp8):
    fa = _fa()
    for d, case, n in ((64, gr.PLACEMENT, 25), (128, gr.DROPS, 12)):
        seed = 3700 + d
        r = _run(kind, d, fp8, case, 0, False, seed, with_q=False, plain=True, expect=n)
        K2, V2 = Alloc(r["K"].shape, r["K"].dtype, seed + 1), Alloc(r["V"].shape, r["V"].dtype, seed + 2)
        _, knd, vnd = gr.views(r["x"].cuda())
        kw = dict(k_descale=torch.tensor(KD).cuda(), v_descale=torch.tensor(VD).cuda()) if fp8 else {}
        cu = r["cu"]
        for b in range(len(r["lens"])):
            s, q = cu[b], cu[b + 1] - cu[b]
            if not q:
                continue
            one = lambda t: t[s:s + q].permute(1, 0, 2)[None]
            if kind == "contiguous":
                fa.kv_cache_append(one(knd), one(vnd), K2.view(K2.dev)[b:b + 1], V2.view(V2.dev)[b:b + 1], _dev_i32(r["lens"][b:b + 1]), **kw)
            else:
                fa.kv_cache_append_paged(one(knd), one(vnd), K2.view(K2.dev), V2.view(V2.dev), r["table"][b:b + 1].cuda(),
                                         _dev_i32(r["lens"][b:b + 1]), **kw)
        torch.cuda.synchronize()
        assert torch.equal(K2.dev, r["K"].dev) and torch.equal(V2.dev, r["V"].dev), d
    # rot_dim = 0 WITH queries: Q_out holds the source bits of owned tokens with a row
    r = _run(kind, 128, fp8, gr.DROPS, 0, False, 3750, expect=12)
    q = gr.views(r["x"])[0]
    assert torch.equal(r["q_out"][11:23].view(torch.int16), q[11:23].view(torch.int16))


# ---- 8. the step in one captured graph
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_one_captured_graph_of_plan_append_and_attention_serves_three_steps(fp8):
    """{extend_ragged_plan, rope_kv_cache_append_ragged_paged, flash_attention_2_extend_ragged_paged}, captured once on a side
    stream with caller buffers; between replays cu, seqlens_k, the source and the table are rewritten IN PLACE.  Every replay
    leaves the pools, Q_out, O and L bit for bit what the same eager calls leave on a copy, and O and L of every owned token bit
    for bit what the per-sequence route gives: uniform rope_kv_cache_append_paged, then uniform flash_attention_2_extend_paged."""
    fa, d, rot, B, n_splits = _fa(), 128, 64, 4, 2
    g = torch.Generator().manual_seed(3800)
    if fp8:
        pools = [torch.randint(0, 0x78, (N_PAGES, HKV, PAGE, d), generator=g, dtype=torch.uint8).cuda().view(E4M3) for _ in range(2)]
        kw = dict(k_descale=(torch.tensor(KD) / 100).cuda(), v_descale=(torch.tensor(VD) / 100).cuda())
    else:
        pools = [((torch.rand(N_PAGES, HKV, PAGE, d, generator=g) - 0.5)).bfloat16().cuda() for _ in range(2)]
        kw = {}
    cos, sin = (t.cuda() for t in rr.random_tables(CAP, rot, 3801))
    # every sequence owns its three pages from the start except where a step assigns one
    steps = [dict(cu=(0, 1, 9, 9, 28), lens=(32, 40, 7, 19)),           # q = 1 8 0 19; sequence 3's first 19 tokens
             dict(cu=(2, 3, 4, 20, 25), lens=(33, 41, 23, 24)),         # q = 1 1 16 5 behind two un-owned tokens, three after
             dict(cu=(0, 0, 1, 2, 3), lens=(33, 42, 24, 25))]           # q = 0 1 1 1: a decode step, tokens 3..27 un-owned
    table = torch.tensor([[5, -1, -1], [2, 9, -1], [7, -1, -1], [11, -1, -1]], dtype=torch.int32, device="cuda")
    assign = {1: (0, 1, 3)}      # before step s: sequence b's logical page p becomes pool page v (sequence 0 writes row 32 at step 1)
    cu_d, lens_d = _dev_i32(steps[0]["cu"]), _dev_i32(steps[0]["lens"])
    x = torch.zeros(T, HQ + 2 * HKV, d, dtype=torch.bfloat16, device="cuda")
    q_view, kn, vn = gr.views(x)
    plan = fa.extend_ragged_plan(cu_d, HQ, HKV, T)
    Q = torch.empty(T, HQ, d, dtype=torch.bfloat16, device="cuda")
    O, L = torch.empty_like(Q), torch.empty(T, HQ, dtype=torch.float32, device="cuda")
    ws = fa.extend_ragged_workspace(B, HQ, HKV, T, MAX_PAGES * PAGE, d, n_splits)
    assert ws.numel() > 0

    def step(Kp, Vp, Q, O, L, ws):
        p = fa.extend_ragged_plan(cu_d, HQ, HKV, T, plan=plan)
        out = fa.rope_kv_cache_append_ragged_paged(q_view, kn, vn, Kp, Vp, table, cos, sin, p, lens_d, Q_out=Q, **kw)
        assert out is Q and p.tensor is plan.tensor                 # (nothing allocated: the capture holds no allocation of the calls')
        return fa.flash_attention_2_extend_ragged_paged(Q, Kp, Vp, table, p, lens_d, n_splits=n_splits, O=O, L=L, workspace=ws, **kw)

    x.copy_(((torch.rand(x.shape, generator=g) - 0.5) * 2).bfloat16().cuda())
    warm = [p.clone() for p in pools]
    step(*warm, Q, O, L, ws)      # (code objects load outside the capture)
    torch.cuda.synchronize()
    eager = [p.clone() for p in pools]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(*pools, Q, O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    for s, st in enumerate(steps):
        cu_d.copy_(_dev_i32(st["cu"]))
        lens_d.copy_(_dev_i32(st["lens"]))
        if s in assign:
            b, p, v = assign[s]
            table[b, p] = v
        x.copy_(((torch.rand(x.shape, generator=g) - 0.5) * 2).bfloat16().cuda())
        x_before = x.clone()
        Q.view(torch.int16).fill_(0x5A5A)
        O.view(torch.int16).fill_(0x5A5A)
        L.view(torch.int32).fill_(0x5A5A5A5A)
        graph.replay()
        torch.cuda.synchronize()
        Qe, Oe, Le = torch.empty_like(Q), torch.empty_like(O), torch.empty_like(L)
        for t_ in (Qe.view(torch.int16), Oe.view(torch.int16)):
            t_.fill_(0x5A5A)
        Le.view(torch.int32).fill_(0x5A5A5A5A)
        route = [p.clone() for p in eager]                           # the per-sequence route starts from the pools before the step
        step(*eager, Qe, Oe, Le, torch.empty_like(ws))
        torch.cuda.synchronize()
        for got, want in zip(pools, eager):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), ("pool", s)
        assert torch.equal(Q.view(torch.int16), Qe.view(torch.int16)), ("Q_out", s)
        assert torch.equal(O.view(torch.int16), Oe.view(torch.int16)) and torch.equal(L.view(torch.int32), Le.view(torch.int32)), s
        assert torch.equal(x.view(torch.int16), x_before.view(torch.int16)), "the source is only read"
        # the per-sequence route: uniform append, then uniform extend, on each sequence alone
        owned = 0
        for b, (s0, n) in enumerate(xr.sanitised(st["cu"], T)):
            if not n:
                continue
            one = lambda t: t[s0:s0 + n].permute(1, 0, 2)[None]
            tb, lb = table[b:b + 1].contiguous(), _dev_i32(st["lens"][b:b + 1])
            q1 = fa.rope_kv_cache_append_paged(one(q_view), one(kn), one(vn), *route, tb, cos, sin, lb, **kw)
            O1, L1 = fa.flash_attention_2_extend_paged(q1, *route, tb, lb, n_splits=n_splits, **kw)
            torch.cuda.synchronize()
            assert torch.equal(O1[0].permute(1, 0, 2).contiguous().view(torch.int16), O[s0:s0 + n].view(torch.int16)), ("O", s, b)
            assert torch.equal(L1[0].permute(1, 0).contiguous().view(torch.int32), L[s0:s0 + n].view(torch.int32)), ("L", s, b)
            owned += n
        assert owned == sum(q for _, q in xr.sanitised(st["cu"], T)) > 0
        for got, want in zip(pools, route):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), ("pool against the per-sequence route", s)
        assert not torch.isnan(O[st["cu"][0]:max(st["cu"])].float()).any()
