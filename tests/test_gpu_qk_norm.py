"""GPU: the ragged rotary-embedding KV-cache append with a per-head QK RMSNorm in front of the rotation
(fa2_norm_rope_kv_append_ragged, _paged through norm_rope_kv_cache_append_ragged / _paged), contiguous and paged, bf16 and e4m3,
both pair forms, rot_dim = d, d / 2 and 0.

The sibling's fixtures (tests/test_gpu_rope_ragged.py): H_q = 4, H_kv = 2, d in 64, 128, T = 28 packed tokens; a contiguous cache
of 96 rows, or pages of 32 keys, three table entries per sequence, in a shuffled pool of 16 pages; ONE fused
[T, H_q + 2 H_kv, d] source whose Q, K and V slices are passed as views; every cache, pool and Q_out a VIEW between 1024-byte
guard bands in an allocation of random bytes, and every check compares the WHOLE allocation with tests/qk_norm_ref.py applied to
a host copy.  THE TOLERANCE IS ZERO everywhere: the contract is IEEE fp32 operations in a fixed order
(include/fa2_rope_norm_mi355x.h, ARITHMETIC), and no source here holds a NaN.  The source holds one all-zero token
(qk_norm_ref.ZERO_TOKEN): r = 1 / sqrt(eps) there and the signed zeros follow the signs of x and of the weights, as in the model.
The weights are qk_norm_ref.weights: a distinct magnitude per (tensor, column), a few negative.  eps is qk_norm_ref.EPS = 0.05,
large enough that an eps left out or added elsewhere changes most elements; the K/V-only case runs at 1e-6.  The inputs are the
ones tests/test_qk_norm_reference.py shows eight wrong models to fail on."""
import pytest
import torch

import extend_ragged_ref as xr
import kv_append_ref as ar
import qk_norm_ref as qk
import rope_ragged_ref as gr
import rope_ref as rr
from test_gpu_rope_append import GUARD, Alloc, _same

pytestmark = pytest.mark.gpu

HQ, HKV, CAP, PAGE, MAX_PAGES, N_PAGES, T = gr.HQ, gr.HKV, gr.CAP, gr.PAGE, gr.MAX_PAGES, gr.N_PAGES, gr.T
KINDS = ("contiguous", "P32")
E4M3 = ar.E4M3
KD, VD = (0.3, 0.7), (1.3, 0.9)                # a descale of its own per head and per tensor, none a power of two
FORMS = ((False, "half"), (True, "pairs"))
SEED = 4000                                    # tests/test_qk_norm_reference.py certifies its mutants on these seeds
assert GUARD == 1024


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _run(kind, d, fp8, case, rot, interleaved, seed, with_q=True, plan=None, untouched=False, x=None, eps=qk.EPS, expect=None, bad=()):
    """One call against the model on the whole allocations of K, V and Q_out.  rot = 0: no tables.  plan: what to pass in place
    of cu_seqlens_q (an ExtendRaggedPlan); untouched: the model is 'nothing changes' (a plan for another batch).  x: the fused
    source (qk_norm_ref.source(d, seed) by default).  Returns what the later checks look at."""
    fa = _fa()
    cu, lens = list(case["cu"]), list(case["lens"])
    B = len(lens)
    dtype = E4M3 if fp8 else torch.bfloat16
    paged = kind != "contiguous"
    shape = (N_PAGES, HKV, PAGE, d) if paged else (B, HKV, CAP, d)
    x = qk.source(d, seed) if x is None else x
    q, kn, vn = gr.views(x)
    qw, kw = qk.weights(d, qk.WEIGHT_SEED)
    cos, sin = rr.random_tables(CAP, rot, seed + 5) if rot else (None, None)
    K, V, Qo = Alloc(shape, dtype, seed + 1), Alloc(shape, dtype, seed + 2), Alloc((T, HQ, d), torch.bfloat16, seed + 4)
    kd, vd = (torch.tensor(KD), torch.tensor(VD)) if fp8 else (None, None)
    table = gr.table_for(cu, lens, seed + 3, bad=bad) if paged else None
    # the model, on host copies
    want = [a.host.clone() for a in (K, V, Qo)]
    q_ref, written = None, None
    if not untouched:
        q_ref, written = qk.ragged_append(q if with_q else None, kn, vn, K.view(want[0]), V.view(want[1]), table, cos, sin,
                                          qw if with_q else None, kw, eps, cu, lens, interleaved, kd, vd)
        if with_q:
            Qo.view(want[2]).view(torch.int16).copy_(q_ref.view(torch.int16))
        if expect is not None:
            assert sum(len(w) for w in written) == expect, (written, expect)
    # the call
    xd = x.cuda()
    qd, knd, vnd = gr.views(xd)
    lens_d = _dev_i32(lens)
    how = _dev_i32(cu) if plan is None else plan
    kw_args = dict(k_descale=None if kd is None else kd.cuda(), v_descale=None if vd is None else vd.cuda())
    tbl = (table.cuda(),) if paged else ()
    f = fa.norm_rope_kv_cache_append_ragged_paged if paged else fa.norm_rope_kv_cache_append_ragged
    out = f(qd if with_q else None, knd, vnd, K.view(K.dev), V.view(V.dev), *tbl, None if cos is None else cos.cuda(),
            None if sin is None else sin.cuda(), qw.cuda() if with_q else None, kw.cuda(), eps, how, lens_d, interleaved=interleaved,
            Q_out=Qo.view(Qo.dev) if with_q else None, **kw_args)
    torch.cuda.synchronize()
    assert (out.data_ptr() == Qo.view(Qo.dev).data_ptr()) if with_q else out is None
    where = (kind, d, "e4m3" if fp8 else "bf16", tuple(cu[:6]), rot, "pairs" if interleaved else "half")
    for a, w, name in zip((K, V, Qo), want, ("K", "V", "Q_out")):
        _same(a.dev, w, where + (name,))
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16)), "the source is only read"
    return dict(written=written, q_out=Qo.view(Qo.dev).cpu(), q_ref=q_ref, K=K, V=V, Qo=Qo, table=table, cos=cos, sin=sin, x=x, lens=lens,
                cu=cu, qw=qw, kw=kw)


def _zero_rows(q_out):
    return (q_out.view(torch.int16) == 0).all(dim=-1).all(dim=-1).tolist()      # [T]: +0.0 throughout in every head


# ---- 1. against the model
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ("PLACEMENT", "DROPS"))
def test_the_call_is_the_model_byte_for_byte(case, kind, d, fp8):
    """PLACEMENT: q = 0, 1, 19, 5 behind an un-owned token 0, tokens 26, 27 un-owned; row 0, rows 31..49 across a page, a
    sequence ending on the last row; token 5 all zeros.  DROPS: a negative position, nine leading tokens before row 0, positions
    past the capacity.  Both pair forms at rot_dim = d, d / 2 and 0 (no rotation: the normalised row itself is stored)."""
    for rot in (d, d // 2, 0):
        for interleaved, _ in FORMS:
            if case == "PLACEMENT":
                r = _run(kind, d, fp8, gr.PLACEMENT, rot, interleaved, SEED + d + rot, expect=25)
                assert _zero_rows(r["q_out"]) == [True] + [False] * 25 + [True, True]
                # the all-zero token: zeros of both signs in Q_out, by the signs of x and w where nothing rotates them
                zero = r["q_out"][qk.ZERO_TOKEN].view(torch.int16)
                assert set(zero.flatten().tolist()) <= {0, -0x8000}
                if rot == 0:
                    assert set(zero.flatten().tolist()) == {0, -0x8000}
                    sign = (gr.views(r["x"])[0][qk.ZERO_TOKEN].view(torch.int16) < 0) ^ (r["qw"] < 0)[None, :]
                    assert torch.equal(zero < 0, sign)
            else:
                r = _run(kind, d, fp8, gr.DROPS, rot, interleaved, SEED + 50 + d + rot, expect=10 + 2)
                assert _zero_rows(r["q_out"]) == [True, True] + [True] * 9 + [False] * 10 + [False, False, True, True, True] + [True, True]


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_a_table_entry_outside_the_pool_drops_k_and_v_only(fp8):
    r = _run("P32", 128, fp8, gr.PLACEMENT, 64, False, SEED + 90, bad=((2, 1, -1), (3, 2, N_PAGES)), expect=1 + 1)
    assert _zero_rows(r["q_out"]) == [True] + [False] * 25 + [True, True]


# ---- 2. composition: the sibling fed the normalised bf16 source, both sides on the device
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_it_is_the_sibling_applied_to_the_normalised_tensors(kind, fp8):
    fa = _fa()
    for d, rot, interleaved in ((128, 64, False), (64, 64, True), (64, 0, False)):
        seed = SEED + 100 + d + rot
        r = _run(kind, d, fp8, gr.PLACEMENT, rot, interleaved, seed)
        K2, V2, Q2 = Alloc(r["K"].shape, r["K"].dtype, seed + 1), Alloc(r["V"].shape, r["V"].dtype, seed + 2), Alloc((T, HQ, d), torch.bfloat16, seed + 4)
        assert torch.equal(K2.host, r["K"].host)      # the same bytes as the fused call's before it ran
        q, kn, vn = gr.views(r["x"])
        xn = torch.cat([qk.rms_rows(q, r["qw"], qk.EPS), qk.rms_rows(kn, r["kw"], qk.EPS), vn], dim=1).cuda()      # the model-normalised source
        qd, knd, vnd = gr.views(xn)
        kw = dict(k_descale=torch.tensor(KD).cuda(), v_descale=torch.tensor(VD).cuda()) if fp8 else {}
        tbl = (r["table"].cuda(),) if kind != "contiguous" else ()
        f = fa.rope_kv_cache_append_ragged_paged if tbl else fa.rope_kv_cache_append_ragged
        f(qd, knd, vnd, K2.view(K2.dev), V2.view(V2.dev), *tbl, None if rot == 0 else r["cos"].cuda(), None if rot == 0 else r["sin"].cuda(),
          _dev_i32(r["cu"]), _dev_i32(r["lens"]), interleaved=interleaved, Q_out=Q2.view(Q2.dev), **kw)
        torch.cuda.synchronize()
        assert torch.equal(K2.dev, r["K"].dev) and torch.equal(V2.dev, r["V"].dev) and torch.equal(Q2.dev, r["Qo"].dev), (d, rot)


# ---- 3. the witness rows of the CPU search
@pytest.mark.parametrize("d", (64, 128))
def test_rows_that_tell_the_contract_from_other_evaluations(d):
    """Every Q row and every K row of the source is a row found by qk_norm_ref.witnesses: its bf16 result differs between the
    contract and a sequential sum of the squares, a scale without the rounding of x * r, or the weight applied before r.  One
    sequence owns all 28 tokens; without a rotation Q_out and the bf16 cache hold the normalised rows themselves."""
    x = qk.witness_source(d, SEED + 300 + d)
    for kind in KINDS:
        r = _run(kind, d, False, qk.WITNESS_CASE, 0, False, SEED + 300 + d, x=x, expect=T)
        assert not any(_zero_rows(r["q_out"]))
        n = qk.rms_rows(gr.views(x)[0], r["qw"], qk.EPS)
        assert torch.equal(r["q_out"].view(torch.int16), n.view(torch.int16))
        for form in qk.WITNESS_FORMS:
            other = qk.rms_rows(gr.views(x)[0], r["qw"], qk.EPS, form=form)
            assert (r["q_out"].view(torch.int16) != other.view(torch.int16)).any(dim=-1).sum() >= 5, form
    _run("contiguous", d, True, qk.WITNESS_CASE, d, False, SEED + 310 + d, x=x, expect=T)
    _run("P32", d, False, qk.WITNESS_CASE, d // 2, True, SEED + 320 + d, x=x, expect=T)


# ---- 4. a hostile cu, and many sequences
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_a_hostile_cu_and_thirty_seven_sequences(kind, fp8):
    assert xr.sanitised(gr.HOSTILE["cu"], T) == [(5, 0), (5, 23), (28, 0), (28, 0)] and len(gr.MANY["lens"]) == 37
    for d in (64, 128):
        r = _run(kind, d, fp8, gr.HOSTILE, d, False, SEED + 400 + d, expect=23)
        assert _zero_rows(r["q_out"]) == [True] * 5 + [False] * 23
        r = _run(kind, d, fp8, gr.MANY, d // 2, True, SEED + 450 + d, expect=23)
        assert _zero_rows(r["q_out"]) == [True, True] + [False] * 23 + [True] * 3


# ---- 5. a wrong plan: no byte of any allocation changes
@pytest.mark.parametrize("with_q", (True, False), ids=("q", "kv-only"))
@pytest.mark.parametrize("kind", KINDS)
def test_a_plan_for_another_batch_changes_nothing(kind, with_q):
    fa = _fa()
    cu = list(gr.PLACEMENT["cu"])
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
            _run(kind, 128, fp8, gr.PLACEMENT, 64, False, SEED + 500 + i, with_q=with_q, plan=plan, untouched=True)
    # (the same call with the right plan does write)
    _run(kind, 128, False, gr.PLACEMENT, 64, False, SEED + 550, with_q=with_q, plan=good, expect=25)


# ---- 6. K/V only: H_q = 0, q_weight = None
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("kind", KINDS)
def test_without_queries_k_is_normalised_and_v_copied(kind, fp8):
    """At eps = 1e-6, a checkpoint's value.  V's allocation equals the plain ragged append's."""
    fa = _fa()
    for d, rot, interleaved in ((64, 32, False), (128, 0, False), (128, 128, True)):
        seed = SEED + 600 + d + rot
        r = _run(kind, d, fp8, gr.PLACEMENT, rot, interleaved, seed, with_q=False, eps=1e-6, expect=25)
        K2, V2 = Alloc(r["K"].shape, r["K"].dtype, seed + 1), Alloc(r["V"].shape, r["V"].dtype, seed + 2)
        _, knd, vnd = gr.views(r["x"].cuda())
        kw = dict(k_descale=torch.tensor(KD).cuda(), v_descale=torch.tensor(VD).cuda()) if fp8 else {}
        tbl = (r["table"].cuda(),) if kind != "contiguous" else ()
        f = fa.kv_cache_append_ragged_paged if tbl else fa.kv_cache_append_ragged
        f(knd, vnd, K2.view(K2.dev), V2.view(V2.dev), *tbl, _dev_i32(r["cu"]), _dev_i32(r["lens"]), **kw)
        torch.cuda.synchronize()
        assert torch.equal(V2.dev, r["V"].dev) and not torch.equal(K2.dev, r["K"].dev), d


# ---- 7. the step in one captured graph
@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
def test_one_captured_graph_of_plan_norm_append_and_attention_serves_two_steps(fp8):
    """{extend_ragged_plan, norm_rope_kv_cache_append_ragged_paged, flash_attention_2_extend_ragged_paged}, captured once on a side
    stream with caller buffers; between replays cu, seqlens_k, the source and the table are rewritten IN PLACE.  Every replay
    leaves the pools, Q_out, O and L bit for bit what the same eager calls leave on a copy."""
    fa, d, rot, B, n_splits = _fa(), 128, 64, 4, 2
    g = torch.Generator().manual_seed(SEED + 700)
    if fp8:
        pools = [torch.randint(0, 0x78, (N_PAGES, HKV, PAGE, d), generator=g, dtype=torch.uint8).cuda().view(E4M3) for _ in range(2)]
        kw = dict(k_descale=(torch.tensor(KD) / 100).cuda(), v_descale=(torch.tensor(VD) / 100).cuda())
    else:
        pools = [((torch.rand(N_PAGES, HKV, PAGE, d, generator=g) - 0.5)).bfloat16().cuda() for _ in range(2)]
        kw = {}
    cos, sin = (t.cuda() for t in rr.random_tables(CAP, rot, SEED + 701))
    qw, kwt = (t.cuda() for t in qk.weights(d, qk.WEIGHT_SEED))
    steps = [dict(cu=(0, 1, 9, 9, 28), lens=(32, 40, 7, 19)),           # q = 1 8 0 19
             dict(cu=(2, 3, 4, 20, 25), lens=(33, 41, 23, 24))]         # q = 1 1 16 5 behind two un-owned tokens, three after
    table = torch.tensor([[5, -1, -1], [2, 9, -1], [7, -1, -1], [11, -1, -1]], dtype=torch.int32, device="cuda")
    assign = {1: (0, 1, 3)}      # before step s: sequence b's logical page p becomes pool page v (sequence 0 writes row 32 at step 1)
    cu_d, lens_d = _dev_i32(steps[0]["cu"]), _dev_i32(steps[0]["lens"])
    x = torch.zeros(T, HQ + 2 * HKV, d, dtype=torch.bfloat16, device="cuda")
    q_view, kn, vn = gr.views(x)
    plan = fa.extend_ragged_plan(cu_d, HQ, HKV, T)
    Q = torch.empty(T, HQ, d, dtype=torch.bfloat16, device="cuda")
    O, L = torch.empty_like(Q), torch.empty(T, HQ, dtype=torch.float32, device="cuda")
    ws = fa.extend_ragged_workspace(B, HQ, HKV, T, MAX_PAGES * PAGE, d, n_splits)

    def step(Kp, Vp, Q, O, L, ws):
        p = fa.extend_ragged_plan(cu_d, HQ, HKV, T, plan=plan)
        out = fa.norm_rope_kv_cache_append_ragged_paged(q_view, kn, vn, Kp, Vp, table, cos, sin, qw, kwt, qk.EPS, p, lens_d, Q_out=Q, **kw)
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
        before = [p.clone() for p in eager]
        step(*eager, Qe, Oe, Le, torch.empty_like(ws))
        torch.cuda.synchronize()
        for got, want, was in zip(pools, eager, before):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), ("pool", s)
            assert not torch.equal(want.view(torch.uint8), was.view(torch.uint8)), ("the step wrote the pool", s)
        assert torch.equal(Q.view(torch.int16), Qe.view(torch.int16)), ("Q_out", s)
        assert torch.equal(O.view(torch.int16), Oe.view(torch.int16)) and torch.equal(L.view(torch.int32), Le.view(torch.int32)), s
        assert torch.equal(x.view(torch.int16), x_before.view(torch.int16)), "the source is only read"
        # Q_out of the owned tokens is the model's: normalised, then rotated at the token's position
        qn = qk.rms_rows(q_view.cpu(), qw.cpu(), qk.EPS)
        for b, (s0, n) in enumerate(xr.sanitised(st["cu"], T)):
            for i in range(n):
                pos = st["lens"][b] - n + i
                want = rr.rotate_bf16(qn[s0 + i], cos[pos].cpu(), sin[pos].cpu(), False)
                assert torch.equal(Q[s0 + i].cpu().view(torch.int16), want.view(torch.int16)), (s, b, i)
        assert not torch.isnan(O[st["cu"][0]:max(st["cu"])].float()).any()
