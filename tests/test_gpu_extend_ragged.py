"""GPU: ragged extend attention (fa2_forward_extend_ragged, _paged through flash_attention_2_extend_ragged / _paged): a q_len per
sequence and token-major rows against bf16 and e4m3 caches, contiguous and paged.

Cases, inputs, the float64 reference and the plan's model are tests/extend_ragged_ref.py's (tests/test_extend_ragged_reference.py
certifies them on the CPU): mixed, mqa, g1, decode and nolens at d = 64 and 128, n_splits in {0, 1, 2, 7, 64}, the causal mask, no
mask, the causal mask under each window, with and without a sink, pages of 32 and 96 keys with shared pages.
Gates: decode_ref.within_gates against the float64 reference (5e-3 on O rel-L2, 1e-4 / 1e-3 on |dL|, the -inf rows exactly the
reference's with O exactly 0), over every row of a batch at once; PER ROW |O_i - O_ref,i| <= KAPPA u sqrt(sum_j P_ij^2 |v_j|^2) +
u |O_i| (tests/decode_rows_ref.py; the worst ratio is printed with its place; the merge of two bf16 partial results gets their
roundings on top); and bit equalities without a tolerance."""
import functools

import pytest
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import decode_ref as dr
import decode_rows_ref as rows
import extend_ragged_ref as rr

pytestmark = pytest.mark.gpu

SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A      # bf16 / fp32 1.5e16: nothing these inputs produce
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _cuda(ts):
    return tuple(t.cuda() if isinstance(t, torch.Tensor) else t for t in ts)


@functools.lru_cache(maxsize=2)
def _dev(i, fp8):
    """(Q, K, V, k_descale, v_descale, scale, lens or None, sink, cu) on the device; the descales are None beside bf16 caches."""
    if fp8:
        Q, K, V, kd, vd, scale, lens, sink, cu = _cuda(rr.inputs_fp8(i))
    else:
        Q, K, V, scale, lens, sink, cu = _cuda(rr.inputs(i))
        kd = vd = None
    return Q, K, V, kd, vd, scale, lens if rr.CASES[i]["seqlens"] else None, sink, cu


@functools.lru_cache(maxsize=4)
def _pages(i, P, fp8):
    Kp, Vp, table, cap = rr.paged_inputs(i, P, fp8)
    return Kp.cuda(), Vp.cuda(), table.cuda(), cap


@functools.lru_cache(maxsize=2)
def _plan(i):
    c = rr.CASES[i]
    return _fa().extend_ragged_plan(_dev(i, False)[8], c["hq"], c["hkv"], rr.total_q(c))


def _gather(pool, table, lens, P):
    return fr.gather(pool, table, lens, P) if pool.dtype == fr.E4M3 else pr.gather(pool, table, lens, P)


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _check(where, O, L, ref, extra=None, cu=None):
    O = O.float().cpu().numpy()
    e = dr.errors(O, L.cpu().numpy(), ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    rows.check(where, O, ref, extra=extra, cu=cu)      # (cu: the place as (sequence, head, token), else as (token, head))


def _kw(i, k, fp8):
    _, _, _, kd, vd, scale, lens, sink, _ = _dev(i, fp8)
    mask, w = rr.VARIANTS[k]
    return dict(seqlens_k=lens, softmax_scale=scale, causal=mask == "causal", sink=sink if rr.has_sink(i, k) else None, k_descale=kd,
                v_descale=vd, window_left=w)


def _contiguous(i, k, fp8, n_splits, K=None, V=None, Q=None, plan=None, **kw):
    Q0, K0, V0 = _dev(i, fp8)[:3]
    return _fa().flash_attention_2_extend_ragged(Q0 if Q is None else Q, K0 if K is None else K, V0 if V is None else V,
                                                 _plan(i) if plan is None else plan, n_splits=n_splits, **dict(_kw(i, k, fp8), **kw))


def _paged(i, k, fp8, P, n_splits, pools=None, Q=None, plan=None, **kw):
    Kp, Vp, table = pools if pools is not None else _pages(i, P, fp8)[:3]
    return _fa().flash_attention_2_extend_ragged_paged(_dev(i, fp8)[0] if Q is None else Q, Kp, Vp, table, _plan(i) if plan is None else plan,
                                                       n_splits=n_splits, **dict(_kw(i, k, fp8), **kw))


# ---- 1. against the float64 reference, on all four cache kinds
@pytest.mark.parametrize("i,k", rr.RUNS, ids=rr.RUN_IDS)
def test_parity_with_the_reference(i, k):
    c = rr.CASES[i]
    for fp8 in (False, True):
        ref = rr.reference(i, k, fp8)
        for n_splits in c["splits"]:
            where = f"{rr.RUN_IDS[rr.RUNS.index((i, k))]} {'e4m3' if fp8 else 'bf16'} splits {n_splits}"
            _check(where, *_contiguous(i, k, fp8, n_splits), ref, cu=rr.cu_of(c["qs"]))
            if c["seqlens"]:      # (seqlens_k = None behind pages has the pages' capacity: test 2 ties it to the contiguous call)
                for P in rr.PAGE_SIZES:
                    _check(f"{where} page {P}", *_paged(i, k, fp8, P, n_splits), ref, cu=rr.cu_of(c["qs"]))


# ---- 2. bit identity: a sequence's rows are the uniform call's on that sequence alone; n_splits = 0; paged with contiguous
def _rows_of(OL, cu, b):
    """Sequence b's rows of a token-major (O, L) as the uniform call lays them out: [1, hq, q_b, d] and [1, hq, q_b]."""
    O, L = OL
    return O[cu[b]:cu[b + 1]].transpose(0, 1)[None].contiguous(), L[cu[b]:cu[b + 1]].transpose(0, 1)[None].contiguous()


@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=rr.IDS)
def test_a_sequences_rows_are_the_uniform_calls_bit_for_bit(i):
    """flash_attention_2_extend / _paged once per sequence with q_b >= 1 -- B = 1, q_len = q_b, its cache slab or table row, its
    length, the same explicit n_splits -- under every variant and both element sizes."""
    fa, c = _fa(), rr.CASES[i]
    cu = rr.cu_of(c["qs"])
    P = 32
    for k in range(len(rr.VARIANTS)):
        for fp8 in (False, True):
            Q, K, V = _dev(i, fp8)[:3]
            Kp, Vp, table, cap = _pages(i, P, fp8)
            kw = _kw(i, k, fp8)
            lens = kw.pop("seqlens_k")
            for n_splits in (1, 2, 7, 64) if k in (0, 5) else (1, 7):
                got = _contiguous(i, k, fp8, n_splits)
                gotp = _paged(i, k, fp8, P, n_splits) if n_splits in (2, 7) else None
                for b, q in enumerate(c["qs"]):
                    if not q:
                        continue
                    Qb = Q[cu[b]:cu[b + 1]].transpose(0, 1)[None].contiguous()
                    lb = None if lens is None else lens[b:b + 1]
                    want = fa.flash_attention_2_extend(Qb, K[b:b + 1], V[b:b + 1], lb, n_splits=n_splits, **kw)
                    _same_bits(_rows_of(got, cu, b), want, (rr.IDS[i], k, fp8, n_splits, b))
                    if gotp is not None:
                        want = fa.flash_attention_2_extend_paged(Qb, Kp, Vp, table[b:b + 1], lb, n_splits=n_splits, **kw)
                        _same_bits(_rows_of(gotp, cu, b), want, (rr.IDS[i], k, fp8, n_splits, b, "paged"))


@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=rr.IDS)
def test_default_split_count_is_the_helpers(i):
    fa, c = _fa(), rr.CASES[i]
    B, T = len(c["qs"]), rr.total_q(c)
    for k in (0, 1, 4, 7):
        wl = rr.VARIANTS[k][1]
        n = fa.extend_ragged_num_splits(B, c["hq"], c["hkv"], T, c["ncap"], c["d"], window_left=wl)
        assert n == rr.num_splits(B, c["hq"], c["hkv"], T, c["ncap"], wl)
        for fp8 in (False, True):
            _same_bits(_contiguous(i, k, fp8, 0), _contiguous(i, k, fp8, n), (rr.IDS[i], k, fp8, n))
            cap = _pages(i, 96, fp8)[3]
            n96 = fa.extend_ragged_num_splits(B, c["hq"], c["hkv"], T, cap, c["d"], window_left=wl)
            _same_bits(_paged(i, k, fp8, 96, 0), _paged(i, k, fp8, 96, n96), (rr.IDS[i], k, fp8, n96, "paged"))


@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=rr.IDS)
def test_paged_equals_contiguous_on_the_gathered_cache(i):
    c = rr.CASES[i]
    for k in (0, 1, 4, 7):      # causal, full, windows 31 and 200
        for fp8 in (False, True):
            for P in rr.PAGE_SIZES:
                Kp, Vp, table, cap = _pages(i, P, fp8)
                lens = rr.lens_under(c, cap)
                K, V = _gather(Kp, table, lens, P), _gather(Vp, table, lens, P)
                assert K.shape[2] == cap
                for n_splits in c["splits"]:
                    got = _paged(i, k, fp8, P, n_splits)
                    _same_bits(got, _contiguous(i, k, fp8, n_splits, K=K, V=V), (rr.IDS[i], k, fp8, P, n_splits))
                if not c["seqlens"] and not fp8:      # the capacity is the pages': the reference on the gathered cache
                    Q, _, _, scale, _, sink, _ = rr.inputs(i)
                    ref = rr.reference64(Q, K.cpu(), V.cpu(), c["qs"], lens, scale, rr.VARIANTS[k][0] == "causal",
                                         sink if rr.has_sink(i, k) else None, rr.VARIANTS[k][1])
                    _check(f"{rr.IDS[i]} variant {k} page {P}", *got, ref)


# ---- 3. the plan
@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=rr.IDS)
def test_the_plan_is_the_models(i):
    fa, c = _fa(), rr.CASES[i]
    G, T, B = c["hq"] // c["hkv"], rr.total_q(c), len(c["qs"])
    plan = _plan(i)
    assert plan.tensor.dtype == torch.int32 and plan.tensor.numel() * 4 == rr.plan_bytes(B, c["hq"], c["hkv"], T)
    assert plan.tensor.cpu().tolist()[:rr.plan_ints(B, c["hq"], c["hkv"], T)] == rr.plan_model(rr.cu_of(c["qs"]), G, T)
    # more tokens than the sequences own, in a caller's buffer between guard bands
    n = rr.plan_bytes(B, c["hq"], c["hkv"], T + 9) // 4
    big = torch.full((n + 128,), SENT32, dtype=torch.int32, device="cuda")
    p2 = fa.extend_ragged_plan(_dev(i, False)[8], c["hq"], c["hkv"], T + 9, plan=big[64:64 + n])
    assert p2.tensor.data_ptr() == big[64:].data_ptr()
    assert big[64:64 + rr.plan_ints(B, c["hq"], c["hkv"], T + 9)].cpu().tolist() == rr.plan_model(rr.cu_of(c["qs"]), G, T + 9)
    assert (big[:64] == SENT32).all() and (big[64 + n:] == SENT32).all()


def test_one_plan_serves_calls_on_different_caches():
    i = rr.IDS.index("mixed-d128")
    plan = _plan(i)
    Q, K, V = _dev(i, False)[:3]
    K2, V2 = V.clone(), K.clone()
    for n_splits in (1, 7):
        a = _contiguous(i, 0, False, n_splits, plan=plan)
        b = _contiguous(i, 0, False, n_splits, K=K2, V=V2, plan=plan)
        a2 = _contiguous(i, 0, False, n_splits, plan=_fa().extend_ragged_plan(_dev(i, False)[8], 8, 2, Q.shape[0]))
        b2 = _contiguous(i, 0, False, n_splits, K=K2, V=V2, plan=_fa().extend_ragged_plan(_dev(i, False)[8], 8, 2, Q.shape[0]))
        _same_bits(a, a2, ("first", n_splits))
        _same_bits(b, b2, ("second", n_splits))
        assert not torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    _check("mixed-d128 reused plan", *a, rr.reference(i, 0, False))


def _carved(n, dtype, pad, fill):
    """A tensor of n elements between two guard bands of `pad` elements holding `fill`: (the whole buffer, the view)."""
    big = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
    return big, big[pad:pad + n]


MALFORMED = {
    "decreasing": [0, 30, 12, 40, 38, 95],
    "negative": [-7, -1, 20, 21, -2 ** 31, 60],
    "above": [0, 50, 200, 2 ** 31 - 1, 96, 95],
    "all-above": [100, 101, 102, 103, 104, 105],
    "short": [5, 5, 9, 9, 41, 41],
}


@pytest.mark.parametrize("name", sorted(MALFORMED), ids=sorted(MALFORMED))
def test_a_malformed_cu_seqlens_gives_the_sanitised_plan_and_stays_inside(name):
    """T = 95 tokens on 8 heads over 2, five sequences: the stored plan is the model's sanitised one; the call computes exactly those
    sequences (the reference on the sanitised q_b, within the gates), tokens of no sequence keep their sentinel and so do the
    guard bands around O and L -- with one split and through the combine."""
    fa = _fa()
    i = rr.IDS.index("mixed-d64")
    Q, K, V, _, _, scale, lens, sink, _ = _dev(i, False)
    hq, hkv, d, T, B, pad = 8, 2, 64, 95, 5, 512
    cu = MALFORMED[name]
    plan = fa.extend_ragged_plan(torch.tensor(cu, dtype=torch.int32, device="cuda"), hq, hkv, T)
    assert plan.tensor.cpu().tolist()[:rr.plan_ints(B, hq, hkv, T)] == rr.plan_model(cu, hq // hkv, T)
    seq = rr.sanitised(cu, T)
    first, last = seq[0][0], seq[-1][0] + seq[-1][1]
    owned = torch.zeros(T, dtype=torch.bool)
    owned[first:last] = True
    qs = [q for _, q in seq]
    Qh, Kh, Vh = rr.inputs(i)[:3]
    ref = rr.reference64(Qh[first:], Kh[:B], Vh[:B], qs, rr.CASES[i]["lens"][:B], scale, True, sink.cpu(), 127)
    for n_splits in (1, 3):
        bO, O = _carved(T * hq * d, torch.int16, pad, SENT16)
        bL, L = _carved(T * hq, torch.int32, pad, SENT32)
        got = fa.flash_attention_2_extend_ragged(Q, K[:B], V[:B], plan, lens[:B], scale, sink=sink, n_splits=n_splits, window_left=127,
                                                 O=O.view(torch.bfloat16).view(T, hq, d), L=L.view(torch.float32).view(T, hq))
        torch.cuda.synchronize()
        for big, sent in ((bO, SENT16), (bL, SENT32)):
            assert (big[:pad] == sent).all() and (big[-pad:] == sent).all(), (name, n_splits)
        Oi, Li = O.view(T, hq * d).cpu(), L.view(T, hq).cpu()
        assert (Oi[~owned] == SENT16).all() and (Li[~owned] == SENT32).all(), (name, n_splits)
        assert not (Oi[owned] == SENT16).any() and not (Li[owned] == SENT32).any(), (name, n_splits)
        if last > first:
            _check(f"{name} splits {n_splits}", got[0][first:last], got[1][first:last], ref.head(last - first))


# ---- 4. strides: the Q slice of a fused QKV output
@pytest.mark.parametrize("i", [rr.IDS.index(n) for n in ("mixed-d64", "g1-d128", "mqa-d128")], ids=("mixed-d64", "g1-d128", "mqa-d128"))
def test_q_as_a_slice_of_a_fused_qkv_buffer(i):
    c = rr.CASES[i]
    T, hq, hkv, d = rr.total_q(c), c["hq"], c["hkv"], c["d"]
    fused = torch.full((T, (hq + 2 * hkv) * d), float("nan"), dtype=torch.bfloat16, device="cuda")
    Q = fused[:, :hq * d].view(T, hq, d)
    Q.copy_(_dev(i, False)[0])
    assert not Q.is_contiguous() and Q.stride(0) == (hq + 2 * hkv) * d
    for fp8 in (False, True):
        for k in (0, 4):
            for n_splits in (1, 7):
                _same_bits(_contiguous(i, k, fp8, n_splits, Q=Q), _contiguous(i, k, fp8, n_splits), (rr.IDS[i], fp8, k, n_splits))
                _same_bits(_paged(i, k, fp8, 32, n_splits, Q=Q), _paged(i, k, fp8, 32, n_splits), (rr.IDS[i], fp8, k, n_splits, "paged"))


# ---- 5. garbage past the lengths and below the windows, guard bands, a NaN workspace, tokens of no sequence
GARBAGE = [(rr.IDS.index(n), k) for n in ("mixed-d64", "mixed-d128", "g1-d64", "decode-d128") for k in (0, 1, 4, 7)]
EXTRA = 5      # tokens behind cu[B]: T = sum q_b + EXTRA


def _unread(c, k, shape):
    """bool [B, H_kv, N_cap, d]: the cache rows no query may read -- at and past each length, below lo_b = len_b - q_b - window_left
    under a window, and every row of a sequence without a query."""
    out = fr.past_lengths(shape, c["lens"])
    wl = rr.VARIANTS[k][1]
    for b, (q, n) in enumerate(zip(c["qs"], c["lens"])):
        if not q:
            out[b] = True
        elif wl is not None:
            out[b, :, :max(0, n - q - wl)] = True
    return out


def _filled(i, k, fp8, fill):
    c = rr.CASES[i]
    K, V = (rr.inputs_fp8(i) if fp8 else rr.inputs(i))[1:3]
    where = _unread(c, k, K.shape)
    if fp8:
        return fr.filled(K, where, fill), fr.filled(V, where, fill)
    return tuple(torch.where(where, torch.tensor(fill, dtype=torch.bfloat16), t) for t in (K, V))


def _pools(i, k, fp8, P, K, V, garbage):
    """Pools and a table of host caches K, V.  garbage: what no key was copied to is NaN, unused entries are -1 / INT_MAX, and the
    entries of the pages wholly below lo_b -- every entry of a sequence without a query -- are -1, INT_MAX, INT_MIN and n_pages in
    turn; otherwise zeros and entry 0."""
    c = rr.CASES[i]
    img = (lambda t: t.to(torch.bfloat16)) if fp8 else (lambda t: t)
    Kp, Vp, table = pr.build(img(K), img(V), c["lens"], P, 99500 + 17 * i + P, fill=float("nan") if garbage else 0.0,
                             unused=pr.UNUSED if garbage else (0, 0))
    rr.shared_pages(c, table, P)
    if garbage:
        bad, n, wl = (-1, INT_MAX, INT_MIN, Kp.shape[0]), 0, rr.VARIANTS[k][1]
        for b, (q, ln) in enumerate(zip(c["qs"], c["lens"])):
            below = table.shape[1] if not q else 0 if wl is None else max(0, ln - q - wl) // P
            for p in range(below):
                table[b, p] = bad[n % 4]
                n += 1
    if fp8:
        Kp, Vp = Kp.to(fr.E4M3), Vp.to(fr.E4M3)
    return Kp.cuda(), Vp.cuda(), table.cuda()


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("i,k", GARBAGE, ids=[rr.RUN_IDS[rr.RUNS.index(r)] for r in GARBAGE])
def test_garbage_changes_nothing_and_what_no_sequence_owns_stays(i, k, fp8):
    fa, c = _fa(), rr.CASES[i]
    B, hq, hkv, d, Ts = len(c["qs"]), c["hq"], c["hkv"], c["d"], rr.total_q(c)
    T = Ts + EXTRA
    Q = torch.cat([_dev(i, fp8)[0], torch.full((EXTRA, hq, d), float("nan"), dtype=torch.bfloat16, device="cuda")])
    pbytes = rr.plan_bytes(B, hq, hkv, T)
    bP, Pl = _carved(pbytes // 4, torch.int32, 64, SENT32)
    plan = fa.extend_ragged_plan(_dev(i, fp8)[8], hq, hkv, T, plan=Pl)
    zero = _filled(i, k, fp8, 0x00 if fp8 else 0.0)
    fills = fr.NAN_CODES if fp8 else (float("nan"),)
    dirty = [_filled(i, k, fp8, f) for f in fills]
    ref = rr.reference(i, k, fp8)
    pad = 512
    wl = rr.VARIANTS[k][1]
    for n_splits in (1, 2, 7):
        need = fa.extend_ragged_workspace(B, hq, hkv, T, c["ncap"], d, n_splits, device="cpu", window_left=wl).numel()
        assert (need > 0) == (n_splits > 1) and need == rr.workspace_bytes(hq, T, d, n_splits)
        want = _contiguous(i, k, fp8, n_splits, K=zero[0].cuda(), V=zero[1].cuda(), Q=Q, plan=plan)
        _check(f"{rr.IDS[i]} zeros splits {n_splits}", want[0][:Ts], want[1][:Ts], ref)
        for f, (K, V) in zip(fills, dirty):
            bO, O = _carved(T * hq * d, torch.int16, pad, SENT16)
            bL, L = _carved(T * hq, torch.int32, pad, SENT32)
            bW, W = _carved(max(need // 4, 64), torch.float32, pad, float("nan"))      # the workspace starts as NaNs
            got = _contiguous(i, k, fp8, n_splits, K=K.cuda(), V=V.cuda(), Q=Q, plan=plan, O=O.view(torch.bfloat16).view(T, hq, d),
                              L=L.view(torch.float32).view(T, hq), workspace=W.view(torch.uint8))
            _same_bits((got[0][:Ts], got[1][:Ts]), (want[0][:Ts], want[1][:Ts]), (rr.IDS[i], n_splits, f))
            assert not (O[:Ts * hq * d] == SENT16).any() and not (L[:Ts * hq] == SENT32).any()      # every owned element written
            assert (O[Ts * hq * d:] == SENT16).all() and (L[Ts * hq:] == SENT32).all()              # the tokens behind cu[B] are not
            for big, sent, band in ((bO, SENT16, pad), (bL, SENT32, pad), (bP, SENT32, 64)):
                assert (big[:band] == sent).all() and (big[-band:] == sent).all()
            assert torch.isnan(bW[:pad]).all() and torch.isnan(bW[-pad:]).all() and torch.isnan(W[need // 4:]).all()
    assert Pl.cpu().tolist()[:rr.plan_ints(B, hq, hkv, T)] == rr.plan_model(rr.cu_of(c["qs"]), hq // hkv, T)      # the calls only read it
    for P in rr.PAGE_SIZES:
        clean = _pools(i, k, fp8, P, *zero, garbage=False)
        nasty = _pools(i, k, fp8, P, *dirty[0], garbage=True)
        assert not torch.equal(clean[2], nasty[2])
        for n_splits in (1, 2, 7):
            want = _paged(i, k, fp8, P, n_splits, pools=clean, Q=Q, plan=plan)
            _check(f"{rr.IDS[i]} page {P} zeros splits {n_splits}", want[0][:Ts], want[1][:Ts], ref)
            got = _paged(i, k, fp8, P, n_splits, pools=nasty, Q=Q, plan=plan)
            _same_bits((got[0][:Ts], got[1][:Ts]), (want[0][:Ts], want[1][:Ts]), (rr.IDS[i], P, n_splits, "garbage"))


# ---- 6. one captured graph of {plan, ragged extend}
def test_one_captured_graph_of_plan_and_extend_serves_a_changing_mix():
    """Paged bf16, 8 heads over 2, pages of 32 keys, window_left = 200, two splits, T = 24 packed tokens for B = 4 sequences.
    Captured once on a single stream with a caller plan buffer, workspace, O and L; between the three replays cu_seqlens_q and
    seqlens_k are rewritten IN PLACE: all-decode (1 1 1 1; twenty tokens of no sequence), a chunk plus decodes (21 1 1 1), and a
    mix that takes sequence 1 across the 128-key boundary (3 17 1 3).  Every replay is bit for bit the eager calls and inside the
    gates of the float64 reference; tokens of no sequence keep their sentinel."""
    fa = _fa()
    hq, hkv, d, P, wl, B, T, max_pages = 8, 2, 128, 32, 200, 4, 24, 8
    n_pages = B * max_pages + 3
    g = torch.Generator().manual_seed(9911)
    rnd = lambda *shape: (torch.rand(*shape, generator=g) - 0.5).bfloat16()
    K, V = rnd(B, hkv, max_pages * P, d), rnd(B, hkv, max_pages * P, d)
    table_host = torch.randperm(n_pages, generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)
    Kp, Vp = (torch.zeros(n_pages, hkv, P, d, dtype=torch.bfloat16) for _ in range(2))
    for b in range(B):
        for p in range(max_pages):
            Kp[table_host[b, p]], Vp[table_host[b, p]] = K[b, :, p * P:(p + 1) * P], V[b, :, p * P:(p + 1) * P]
    Kp, Vp, table = Kp.cuda(), Vp.cuda(), table_host.cuda()
    steps = (((1, 1, 1, 1), (100, 127, 30, 5)), ((21, 1, 1, 1), (121, 128, 31, 6)), ((3, 17, 1, 3), (124, 145, 32, 9)))
    cu = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    lens = torch.zeros(B, dtype=torch.int32, device="cuda")
    Q = torch.zeros(T, hq, d, dtype=torch.bfloat16, device="cuda")
    O, L = torch.empty_like(Q), torch.empty(T, hq, dtype=torch.float32, device="cuda")
    ws = fa.extend_ragged_workspace(B, hq, hkv, T, max_pages * P, d, 2, window_left=wl)
    assert ws.numel() > 0
    buf = torch.zeros(rr.plan_bytes(B, hq, hkv, T) // 4, dtype=torch.int32, device="cuda")
    sink = dr.sink_of(hq, 99).cuda()

    def step(buf, O, L, ws):
        plan = fa.extend_ragged_plan(cu, hq, hkv, T, plan=buf)
        return fa.flash_attention_2_extend_ragged_paged(Q, Kp, Vp, table, plan, lens, sink=sink, n_splits=2, O=O, L=L, workspace=ws,
                                                        window_left=wl)

    step(torch.empty_like(buf), torch.empty_like(O), torch.empty_like(L), torch.empty_like(ws))      # the code objects load outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(buf, O, L, ws)
    torch.cuda.current_stream().wait_stream(side)
    for s, (qs, ls) in enumerate(steps):
        cu.copy_(torch.tensor(rr.cu_of(qs), dtype=torch.int32))
        lens.copy_(torch.tensor(ls, dtype=torch.int32))
        q = rnd(T, hq, d)
        Q.copy_(q.cuda())
        O.view(torch.int16).fill_(SENT16)
        L.view(torch.int32).fill_(SENT32)
        graph.replay()
        torch.cuda.synchronize()
        Oe, Le = torch.empty_like(O), torch.empty_like(L)
        Oe.view(torch.int16).fill_(SENT16)
        Le.view(torch.int32).fill_(SENT32)
        step(torch.empty_like(buf), Oe, Le, torch.empty_like(ws))
        torch.cuda.synchronize()
        _same_bits((O, L), (Oe, Le), ("replay", s))
        n = sum(qs)
        assert buf.cpu().tolist()[:rr.plan_ints(B, hq, hkv, T)] == rr.plan_model(rr.cu_of(qs), hq // hkv, T)
        assert (O[n:].view(torch.int16) == SENT16).all() and (L[n:].view(torch.int32) == SENT32).all()
        ref = rr.reference64(q[:n], K, V, qs, ls, 1.0 / d ** 0.5, True, sink.cpu(), wl)
        _check(f"replay {s} q {qs} lens {ls}", O[:n], L[:n], ref)


# ---- 7. (O, L) is what merge_states_forward takes
def test_two_calls_over_two_halves_of_the_keys_merge_into_one():
    """Keys [0, 64) without a mask or a sink (every query of these sequences sees all of them), keys [64, len_b) with the mask and
    the sink, merged on the flattened rows: within the gates of the one call's reference, and of the one call."""
    fa = _fa()
    hq, hkv, d, cap, h = 8, 2, 64, 320, 64
    qs, ls = (1, 9, 20, 0, 3), (100, 200, 300, 150, 67)
    B, T = len(qs), sum(qs)
    g = torch.Generator().manual_seed(9922)
    rnd = lambda *shape: (torch.rand(*shape, generator=g) - 0.5).bfloat16()
    Q, K, V = rnd(T, hq, d), rnd(B, hkv, cap, d), rnd(B, hkv, cap, d)
    sink = dr.sink_of(hq, 101)
    cu = torch.tensor(rr.cu_of(qs), dtype=torch.int32, device="cuda")
    plan = fa.extend_ragged_plan(cu, hq, hkv, T)
    Qd, Kd, Vd = Q.cuda(), K.cuda(), V.cuda()
    lens = torch.tensor(ls, dtype=torch.int32, device="cuda")
    ref = rr.reference64(Q, K, V, qs, ls, 1.0 / d ** 0.5, True, sink, None)
    # the two partial O's are rounded to bf16 before the merge weighs them: u (w_a |O_a,i| + w_b |O_b,i|) on top of the row gate
    parts = [rr.reference64(Q, K[:, :, :h], V[:, :, :h], qs, [h] * B, 1.0 / d ** 0.5, False, None, None),
             rr.reference64(Q, K[:, :, h:], V[:, :, h:], qs, [n - h for n in ls], 1.0 / d ** 0.5, True, sink, None)]
    extra = rows.merged_extra(parts, ref[1])
    for n_splits in (1, 2):
        O1, L1 = fa.flash_attention_2_extend_ragged(Qd, Kd[:, :, :h].contiguous(), Vd[:, :, :h].contiguous(), plan, None, causal=False,
                                                    n_splits=n_splits)
        O2, L2 = fa.flash_attention_2_extend_ragged(Qd, Kd[:, :, h:].contiguous(), Vd[:, :, h:].contiguous(), plan, lens - h, causal=True,
                                                    sink=sink.cuda(), n_splits=n_splits)
        Om, Lm = fa.merge_states_forward([O1.flatten(0, 1), O2.flatten(0, 1)], [L1.flatten(), L2.flatten()])
        one = fa.flash_attention_2_extend_ragged(Qd, Kd, Vd, plan, lens, sink=sink.cuda(), n_splits=n_splits)
        _check(f"one call splits {n_splits}", *one, ref)
        _check(f"merged splits {n_splits}", Om.view(T, hq, d), Lm.view(T, hq), ref, extra=extra)
