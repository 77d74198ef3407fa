"""GPU: the regimes of tests/regimes.py on every body of the cache-side attention family, gated per row.

Before this file only the plain decode ran `peaked`, `spikes`, `scale-one` and `low-level` (and the paged decode one of them); the
windowed and e4m3 instantiations, extend (a body of its own: two row tiles that meet through one LDS image) and ragged extend with
their combine kernel had only seen flat softmax -- no running maximum that jumps by 100, no wave or split whose weight underflows
to 0 beside another, no L < -88, no spike key in a tile the window drops.

RUNS (tests/decode_rows_cases.py): decode (8, 2) N_q = 4, extend (8, 2) N_q = 17 (M = 68, a spiked head in each row tile), ragged
extend (8, 2) with q_b = (17, 1, 4) on lengths (1100, 300, 1100); lengths 300 and 1100 in one batch, causal, d = 64 and 128.  A test is
one (body, d, regime) and loops over bf16 and e4m3 caches, contiguous and behind pages of 32, no window and window_left 127 and
200, and 1, 7 and 0 splits; the sink alternates (none under `low-level`).

GATES, all against the float64 reference (on the dequantised caches for e4m3): the row gate of tests/decode_rows_ref.py on every
row of O, decode_ref's L gates per row, the -inf / zero-row rules and the tensor gate (decode_ref.within_gates).
tests/test_decode_rows_reference.py certifies on the CPU that the emulated data flow uses at most 0.75 of each on these inputs,
that the rows which see a spike have L above regimes.SPIKE_L and that every `low-level` L is below -88.
BIT IDENTITIES, on these inputs too: paged equals contiguous; an extend row is the decode's row on Q[:, g::G]; a ragged
sequence's rows are the extend call's on that sequence alone (explicit split counts)."""
import pytest
import torch

import decode_ref as dr
import decode_rows_cases as rc
import decode_rows_ref as rows
import extend_ragged_ref as rr

pytestmark = pytest.mark.gpu


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _same_bits(got, want, where):
    assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), (where, "O")
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (where, "L")


def _check(where, O, L, ref, cu):
    e = dr.errors(O.float().cpu().numpy(), L.cpu().numpy(), ref)
    print(where, f"O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
    assert dr.within_gates(e), (where, e)
    return rows.check(where, O, ref, cu=cu)


def _call(body, paged, Q, caches, plan, **kw):
    fa = _fa()
    if body == "ragged":
        f = fa.flash_attention_2_extend_ragged_paged if paged else fa.flash_attention_2_extend_ragged
        return f(Q, *caches, plan, **kw)
    name = "flash_attention_2_" + body + ("_paged" if paged else "")
    return getattr(fa, name)(Q, *caches, **kw)


@pytest.mark.parametrize("run", rc.RUNS, ids=rc.RUN_IDS)
def test_the_regimes_on_every_body(run):
    fa = _fa()
    body, d, regime = run
    Q, K, V, scale, lens, sink, cu = rc.inputs(body, d, regime)
    qs, _ = rc.shape_of(body)
    Qd, lens_d, sink_d = Q.cuda(), lens.cuda(), sink.cuda()
    cu_host = None if cu is None else cu.tolist()
    plan = fa.extend_ragged_plan(cu.cuda(), rc.HQ, rc.HKV, Q.shape[0]) if body == "ragged" else None
    G = rc.HQ // rc.HKV
    top = 0.0
    for kind in rc.KINDS:
        if kind == "bf16":
            flat, kd, vd = (K.cuda(), V.cuda()), None, None
        else:
            K8, V8, kd, vd = (t.cuda() for t in rc.inputs_fp8(body, d, regime))
            flat = (K8, V8)
        pools = tuple(t.cuda() for t in rc.paged_inputs(body, d, regime, kind))
        for wi, wl in enumerate(rc.WINDOWS):
            ref = rc.reference(body, d, regime, kind, wi)
            s = sink_d if rc.has_sink(regime, kind, wi) else None
            kw = dict(seqlens_k=lens_d, softmax_scale=scale, causal=True, sink=s, k_descale=kd, v_descale=vd, window_left=wl)
            for n_splits in rc.SPLITS:
                where = f"{rc.RUN_IDS[rc.RUNS.index(run)]} {kind} w{wl} splits {n_splits}"
                got = _call(body, False, Qd, flat, plan, n_splits=n_splits, **kw)
                top = max(top, _check(where, *got, ref, cu_host))
                gotp = _call(body, True, Qd, pools, plan, n_splits=n_splits, **kw)
                _same_bits(gotp, got, (where, "paged"))      # (so the paged call is inside every gate as well)
                if not n_splits:
                    continue
                if body == "extend":      # a row is the decode's row: the sibling once per group member, on Q[:, g::G]
                    for g in range(G):
                        want = fa.flash_attention_2_decode(Qd[:, g::G].contiguous(), *flat, n_splits=n_splits,
                                                           **dict(kw, sink=None if s is None else s[g::G].contiguous()))
                        _same_bits((got[0][:, g::G].contiguous(), got[1][:, g::G].contiguous()), want, (where, "decode rows", g))
                if body == "ragged":      # a sequence's rows are the extend call's on that sequence alone
                    for b, q in enumerate(qs):
                        t0, t1 = cu_host[b], cu_host[b + 1]
                        want = fa.flash_attention_2_extend(Qd[t0:t1].transpose(0, 1)[None].contiguous(), flat[0][b:b + 1], flat[1][b:b + 1],
                                                           n_splits=n_splits, **dict(kw, seqlens_k=lens_d[b:b + 1]))
                        _same_bits((got[0][t0:t1].transpose(0, 1)[None].contiguous(), got[1][t0:t1].transpose(0, 1)[None].contiguous()),
                                   want, (where, "extend rows", b))
    print(f"ROWS-GPU {rc.RUN_IDS[rc.RUNS.index(run)]}: largest row ratio {top:.3f}")
