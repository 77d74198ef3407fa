"""CPU: what tests/extend_ragged_ref.py provides, before tests/test_gpu_extend_ragged.py relies on it.
(i) The cases are the ones the issue sets, with the lengths it asks for.
(ii) The modelled plan (plan_model, the plan kernel in Python integers) puts every live row in exactly one work item, never
exceeds max_blocks and keeps start_b + q_b <= T -- on every case and on a few hundred random cu_seqlens_q, non-monotone and
out-of-range ones included.
(iii) The clip of a work item is extend_ref.block_tiles with q_b for N_q: on every case, variant, sequence and split count it
drops no visible key, processes each tile once and on the wave the siblings give it.
(iv) The packed reference is extend_ref's on a uniform batch."""
import random

import numpy as np
import pytest
import torch

import extend_ragged_ref as rr
import extend_ref as er


def test_cases_are_the_issues():
    by = {c["name"]: c for c in rr.CASES if c["d"] == 64}
    assert [(c["name"], c["d"]) for c in rr.CASES] == [(n, d) for n in ("mixed", "mqa", "g1", "decode", "nolens") for d in (64, 128)]
    assert (by["mixed"]["hq"], by["mixed"]["hkv"], by["mixed"]["qs"]) == (8, 2, (0, 1, 8, 9, 16, 17, 1, 40, 3, 0))
    assert [4 * q for q in by["mixed"]["qs"]] == [0, 4, 32, 36, 64, 68, 4, 160, 12, 0]
    assert (by["mqa"]["hq"], by["mqa"]["hkv"], by["mqa"]["qs"]) == (33, 1, (1, 1, 2, 0, 1))
    assert (by["g1"]["hq"], by["g1"]["hkv"], by["g1"]["qs"]) == (4, 4, (70, 1, 64, 65, 33))
    assert (by["decode"]["hq"], by["decode"]["hkv"], by["decode"]["qs"]) == (16, 2, (1,) * 10)
    assert (by["nolens"]["hq"], by["nolens"]["hkv"], by["nolens"]["qs"], by["nolens"]["ncap"], by["nolens"]["seqlens"]) == (8, 1, (5, 24), 300, False)
    for c in rr.CASES:
        assert c["splits"] == (0, 1, 2, 7, 64) and len(c["qs"]) == len(c["lens"])
        if not c["seqlens"]:
            continue
        assert c["ncap"] == 2560
        pairs = list(zip(c["qs"], c["lens"]))
        for q, n in pairs:
            assert n in {0, 1, q - 1, q, 127, 128, 129, 300, 1100, 2500}, (c["name"], q, n)
        live = [(q, n) for q, n in pairs if q]
        assert any(n < q for q, n in live) and any(n == q for q, n in live), c["name"]
        lo, hi = {n for _, n in live} & {127, 128}, {n for _, n in live} & {128, 129}      # each side of a 128-key boundary
        assert lo and hi and len(lo | hi) >= 2, c["name"]
        if c["share"]:
            s, t = c["share"]
            assert c["qs"][s] and c["qs"][t] and min(c["lens"][s], c["lens"][t]) >= rr.SHARED_KEYS
    assert rr.VARIANTS == er.VARIANTS
    for i in range(len(rr.CASES)):
        assert {rr.has_sink(i, k) for k in range(2, len(rr.VARIANTS))} == {False, True}


def _check_plan(cu, B, G, T):
    plan = rr.plan_model(cu, G, T)
    hq, hkv = G, 1
    mb = rr.max_blocks(B, hq, hkv, T)
    assert len(plan) == rr.plan_ints(B, hq, hkv, T) and plan[3] <= mb
    seq = rr.sanitised(cu, T)
    assert sum(q for _, q in seq) <= T
    at = seq[0][0]
    for start, q in seq:      # the sequences tile [first, last) in order
        assert 0 <= start and q >= 0 and start + q <= T and start == at
        at += q
    assert (plan[4], plan[5]) == (seq[0][0], at)
    rows = rr.plan_rows(plan, G)
    assert set(rows) == {(t, g) for start, q in seq for t in range(start, start + q) for g in range(G)}
    items = [(plan[rr.HEADER + 2 * B + 2 * i], plan[rr.HEADER + 2 * B + 2 * i + 1]) for i in range(mb)]
    assert items[:plan[3]] == sorted(items[:plan[3]]) and all(it == (-1, 0) for it in items[plan[3]:])
    return seq


def test_the_plan_covers_every_live_row_once_on_the_cases():
    for c in rr.CASES:
        cu, T = rr.cu_of(c["qs"]), rr.total_q(c)
        seq = _check_plan(cu, len(c["qs"]), c["hq"] // c["hkv"], T)
        assert seq == [(cu[b], c["qs"][b]) for b in range(len(c["qs"]))]      # a well-formed cu_seqlens_q is taken as it is
        seq = _check_plan(cu, len(c["qs"]), c["hq"] // c["hkv"], T + 7)       # cu[B] < T: the last tokens belong to no sequence
        assert seq[-1][0] + seq[-1][1] == T


def test_the_plan_is_safe_on_random_cu_seqlens():
    rnd = random.Random(4711)
    shapes = 0
    for n in range(400):
        B, G, T = rnd.choice((1, 2, 5, 17, 300)), rnd.choice((1, 4, 8, 33)), rnd.choice((1, 3, 64, 200, 1000))
        kind = n % 4
        if kind == 0:      # well formed
            cuts = sorted(rnd.randint(0, T) for _ in range(B + 1))
        elif kind == 1:    # non-monotone, in range
            cuts = [rnd.randint(0, T) for _ in range(B + 1)]
        elif kind == 2:    # out of range on both sides
            cuts = [rnd.randint(-T - 5, 2 * T + 5) for _ in range(B + 1)]
        else:              # the extremes of an int
            cuts = [rnd.choice((-2 ** 31, -1, 0, T // 2, T, T + 1, 2 ** 31 - 1)) for _ in range(B + 1)]
        _check_plan(cuts, B, G, T)
        shapes += 1
    assert shapes == 400
    # the documented outcomes: a decreasing entry is an empty sequence, an entry out of range is clamped
    assert rr.sanitised([0, 5, 3, 9], 9) == [(0, 5), (5, 0), (5, 4)]
    assert rr.sanitised([-4, 2, 50], 9) == [(0, 2), (2, 7)]
    assert rr.sanitised([12, 2, 3], 9) == [(9, 0), (9, 0)]


@pytest.mark.parametrize("i", range(len(rr.CASES)), ids=rr.IDS)
def test_the_work_item_clip_drops_no_visible_key(i):
    """extend_ref's check of the uniform call, per sequence with N_q = q_b: the ragged body's clip is that one with q_b."""
    c = rr.CASES[i]
    G = c["hq"] // c["hkv"]
    skipped = exits = 0
    for mask, wl in rr.VARIANTS:
        causal = mask == "causal"
        for q, n in sorted(set(zip(c["qs"], c["lens"]))):
            if not q:
                continue
            M = G * q
            for n_splits in (1, 2, 7, 64):
                for s in range(n_splits):
                    begin, end = er.split_range(n, q, wl, n_splits, s)
                    for j in range(-(-M // rr.ROWS)):
                        seen = set()
                        for rho in range(rr.ROWS * j, min(rr.ROWS * (j + 1), M)):
                            kmin, kmax = er.row_window(rho, q, n, causal, wl)
                            seen.update(range(max(kmin, begin), min(kmax, end)))
                        tiles = er.block_tiles(M, q, n, causal, wl, n_splits, s, j)
                        if tiles is None:
                            assert not seen, (mask, wl, q, n, n_splits, s, j)
                            exits += 1
                            continue
                        flat = [kb for w in tiles for kb in tiles[w]]
                        assert len(flat) == len(set(flat))
                        for w, kbs in tiles.items():
                            assert kbs == sorted(kbs)
                            for kb in kbs:
                                assert begin <= kb < end and (kb - begin) % rr.TILE == 0 and (kb - begin) // rr.TILE % rr.WAVES == w
                        assert {key // rr.TILE for key in seen} <= {kb // rr.TILE for kb in flat}, (mask, wl, q, n, n_splits, s, j)
                        skipped += len(range(begin, end, rr.TILE)) - len(flat)
    assert exits > 0
    if c["name"] in ("mixed", "g1"):
        assert skipped > 0      # the clip does skip tiles where a sequence has more than one token


def test_packed_reference_is_extend_refs_on_a_uniform_batch():
    i = next(k for k, c in enumerate(er.CASES) if (c["hq"], c["hkv"], c["nq"], c["d"]) == (8, 1, 5, 64) and c["seqlens"])
    c = er.CASES[i]
    Q, K, V, scale, _, sink = er.inputs(i)
    B, nq = len(c["lens"]), c["nq"]
    packed = Q.permute(0, 2, 1, 3).reshape(B * nq, c["hq"], c["d"])
    for causal, wl, sk in ((True, None, None), (False, None, sink), (True, 31, sink)):
        O, L = rr.reference64(packed, K, V, (nq,) * B, c["lens"], scale, causal, sk, wl)
        rO, rL = er.reference64(Q, K, V, c["lens"], scale, causal, sk, wl)
        assert np.array_equal(O.reshape(B, nq, c["hq"], c["d"]).transpose(0, 2, 1, 3), rO)
        assert np.array_equal(L.reshape(B, nq, c["hq"]).transpose(0, 2, 1), rL)
    O, L = rr.reference64(torch.cat([packed, packed[:3]]), K, V, (nq,) * B, c["lens"], scale, True, None, None)
    assert np.isnan(O[B * nq:]).all() and np.isnan(L[B * nq:]).all() and not np.isnan(L[:B * nq]).any()
