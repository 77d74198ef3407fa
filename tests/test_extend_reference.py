"""CPU: what tests/extend_ref.py provides, before tests/test_gpu_extend.py relies on it.
(i) Its float64 reference is decode_ref's (decode_window_ref's under a window) on cases with M <= 32: the extend cases add rows,
not another rule.
(ii) The model of the kernels' row blocks (block_tiles, the clip of extend_split_body in Python integers) drops no visible key: on
every case, variant, length and split count, every key some row of a block sees in a split lies in a tile the block processes,
each tile is processed once and by the wave the siblings give it (tile number counted from the split's first key, modulo 4), and a
block that takes the empty-split exit has no visible key in that split.
(iii) The cases are the ones the issue sets."""
import numpy as np
import pytest

import decode_ref as dr
import decode_window_ref as wr
import extend_ref as er


def test_cases_cover_the_shapes():
    assert {(c["hq"], c["hkv"], c["nq"]) for c in er.CASES} == set(er.SHAPES)
    assert sorted({er.rows_of(c) for c in er.CASES}) == [33, 40, 64, 65, 68, 70, 96, 160]
    assert {c["d"] for c in er.CASES} == {64, 128}
    for c in er.CASES:
        if c["seqlens"]:
            nq = c["nq"]
            assert c["lens"] == (0, 1, nq - 1, nq, 127, 128, 129, 300, 1100, 2500) and c["ncap"] == 2560
        assert c["splits"] == (0, 1, 2, 7, 64)
    assert any(not c["seqlens"] for c in er.CASES)
    assert er.WINDOWS == (0, 1, 31, 127, 128, 200, er.N_CAP - 1)
    assert {er.has_sink(i, k) for i, k in er.RUNS} == {False, True}
    for i in range(len(er.CASES)):      # every case meets a sink and its absence under the causal mask, a window and no mask
        assert {er.has_sink(i, k) for k in range(2, len(er.VARIANTS))} == {False, True}
    assert len(er.SLICED) == len(er.CASES) - 4


# two float64 evaluations of one O element that sum in different orders: at most n eps max|v| = 2560 x 1.1e-16 x 0.5 = 1.4e-13 apart
SUM_ORDER = 1e-12

DECODE = [i for i, c in enumerate(dr.CASES) if c["regime"] is None and c["seqlens"]][:6]


@pytest.mark.parametrize("i", DECODE, ids=[dr.case_id(dr.CASES[i]) for i in DECODE])
def test_reference_is_decode_refs_on_small_cases(i):
    c = dr.CASES[i]
    Q, K, V, scale, lens, sink = dr.inputs(i)
    O, L = er.reference64(Q, K, V, c["lens"], scale, c["causal"], sink, None)
    rO, rL = dr.reference(i)
    assert np.array_equal(O, rO) and np.array_equal(L, rL)


@pytest.mark.parametrize("i", [0, 7, wr.GPT_OSS], ids=lambda i: wr.IDS[i])
def test_reference_is_decode_window_refs_on_small_cases(i):
    c = wr.CASES[i]
    Q, K, V, scale, lens, sink = wr.inputs(i)
    O, L = er.reference64(Q, K, V, c["lens"], scale, True, sink, c["wl"])
    rO, rL = wr.reference(i)
    assert np.array_equal(O, rO) and np.array_equal(L, rL)
    if c["wl"] >= max(c["lens"]):      # a window that excludes no key is the plain reference
        pO, pL = er.reference64(Q, K, V, c["lens"], scale, True, sink, None)
        assert np.allclose(O, pO, rtol=0, atol=SUM_ORDER) and np.allclose(L, pL, rtol=1e-12)


def test_a_window_of_the_capacity_is_the_plain_reference():
    i = next(k for k, c in enumerate(er.CASES) if (c["hq"], c["hkv"], c["nq"], c["d"]) == (8, 1, 5, 64) and c["seqlens"])
    c = er.CASES[i]
    Q, K, V, scale, _, sink = er.inputs(i)
    a = er.reference64(Q, K, V, c["lens"], scale, True, sink, er.N_CAP - 1)
    b = er.reference64(Q, K, V, c["lens"], scale, True, sink, None)
    assert np.array_equal(np.isneginf(a[1]), np.isneginf(b[1]))
    assert np.allclose(a[0], b[0], rtol=0, atol=SUM_ORDER) and np.allclose(a[1], b[1], rtol=1e-12)


@pytest.mark.parametrize("i", range(len(er.CASES)), ids=er.IDS)
def test_the_row_block_clip_drops_no_visible_key(i):
    c = er.CASES[i]
    M, nq = er.rows_of(c), c["nq"]
    blocks = -(-M // er.ROWS)
    skipped = exits = 0
    for mask, wl in er.VARIANTS:
        causal = mask == "causal"
        for n in sorted(set(c["lens"])):
            for n_splits in (1, 2, 7, 64):
                for s in range(n_splits):
                    begin, end = er.split_range(n, nq, wl, n_splits, s)
                    for j in range(blocks):
                        rows = range(er.ROWS * j, min(er.ROWS * (j + 1), M))
                        seen = set()
                        for rho in rows:
                            kmin, kmax = er.row_window(rho, nq, n, causal, wl)
                            seen.update(range(max(kmin, begin), min(kmax, end)))
                        tiles = er.block_tiles(M, nq, n, causal, wl, n_splits, s, j)
                        if tiles is None:
                            assert not seen, (mask, wl, n, n_splits, s, j)
                            exits += 1
                            continue
                        flat = [kb for w in tiles for kb in tiles[w]]
                        assert len(flat) == len(set(flat))
                        for w, kbs in tiles.items():
                            assert kbs == sorted(kbs)
                            for kb in kbs:
                                assert begin <= kb < end and (kb - begin) % er.TILE == 0 and (kb - begin) // er.TILE % er.WAVES == w
                        covered = {kb // er.TILE for kb in flat}
                        assert {key // er.TILE for key in seen} <= covered, (mask, wl, n, n_splits, s, j)
                        skipped += len(range(begin, end, er.TILE)) - len(flat)
    assert exits > 0
    if c["seqlens"]:
        assert skipped > 0      # the clip does skip tiles on these cases
