"""CPU: what tests/decode_window_ref.py holds is what tests/test_gpu_decode_window.py may lean on.
(i) The emulation of the windowed kernels' data flow stays inside decode_ref's gates against the float64 reference on every case
of the GPU file, for every split count, bf16 and dequantised e4m3 caches (the worst figures are printed: DESIGN.md 3k).
(ii) The split ranges partition [rounddown(lo, 128), len), start on multiples of 128 and never hold more than window_left + N_q +
127 keys in total, for window_left in {0, 1, 31, 127, 128, 2^31 - 1} and every length 0..600.
(iii) A window at or above len - 1 is the unwindowed reference; split_partial with kmin = 0 is decode_ref._split_partial."""
import numpy as np
import pytest
import torch

import decode_paged_ref as pr
import decode_ref as dr
import decode_window_ref as wr

WORST = {}


@pytest.mark.parametrize("i", range(len(wr.CASES)), ids=wr.IDS)
def test_emulation_within_gates(i):
    c = wr.CASES[i]
    for fp8 in (False, True):
        Q, K, V, scale, lens, sink = wr.inputs(i)
        if fp8:
            K, V = wr.dequantised(i)
        ref = wr.reference(i, fp8)
        for n_splits in c["splits"]:
            s = wr.resolved_splits(c, n_splits)
            e = dr.errors(*wr.emulate(Q, K, V, lens.tolist(), scale, sink, c["wl"], s), ref)
            assert dr.within_gates(e), (wr.case_id(c), fp8, n_splits, e)
            w = WORST.setdefault(fp8, [0.0, 0.0, 0.0])
            w[:] = [max(a, b) for a, b in zip(w, e[:3])]
    print(wr.case_id(c), {k: [f"{x:.3e}" for x in v] for k, v in WORST.items()})


def test_reference_rows_without_a_key():
    """len < N_q rows: O = 0 and L = -inf, or the sink."""
    for i, c in enumerate(wr.CASES):
        if c["nq"] != 4 or c["wl"] not in (0, 127):
            continue
        O, L = wr.reference(i)
        sink = wr.inputs(i)[5]
        for b, n in enumerate(c["lens"]):
            for q in range(c["nq"]):
                if q + n - c["nq"] < 0:
                    assert (O[b, :, q] == 0).all()
                    want = np.full(c["hq"], -np.inf) if sink is None else sink.double().numpy()
                    assert np.array_equal(L[b, :, q], want)
                else:
                    assert np.isfinite(L[b, :, q]).all()


@pytest.mark.parametrize("wl", [0, 1, 31, 127, 128, wr.INT_MAX])
def test_split_ranges(wl):
    for nq in (1, 4):
        for n in range(601):
            lo = wr.lo_of(n, nq, wl)
            base = lo // wr.KB * wr.KB
            assert lo == max(0, n - nq - wl) and base <= lo <= n
            for n_splits in (1, 2, 3, 5, 64, 256):
                at, total = base, 0
                for s in range(n_splits):
                    begin, end = wr.window_range(n, nq, wl, n_splits, s)
                    assert begin % wr.KB == 0 and begin >= base
                    if begin < end:
                        assert begin == at      # no gap and no overlap: a partition in ascending order
                        at, total = end, total + end - begin
                assert at == (n if n > base else base) and total == n - base
                assert total <= min(wl + nq + wr.KB - 1, n)
                # every visible key of every row is covered, and the first range holds lo's tile
                if n:
                    assert wr.window_range(n, nq, wl, n_splits, 0)[0] <= lo


def test_window_at_or_above_the_length_is_no_window():
    i = next(k for k, c in enumerate(wr.CASES) if c["nq"] == 4 and c["sink"] and c["d"] == 64)
    c = wr.CASES[i]
    Q, K, V, scale, lens, sink = wr.inputs(i)
    plain = wr.reference64(Q, K, V, c["lens"], scale, sink, None)
    for wl in (wr.N_CAP - 1, wr.N_CAP, wr.INT_MAX):
        got = wr.reference64(Q, K, V, c["lens"], scale, sink, wl)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    # per sequence: len - 1 is enough, len - 2 is not (N_q = 4: row 3 of a sequence of n keys sits at n - 1)
    for b, n in enumerate(c["lens"]):
        if n >= 3:
            one = lambda wl: wr.reference64(Q[b:b + 1], K[b:b + 1], V[b:b + 1], [n], scale, sink, wl)
            assert np.array_equal(one(n - 1)[1], plain[1][b:b + 1])
            assert not np.array_equal(one(n - 2)[1], plain[1][b:b + 1])
    # and the plain float64 reference of decode_ref's own rule agrees with this module's, to rounding
    want = pr.reference64(Q, K, V, c["lens"], scale, True, sink)
    assert np.allclose(plain[0], want[0], rtol=0, atol=1e-12) and np.array_equal(np.isneginf(plain[1]), np.isneginf(want[1]))
    fin = np.isfinite(want[1])
    assert np.allclose(plain[1][fin], want[1][fin], rtol=0, atol=1e-12)


def test_split_partial_without_a_lower_bound_is_decode_refs():
    g = torch.Generator().manual_seed(5)
    hkv, M, d, n = 2, 8, 64, 300
    q = (torch.rand(hkv, M, d, generator=g) - 0.5).bfloat16().float().numpy()
    k, v = ((torch.rand(hkv, n, d, generator=g) - 0.5).bfloat16().float().numpy() for _ in range(2))
    kmax = np.arange(M) % 4 + n - 3
    sc = np.float32(0.125) * dr._LOG2E
    for begin, end in ((0, 300), (128, 300), (256, 290)):
        want = dr._split_partial(q, k, v, np.minimum(kmax, end), begin, end, sc)
        got = wr.split_partial(q, k, v, np.zeros(M, dtype=np.int64), np.minimum(kmax, end), begin, end, sc)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_the_emulation_with_a_wide_window_is_decode_refs():
    i = 0
    c = wr.CASES[i]
    Q, K, V, scale, lens, sink = wr.inputs(i)
    for n_splits in (1, 2, 5):
        want = dr.emulate(Q, K, V, lens.tolist(), scale, True, sink, n_splits)
        got = wr.emulate(Q, K, V, lens.tolist(), scale, sink, wr.INT_MAX, n_splits)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
