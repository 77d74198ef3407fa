"""CPU: what tests/test_gpu_decode_paged.py rests on (tests/decode_paged_ref.py), without a GPU: the pools and tables build() makes
stand for the caches they were made from (gather() is build()'s inverse on the rows in use, and what is not in use is NaN in the
pool and out of range in the table), and the emulation of the kernels' data flow (decode_ref.emulate) on the GATHERED caches of
the page-edge batch meets decode_ref's gates at every page size and split count the GPU test uses -- so a GPU result outside the
gates is the kernel's doing, not the reference's."""
import numpy as np
import pytest
import torch

import decode_paged_ref as pr
import decode_ref as dr


@pytest.mark.parametrize("P", pr.PAGE_SIZES)
def test_gather_rebuilds_the_cache_on_the_rows_in_use(P):
    for i in pr.BIT_CASES:
        c = dr.CASES[i]
        _, K, V, _, _, _ = dr.inputs(i)
        Kp, Vp, table, lens, cap = pr.paged_inputs(i, P)
        B, max_pages = table.shape
        assert cap == max_pages * P >= c["ncap"] and Kp.shape == (B * max_pages + pr.SPARE_PAGES, c["hkv"], P, c["d"])
        for pool, t in ((Kp, K), (Vp, V)):
            got = pr.gather(pool, table, lens, P)
            assert got.shape == (B, c["hkv"], cap, c["d"])
            for b, n in enumerate(c["lens"]):      # (with seqlens_k = None the rows past the case's cache are new data)
                assert torch.equal(got[b, :, :n].view(torch.int16), t[b, :, :n].view(torch.int16)), (i, P, b)
            for b, n in enumerate(lens):
                assert not torch.isnan(got[b, :, :n].float()).any() and torch.isnan(got[b, :, n:pr.pages_for(n, P) * P].float()).all()
        used = [int(table[b, p]) for b, n in enumerate(lens) for p in range(pr.pages_for(n, P))]
        assert len(set(used)) == len(used) and all(0 <= u < Kp.shape[0] for u in used)      # a permutation: no page twice
        spare = sorted(set(range(Kp.shape[0])) - set(used))
        assert len(spare) >= pr.SPARE_PAGES and torch.isnan(Kp[spare].float()).all() and torch.isnan(Vp[spare].float()).all()
        unused = [int(table[b, p]) for b, n in enumerate(lens) for p in range(pr.pages_for(n, P), max_pages)]
        assert all(u in pr.UNUSED for u in unused)
        if c["seqlens"] and min(c["lens"]) < cap - P:
            assert set(unused) == set(pr.UNUSED)


def test_garbage_variants_share_the_table_and_the_rows_in_use():
    i, P = pr.GARBAGE_CASES[0], 96
    base = pr.paged_inputs(i, P)
    for fill in ("3e38", "zero"):
        other = pr.paged_inputs(i, P, fill)
        assert torch.equal(other[2], base[2])
        same = ~torch.isnan(base[0].float())
        filled = torch.tensor(pr.FILLS[fill]).bfloat16()      # (3e38 rounds to 3.004e38 in bf16)
        assert torch.equal(other[0][same], base[0][same]) and (other[0][~same] == filled).all()
    zeroed = pr.paged_inputs(i, P, "nan", True)
    used = (base[2] >= 0) & (base[2] < base[0].shape[0])
    assert torch.equal(zeroed[2][used], base[2][used]) and (zeroed[2][~used] == 0).all() and (~used).any()


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("P", pr.PAGE_SIZES)
def test_emulation_on_the_gathered_edge_batch_meets_the_gates(P, d):
    c = pr.edge_case(P, d)
    Q, Kp, Vp, table, scale, lens, sink = pr.edge_inputs(P, d)
    assert table.shape == (len(c["lens"]), c["ncap"] // P) and tuple(lens.tolist()) == pr.edge_lens(P)
    K, V = pr.edge_gathered(P, d)
    assert K.shape[2] == c["ncap"]
    ref = pr.edge_reference(P, d)
    for n_splits in sorted({dr.resolved_splits(c, s) for s in pr.SPLITS}):
        O, L = dr.emulate(Q, K, V, lens.tolist(), scale, True, sink, n_splits)
        e = dr.errors(O, L, ref)
        print(f"P {P} d {d} splits {n_splits}: O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e} rows {e[3]}")
        assert dr.within_gates(e), (P, d, n_splits, e)
        assert (O[6] == 0).all() and (sink is not None or np.isneginf(L[6]).all())      # the sequence without a key
