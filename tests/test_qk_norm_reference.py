"""CPU: certifies the model of the ragged rotary append with a per-head QK RMSNorm (tests/qk_norm_ref.py), which the GPU tests
compare bytes with.
(i) The model is an RMSNorm.  Against x / sqrt(mean(x^2) + eps) * w in float64, on the GPU tests' own sources, every element n
lies within (1 + 2^-6) HALF A bf16 ULP of the exact value e: |n - e| <= (1 + 2^-6) 2^(floor(log2 |e|) - 8).  Half an ulp is the one
rounding to bf16; the fp32 chain in front of it adds less than (d + 5) 2^-24 |e| < 2^-16 |e|, which the factor 1 + 2^-6 covers
(2^-6 of half an ulp is at least 2^-15 |e|).  Relative to |e| half an ulp runs from 2^-9 |e| (e just below a power of two) to
2^-8 |e| (e at one): a bound of 2^-9 (1 + 2^-6) |e| for EVERY element, as the feature's description words it, is met by no
rounding to bf16, the correctly rounded exact value included -- measured here, the largest |n - e| / |e| is 1.99 x 2^-9 -- so the
test bounds the error by half an ulp of e itself, which is 2^-9 (1 + 2^-6) |e| exactly where the description's figure can hold.
(ii) The butterfly gives every lane of a row identical bits, at d = 64 and d = 128, and the pinned order matters: a sequential sum
differs in fp32 on a large share of rows.
(iii) With weights of one and tables of zero columns the model is the sibling's model on the normalised tensors; V is untouched.
(iv) Eight mutants -- models that differ from the contract in one word -- each change bytes on the GPU tests' OWN inputs.
(v) The witness search: over 2^15 seeded rows per (d, kind of head) it finds rows whose bf16 result tells the contract from
sequential_sum, contracted_scale and weight_before_r, and NONE for contracted_squares (a bf16 square is exact in fp32), which is
therefore not among qk_norm_ref.WITNESS_FORMS."""
import numpy as np
import pytest
import torch

import kv_append_ref as ar
import qk_norm_ref as qk
import rope_ragged_ref as gr
import rope_ref as rr

SEED = 4000                                     # tests/test_gpu_qk_norm.py: case 1 runs on qk.source(d, SEED + d + rot)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("d", (64, 128))
def test_the_model_is_an_rmsnorm(d):
    qw, kw = qk.weights(d, qk.WEIGHT_SEED)
    worst = 0.0
    for rot in (d, d // 2, 0):
        x = qk.source(d, SEED + d + rot)
        for rows, w in ((x[:, :gr.HQ], qw), (x[:, gr.HQ:gr.HQ + gr.HKV], kw)):
            n = qk.rms_rows(rows, w, qk.EPS).double()
            xd = rows.double()
            exact = xd / torch.sqrt((xd * xd).mean(dim=-1, keepdim=True) + float(np.float32(qk.EPS))) * w.double()
            half_ulp = torch.where(exact == 0, torch.zeros_like(exact), torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(1e-300))) - 8))
            err = (n - exact).abs()
            assert (err <= (1 + 2.0 ** -6) * half_ulp).all(), (d, rot, float((err / half_ulp.clamp_min(1e-300)).max()))
            assert (n[exact == 0] == 0).all()
            worst = max(worst, float((err / exact.abs().clamp_min(1e-300)).max()))
    print(f"d = {d}: the largest |n - e| / |e| is {worst * 2 ** 9:.3f} x 2^-9")
    assert worst < 2.0 ** -8 * (1 + 2.0 ** -6)


@pytest.mark.parametrize("d", (64, 128))
def test_the_butterfly_gives_every_lane_the_same_bits(d):
    g = torch.Generator().manual_seed(41 + d)
    xf = ((torch.rand(4096, d, generator=g) - 0.5) * 6).bfloat16().float().numpy()
    s = qk.butterfly(qk.lane_sums(xf))
    assert s.shape == (4096, d // 8) and s.dtype == np.float32
    assert (s.view(np.int32) == s[:, :1].view(np.int32)).all()
    # the order is part of the contract: one chain over the d squares gives other fp32 bits on a large share of rows
    q = xf * xf
    chain = q[:, 0]
    for k in range(1, d):
        chain = chain + q[:, k]
    share = float((chain.view(np.int32) != s[:, 0].view(np.int32)).mean())
    assert share > 0.25, share
    # and both are sums of the same squares
    assert np.allclose(chain, s[:, 0], rtol=1e-5, atol=0)


def _caches(B, d, fp8, paged, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (gr.N_PAGES, gr.HKV, gr.PAGE, d) if paged else (B, gr.HKV, gr.CAP, d)
    mk = lambda: torch.randint(0, 0x78, shape, generator=g, dtype=torch.uint8).view(ar.E4M3) if fp8 else \
        (torch.rand(shape, generator=g) - 0.5).bfloat16()
    return mk(), mk()


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_it_is_the_sibling_on_the_normalised_tensors(paged, fp8):
    d, rot, case = 64, 32, gr.PLACEMENT
    cu, lens = case["cu"], case["lens"]
    x = qk.source(d, 210)
    q, kn, vn = gr.views(x)
    qw, kw = qk.weights(d, qk.WEIGHT_SEED)
    cos, sin = rr.random_tables(gr.CAP, rot, 211)
    table = gr.table_for(cu, lens, 212) if paged else None
    kd, vd = (torch.tensor((0.3, 0.7)), torch.tensor((1.3, 0.9))) if fp8 else (None, None)
    K1, V1 = _caches(len(lens), d, fp8, paged, 213)
    K2, V2 = K1.clone(), V1.clone()
    got, w1 = qk.ragged_append(q, kn, vn, K1, V1, table, cos, sin, qw, kw, qk.EPS, cu, lens, True, kd, vd)
    want, w2 = gr.ragged_append(qk.rms_rows(q, qw, qk.EPS), qk.rms_rows(kn, kw, qk.EPS), vn, K2, V2, table, cos, sin, cu, lens, True, kd, vd)
    assert w1 == w2 and sum(len(w) for w in w1) == 25
    assert torch.equal(_bytes(K1), _bytes(K2)) and torch.equal(_bytes(V1), _bytes(V2)) and torch.equal(_bytes(got), _bytes(want))
    # without a rotation Q_out holds n itself; the all-zero token's signed zeros follow the signs of x and w
    K3, V3 = K2.clone(), V2.clone()
    plain, _ = qk.ragged_append(q, kn, vn, K3, V3, table, None, None, qw, kw, qk.EPS, cu, lens, False, kd, vd)
    n = qk.rms_rows(q, qw, qk.EPS)
    assert torch.equal(_bytes(plain[1:26]), _bytes(n[1:26])) and not _bytes(plain[0]).any() and not _bytes(plain[26:]).any()
    zero = plain[qk.ZERO_TOKEN].view(torch.int16)
    assert set(zero.flatten().tolist()) == {0, -0x8000}
    sign = (q[qk.ZERO_TOKEN].view(torch.int16) < 0) ^ (qw < 0)[None, :]
    assert torch.equal(zero < 0, sign)
    # V is the sibling's V: the plain append's
    K4, V4 = _caches(len(lens), d, fp8, paged, 213)
    gr.ragged_append(None, kn, vn, K4, V4, table, None, None, cu, lens, False, kd, vd)
    assert torch.equal(_bytes(V3), _bytes(V4)) and not torch.equal(_bytes(K3), _bytes(K4))


def _model(where, d, paged, mutant):
    """K, V and Q_out bytes of the model (a mutant) on one of the GPU tests' inputs: "placement" -- case 1 at rot_dim = d / 2,
    rotate-half --, or "witness" -- case 3."""
    if where == "placement":
        case, rot = gr.PLACEMENT, d // 2
        x = qk.source(d, SEED + d + rot)
        cos, sin = rr.random_tables(gr.CAP, rot, SEED + d + rot + 5)
    else:
        case, rot = qk.WITNESS_CASE, 0
        x = qk.witness_source(d, SEED + 300 + d)
        cos = sin = None
    cu, lens = case["cu"], case["lens"]
    q, kn, vn = gr.views(x)
    qw, kw = qk.weights(d, qk.WEIGHT_SEED)
    table = gr.table_for(cu, lens, 7) if paged else None
    K, V = _caches(len(lens), d, False, paged, 8)
    q_out, _ = qk.ragged_append(q, kn, vn, K, V, table, cos, sin, qw, kw, qk.EPS, cu, lens, False, mutant=mutant)
    return torch.cat([_bytes(t).flatten() for t in (K, V, q_out)])


# the GPU test's input on which each mutant must show
WHERE = {"swapped_weights": "placement", "weight_column_off_by_8": "placement", "eps_outside_sqrt": "placement",
         "weight_before_r": "witness", "norm_after_rotation": "placement", "no_round_before_rotation": "placement",
         "v_normalised": "placement", "mean_over_rot_dim": "placement"}


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("mutant", qk.MUTANTS)
def test_every_mutant_changes_bytes_on_the_gpu_tests_inputs(mutant, paged):
    assert set(WHERE) == set(qk.MUTANTS) and len(qk.MUTANTS) == 8
    for d in (64, 128):
        assert not torch.equal(_model(WHERE[mutant], d, paged, None), _model(WHERE[mutant], d, paged, mutant)), (mutant, d)


@pytest.mark.parametrize("head", ("q", "k"))
@pytest.mark.parametrize("d", (64, 128))
def test_the_witness_search_finds_rows_for_every_witness_form(d, head):
    found = qk.witnesses(d, head)
    assert set(found) == set(qk.FORMS) and qk.WITNESS_ROWS == 1 << 15
    w = qk.weights(d, qk.WEIGHT_SEED)[("q", "k").index(head)]
    for form in qk.FORMS:
        rows = found[form]
        if form not in qk.WITNESS_FORMS:
            assert form == "contracted_squares" and rows.shape[0] == 0      # a bf16 square is exact in fp32
            continue
        assert rows.shape[0] > 0 and rows.shape[1] == d, (form, rows.shape)
        a, b = qk.rms_rows(rows, w, qk.EPS), qk.rms_rows(rows, w, qk.EPS, form=form)
        assert (a.view(torch.int16) != b.view(torch.int16)).any(dim=-1).all(), form


def test_the_witness_source_holds_every_form_in_every_kind_of_head():
    for d in (64, 128):
        x = qk.witness_source(d, SEED + 300 + d)
        q, kn, _ = gr.views(x)
        for rows, head in ((q, "q"), (kn, "k")):
            w = qk.weights(d, qk.WEIGHT_SEED)[("q", "k").index(head)]
            flat = rows.reshape(-1, d)
            want = qk.rms_rows(flat, w, qk.EPS).view(torch.int16)
            for form in qk.WITNESS_FORMS:
                other = qk.rms_rows(flat, w, qk.EPS, form=form).view(torch.int16)
                assert (want != other).any(dim=-1).sum() >= 5, (d, head, form)
