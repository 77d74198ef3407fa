"""CPU: tests/rope_ref.py, the model the rotary-embedding append's GPU tests compare against, certified on properties that do
not come from the model itself: in float64 with a real cos/sin table a rotation preserves every pair's norm and the score of a
rotated query against a rotated key depends only on the distance of their positions; the rotate-half form is HF's
x*cos + rotate_half(x)*sin with concatenated tables; a partial rot_dim leaves the tail's bits alone; position 0 of a table with
cos = 1, sin = 0 is the identity bit for bit; the Q_out rule and the hand-off to the append's model; and the witness search finds
elements whose bf16 result tells the contract's arithmetic from each of the two contracted (fused multiply-add) forms."""
import pytest
import torch

import kv_append_ref as ar
import rope_ref as rr

D = 128


def _x(*shape, seed=0, dtype=torch.float64):
    return ((torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5) * 6).to(dtype)


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "pairs"))
@pytest.mark.parametrize("rot", (128, 64, 16))
def test_a_real_rotation_preserves_pair_norms_and_scores_depend_on_distance(rot, interleaved):
    cos, sin = rr.real_tables(64, rot)
    q, k = _x(D, seed=1), _x(D, seed=2)
    half = rot // 2
    pairs = (lambda v: (v[0:rot:2], v[1:rot:2])) if interleaved else (lambda v: (v[:half], v[half:rot]))
    for m in (0, 1, 17, 63):
        y = rr.rotate(q, cos[m], sin[m], interleaved)
        (x1, x2), (y1, y2) = pairs(q), pairs(y)
        assert torch.allclose(x1 * x1 + x2 * x2, y1 * y1 + y2 * y2, rtol=1e-13, atol=0)
        assert torch.equal(y[rot:], q[rot:])
    score = lambda m, n: float(rr.rotate(q, cos[m], sin[m], interleaved) @ rr.rotate(k, cos[n], sin[n], interleaved))
    for dist in (0, 3, 20):
        ref = score(dist, 0)
        for n in (1, 9, 40):
            assert abs(score(n + dist, n) - ref) < 1e-11 * (1 + abs(ref)), (dist, n)
    assert abs(score(5, 0) - score(9, 0)) > 1e-3      # (and it does depend on the distance)


@pytest.mark.parametrize("rot", (128, 64, 16))
def test_rotate_half_is_hf_expression_with_concatenated_tables(rot):
    cos, sin = rr.real_tables(32, rot)
    x = _x(5, D, seed=3)
    pos = torch.tensor([0, 1, 7, 30, 31])
    c2, s2 = torch.cat([cos, cos], dim=1)[pos], torch.cat([sin, sin], dim=1)[pos]
    xr = x[:, :rot]
    rotate_half = torch.cat([-xr[:, rot // 2:], xr[:, :rot // 2]], dim=1)
    want = torch.cat([xr * c2 + rotate_half * s2, x[:, rot:]], dim=1)
    got = rr.rotate(x, cos[pos], sin[pos], False)
    assert torch.allclose(got, want, rtol=1e-15, atol=1e-15)
    # the two pair forms are one rotation under a permutation of the elements
    perm = torch.arange(rot).view(2, rot // 2).t().reshape(-1)                    # interleaved slot 2i, 2i+1 <- i, i + rot/2
    xi = torch.cat([x[:, :rot][:, perm], x[:, rot:]], dim=1)
    gi = rr.rotate(xi, cos[pos], sin[pos], True)
    assert torch.equal(gi[:, :rot], got[:, :rot][:, perm]) and torch.equal(gi[:, rot:], x[:, rot:])


@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "pairs"))
def test_partial_rot_dim_keeps_the_tails_bits_and_identity_is_exact(interleaved):
    x = _x(4, D, seed=4).bfloat16()
    x[0, 100], x[1, 101], x[2, 127] = float("nan"), float("inf"), -0.0
    cos, sin = rr.random_tables(8, 64, 5)
    y = rr.rotate_bf16(x, cos[3], sin[3], interleaved)
    assert torch.equal(y.view(torch.int16)[:, 64:], x.view(torch.int16)[:, 64:])
    assert not torch.equal(y.view(torch.int16)[:, :64], x.view(torch.int16)[:, :64])
    x = _x(4, D, seed=6).bfloat16()
    x[0, 0], x[0, 64], x[1, 1] = -0.0, 0.0, 2.0 ** -130      # signed zeros stay what x*1 - y*0 makes of them, subnormals are kept
    for rot in (128, 16):
        one, zero = torch.ones(1, rot // 2), torch.zeros(1, rot // 2)
        y = rr.rotate_bf16(x, one[0], zero[0], interleaved)
        assert torch.equal(y.float(), x.float()) and torch.equal(y.view(torch.int16)[:, rot:], x.view(torch.int16)[:, rot:])
        nz = x.float() != 0
        assert torch.equal(y.view(torch.int16)[nz], x.view(torch.int16)[nz])


def test_random_tables_hold_a_distinct_value_everywhere():
    cos, sin = rr.random_tables(96, 128, 7)
    assert cos.shape == sin.shape == (96, 64) and cos.dtype == torch.float32
    both = torch.cat([cos.flatten(), sin.flatten()])
    assert both.unique().numel() == both.numel() and (both.abs() < 1).all()
    again = rr.random_tables(96, 128, 7)
    assert torch.equal(again[0], cos) and torch.equal(again[1], sin)


def test_q_out_rule_and_the_hand_off_to_the_append():
    B, Hq, Hkv, n_new, cap, d = 3, 4, 2, 3, 96, 64
    g = torch.Generator().manual_seed(8)
    x = ((torch.rand(B, n_new, Hq + 2 * Hkv, d, generator=g) - 0.5) * 6).bfloat16()
    q, kn, vn = (t.permute(0, 2, 1, 3) for t in (x[:, :, :Hq], x[:, :, Hq:Hq + Hkv], x[:, :, Hq + Hkv:]))
    cos, sin = rr.random_tables(cap, 32, 9)
    lens = [1, cap + 2, 50]      # rows -2 -1 0 | 95 96 97 | 47 48 49
    K, V = torch.zeros(B, Hkv, cap, d, dtype=torch.bfloat16), torch.zeros(B, Hkv, cap, d, dtype=torch.bfloat16)
    q_out, written = rr.rope_append(q, kn, vn, K, V, cos, sin, lens, True)
    assert sorted(written) == [(0, 2, 0), (1, 0, 95), (2, 0, 47), (2, 1, 48), (2, 2, 49)]
    assert q_out.is_contiguous() and q_out.shape == (B, Hq, n_new, d)
    zero = q_out.view(torch.int16) == 0
    assert zero[0, :, :2].all() and zero[1, :, 1:].all() and not zero[0, :, 2].all() and not zero[2].all(dim=-1).any()
    assert torch.equal(q_out[2, 1, 1], rr.rotate_bf16(q[2, 1, 1], cos[48], sin[48], True))
    assert torch.equal(K[1, :, 95], rr.rotate_bf16(kn[1, :, 0], cos[95], sin[95], True))
    assert torch.equal(V[2, :, 49], vn[2, :, 2])                                  # V is never rotated
    assert torch.equal(K[2, 0, 47, 32:].view(torch.int16), kn[2, 0, 0, 32:].view(torch.int16))
    # paged: a bad entry drops K and V, not Q; an e4m3 pool holds the quantised ROUNDED bf16 rotation
    table = torch.tensor([[4, -1, -1], [-1, -1, 7], [-1, 8, -1]], dtype=torch.int32)      # sequence 2's page is outside a pool of 8
    Kp, Vp = (torch.zeros(8, Hkv, 32, d, dtype=torch.uint8).view(ar.E4M3) for _ in range(2))
    kd = torch.tensor([0.3, 0.7])
    q2, written = rr.rope_append_paged(q, kn, vn, Kp, Vp, table, cos, sin, lens, True, kd, None)
    assert sorted(written) == [(0, 2, 4, 0), (1, 0, 7, 31)] and torch.equal(q2.view(torch.int16), q_out.view(torch.int16))
    want = ar.quantise(rr.rotate_bf16(kn[1, :, 0], cos[95], sin[95], True)[None, :, None], kd)[0, :, 0]
    assert torch.equal(Kp[7, :, 31].view(torch.uint8), want.view(torch.uint8))
    assert rr.rope_append(None, kn, vn, K, V, cos, sin, lens)[0] is None


def test_the_witness_search_finds_both_contracted_forms():
    w = rr.witnesses()
    for form in ("fma_first", "fma_second"):
        x1, x2, c, s = w[form]
        assert x1.numel() >= 32, (form, x1.numel())
        assert x1.dtype == torch.bfloat16 and c.dtype == torch.float32
        assert (x1.float().abs() <= 3).all() and (c.abs() <= 1).all() and (s.abs() <= 1).all()
        # through the model itself: a one-pair rotation of each witness is the contract's value, not the contracted one
        x = torch.stack([x1, x2], dim=1)
        got = rr.rotate_bf16(x, c[:, None], s[:, None], False)[:, 0]
        a, b = x1.float() * c, x2.float() * s
        fused = ((x1.double() * c.double() - b.double()) if form == "fma_first" else (a.double() - x2.double() * s.double())).float().bfloat16()
        assert torch.equal(got, (a - b).bfloat16()) and (got.view(torch.int16) != fused.view(torch.int16)).all()
    print({k: v[0].numel() for k, v in w.items()})
