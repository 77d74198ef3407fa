"""CPU: the torch model of the KV-cache append (tests/kv_append_ref.py) is what the contract says.
(i) Appending step by step into an empty cache, contiguous or paged, and gathering gives back the concatenation of what was
appended (decode_paged_ref.gather is the inverse the decode tests already use).
(ii) Its quantiser is decode_fp8kv_ref.quantise's expression, bit for bit, and has the byte table of the contract.
(iii) Drops: tokens outside [0, capacity) and tokens behind an out-of-pool table entry change nothing, and do not stop the rest."""
import pytest
import torch

import decode_fp8kv_ref as fr
import decode_paged_ref as pr
import kv_append_ref as ar

B, H, D = 3, 2, 64


def _new(n_new, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, H, n_new, D, generator=g) - 0.5).bfloat16() for _ in range(2)]


@pytest.mark.parametrize("fp8", (False, True))
def test_steps_into_an_empty_cache_concatenate(fp8):
    cap, dt = 96, (ar.E4M3 if fp8 else torch.bfloat16)
    kd, vd = (torch.tensor([0.3, 0.7]), torch.tensor([1.3, 0.9])) if fp8 else (None, None)
    K = torch.zeros(B, H, cap, D, dtype=torch.bfloat16).to(dt)
    V = K.clone()
    lens, ks, vs = [0] * B, [], []
    for step, n_new in enumerate((5, 1, 3, 1)):
        kn, vn = _new(n_new, 100 + step)
        lens = [n + n_new for n in lens]
        ar.append(kn, vn, K, V, lens, kd, vd)
        ks.append(kn)
        vs.append(vn)
    n = lens[0]
    for cache, parts, ds in ((K, ks, kd), (V, vs, vd)):
        want = torch.cat(parts, dim=2)
        want = ar.quantise(want, ds).view(torch.uint8) if fp8 else want.view(torch.int16)
        assert torch.equal(ar._bits(cache)[:, :, :n], want)
        assert not ar._bits(cache)[:, :, n:].any()


@pytest.mark.parametrize("P", (32, 96))
def test_paged_steps_gather_back_to_the_concatenation(P):
    max_pages, n_pages = 3, 11
    perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(P))
    table = perm[:B * max_pages].view(B, max_pages).int()
    Kp = torch.zeros(n_pages, H, P, D, dtype=torch.bfloat16)
    Vp = Kp.clone()
    lens, ks = [0, 30, 2 * P - 1], []
    first = list(lens)
    for step, n_new in enumerate((3, 1, 2)):
        kn, vn = _new(n_new, 200 + step)
        lens = [n + n_new for n in lens]
        ar.append_paged(kn, vn, Kp, Vp, table, lens)
        ks.append(kn)
    got = pr.gather(Kp, table, lens, P)
    want = torch.cat(ks, dim=2)
    for b in range(B):
        assert torch.equal(got[b, :, first[b]:lens[b]].view(torch.int16), want[b].view(torch.int16))
        assert not got[b, :, :first[b]].view(torch.int16).any() and not got[b, :, lens[b]:].view(torch.int16).any()


def test_quantiser_is_the_decode_tests_expression():
    g = torch.Generator().manual_seed(5)
    X = ((torch.rand(2, 3, 40, D, generator=g) - 0.5) * 7).bfloat16()
    X8, descale = fr.quantise(X, headroom=0.25)
    assert torch.equal(ar.quantise(X, descale).view(torch.uint8), X8.view(torch.uint8))
    assert torch.equal(ar.quantise(X).view(torch.uint8), X.float().clamp(-448, 448).to(ar.E4M3).view(torch.uint8))


def test_byte_table():
    for x, byte in ar.BYTE_TABLE:
        got = int(ar.quantise(torch.tensor([[[[x]]]], dtype=torch.float32)).view(torch.uint8))
        assert (got in ar.NAN_CODES) if byte is None else got == byte, (x, got, byte)


def test_special_values_survive_bf16():
    """The values the GPU test feeds are what the table names: bf16 holds +-inf, NaN, -0.0 and the ties exactly."""
    v = ar.special_values()
    assert torch.isnan(v).sum() == 1 and torch.isinf(v).sum() == 2       # (+-3e38 stay finite in bf16)
    assert (v.view(torch.int16) == -32768).sum() == 1                   # -0.0
    q = ar.quantise(v.view(1, 1, 1, -1)).view(torch.uint8).flatten().tolist()
    assert q[0] == 126 and q[1] == 254 and q[2] == 126 and q[3] == 254 and q[4] in ar.NAN_CODES


@pytest.mark.parametrize("length, rows", ((1, {2: 0}), (98, {0: 95}), (0, {}), (-5, {}), (ar.INT_MAX, {}), (ar.INT_MIN, {}), (96, {0: 93, 1: 94, 2: 95})))
def test_drops(length, rows):
    """n_new = 3 against a capacity of 96: which token lands where (token -> row); everything else is untouched."""
    cap = 96
    kn, vn = _new(3, 7)
    K = torch.full((B, H, cap, D), 3.0, dtype=torch.bfloat16)
    V = K.clone()
    before = K.clone()
    written = ar.append(kn, vn, K, V, [length] * B)
    assert sorted({(t, pos) for _, t, pos in written}) == sorted(rows.items())
    keep = torch.ones(cap, dtype=torch.bool)
    for t, pos in rows.items():
        keep[pos] = False
        assert torch.equal(K[:, :, pos].view(torch.int16), kn[:, :, t].view(torch.int16))
        assert torch.equal(V[:, :, pos].view(torch.int16), vn[:, :, t].view(torch.int16))
    assert torch.equal(K[:, :, keep], before[:, :, keep]) and torch.equal(V[:, :, keep], before[:, :, keep])


@pytest.mark.parametrize("bad", (-1, 8, ar.INT_MAX, ar.INT_MIN))
def test_a_bad_table_entry_drops_its_tokens_only(bad):
    P, max_pages, n_pages = 32, 3, 8
    table = torch.tensor([[0, 1, 2], [3, bad, 5], [6, 7, 4]], dtype=torch.int32)
    kn, vn = _new(3, 9)
    Kp = torch.zeros(n_pages, H, P, D, dtype=torch.bfloat16)
    Vp = Kp.clone()
    written = ar.append_paged(kn, vn, Kp, Vp, table, [34, 34, 34])      # rows 31 (page 0), 32, 33 (page 1)
    assert sorted(written) == [(0, 0, 0, 31), (0, 1, 1, 0), (0, 2, 1, 1), (1, 0, 3, 31), (2, 0, 6, 31), (2, 1, 7, 0), (2, 2, 7, 1)]
    assert torch.equal(Kp[3, :, 31].view(torch.int16), kn[1, :, 0].view(torch.int16))
    used = {(p, r) for _, _, p, r in written}
    for p in range(n_pages):
        for r in range(P):
            if (p, r) not in used:
                assert not Kp[p, :, r].view(torch.int16).any() and not Vp[p, :, r].view(torch.int16).any()
