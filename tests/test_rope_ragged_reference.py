"""CPU: certifies the model of the ragged rotary append (tests/rope_ragged_ref.py), which the GPU tests compare bytes with.
(i) At a uniform q_b with cu[0] = 0 the model is rope_ref's uniform call, byte for byte, contiguous and paged, bf16 and e4m3.
(ii) With rot_dim = 0 it is kv_append_ref.append / append_paged, and its Q_out the source bits.
(iii) Five mutants -- models that differ from the contract in one word -- each change bytes on the GPU tests' OWN inputs, so a
kernel that made that mistake could not pass them."""
import pytest
import torch

import kv_append_ref as ar
import rope_ragged_ref as gr
import rope_ref as rr

E4M3 = ar.E4M3
KD, VD = torch.tensor((0.3, 0.7)), torch.tensor((1.3, 0.9))


def _caches(B, d, fp8, paged, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (gr.N_PAGES, gr.HKV, gr.PAGE, d) if paged else (B, gr.HKV, gr.CAP, d)
    mk = lambda: torch.randint(0, 0x78, shape, generator=g, dtype=torch.uint8).view(E4M3) if fp8 else \
        (torch.rand(shape, generator=g) - 0.5).bfloat16()
    return mk(), mk()


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("interleaved", (False, True), ids=("half", "pairs"))
def test_uniform_q_equals_the_uniform_model(interleaved, paged, fp8):
    B, n, d, rot = 4, 7, 64, 32
    lens = [n, 40, 3, gr.CAP + 2]                       # dropped leading tokens, dropped trailing tokens
    cu = [n * b for b in range(B + 1)]
    x = gr.source(d, 100)
    q, kn, vn = gr.views(x)
    cos, sin = rr.random_tables(gr.CAP, rot, 101)
    table = gr.table_for(cu, lens, 102) if paged else None
    kd, vd = (KD, VD) if fp8 else (None, None)
    K1, V1 = _caches(B, d, fp8, paged, 103)
    K2, V2 = K1.clone(), V1.clone()
    got, _ = gr.ragged_append(q, kn, vn, K1, V1, table, cos, sin, cu, lens, interleaved, kd, vd)
    u = lambda t: t.reshape(B, n, -1, d).permute(0, 2, 1, 3)      # the uniform call's [B, H, n_new, d] views of the same tokens
    if paged:
        want, written = rr.rope_append_paged(u(q), u(kn), u(vn), K2, V2, table, cos, sin, lens, interleaved, kd, vd)
    else:
        want, written = rr.rope_append(u(q), u(kn), u(vn), K2, V2, cos, sin, lens, interleaved, kd, vd)
    assert 0 < len(written) < B * n
    assert torch.equal(_bytes(K1), _bytes(K2)) and torch.equal(_bytes(V1), _bytes(V2))
    assert torch.equal(_bytes(got), _bytes(want.permute(0, 2, 1, 3).reshape(B * n, -1, d)))
    assert not torch.equal(_bytes(K1), _bytes(_caches(B, d, fp8, paged, 103)[0]))


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "e4m3"))
@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
def test_without_rotation_it_is_the_plain_append(paged, fp8):
    d = 64
    case = gr.PLACEMENT
    cu, lens = case["cu"], case["lens"]
    B = len(lens)
    x = gr.source(d, 110)
    q, kn, vn = gr.views(x)
    table = gr.table_for(cu, lens, 111) if paged else None
    kd, vd = (KD, VD) if fp8 else (None, None)
    K1, V1 = _caches(B, d, fp8, paged, 112)
    K2, V2 = K1.clone(), V1.clone()
    q_out, _ = gr.ragged_append(q, kn, vn, K1, V1, table, None, None, cu, lens, False, kd, vd)
    n_written = 0
    for b in range(B):
        s, n = cu[b], cu[b + 1] - cu[b]
        if n:
            kb, vb = (t[s:s + n].permute(1, 0, 2)[None] for t in (kn, vn))
            if paged:
                n_written += len(ar.append_paged(kb, vb, K2, V2, table[b:b + 1], [lens[b]], kd, vd))
            else:
                n_written += len(ar.append(kb, vb, K2[b:b + 1], V2[b:b + 1], [lens[b]], kd, vd))
    assert n_written == 25
    assert torch.equal(_bytes(K1), _bytes(K2)) and torch.equal(_bytes(V1), _bytes(V2))
    want = torch.zeros_like(q)
    want[1:26] = q[1:26]                                   # every owned token has a row here; tokens 0, 26, 27 are un-owned
    assert torch.equal(_bytes(q_out), _bytes(want))


def _model(case, d, paged, mutant, seed=120):
    cu, lens = case["cu"], case["lens"]
    x = gr.source(d, seed)
    q, kn, vn = gr.views(x)
    cos, sin = rr.random_tables(gr.CAP, d // 2, seed + 1)
    table = gr.table_for(cu, lens, seed + 2) if paged else None
    K, V = _caches(len(lens), d, False, paged, seed + 3)
    before = torch.full(q.shape, 1.5, dtype=torch.bfloat16)      # what Q_out held before the call
    q_out, _ = gr.ragged_append(q, kn, vn, K, V, table, cos, sin, cu, lens, False, mutant=mutant, Q_out=before)
    return torch.cat([_bytes(t).flatten() for t in (K, V, q_out)])


# the GPU test's input on which each mutant must show
WHERE = {"start_off_by_one": gr.PLACEMENT, "neighbours_q": gr.PLACEMENT, "position_from_T": gr.PLACEMENT,
         "unowned_unwritten": gr.PLACEMENT, "raw_cu": gr.HOSTILE}


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_every_mutant_changes_bytes_on_the_gpu_tests_inputs(mutant, paged):
    assert set(WHERE) == set(gr.MUTANTS) and len(gr.MUTANTS) >= 5
    for d in (64, 128):
        assert not torch.equal(_model(WHERE[mutant], d, paged, None), _model(WHERE[mutant], d, paged, mutant)), (mutant, d)


def test_the_inputs_are_what_the_gpu_tests_say():
    own = gr.owners(gr.PLACEMENT["cu"], gr.T)
    assert [o and o[0] for o in own] == [None, 1] + [2] * 19 + [3] * 5 + [None, None]
    assert len({o and o[0] for o in own[:8]}) == 3                       # one 8-token group: an un-owned token and two sequences
    pos = lambda case: [None if o is None else ar.position(case["lens"][o[0]], o[2], o[1], gr.CAP) for o in gr.owners(case["cu"], gr.T)]
    assert pos(gr.PLACEMENT) == [None, 0] + list(range(31, 50)) + list(range(91, 96)) + [None, None]
    assert pos(gr.DROPS) == [None, None] + [None] * 9 + list(range(0, 10)) + [94, 95, None, None, None] + [None, None]
    import extend_ragged_ref as xr
    assert xr.sanitised(gr.HOSTILE["cu"], gr.T) == [(5, 0), (5, 23), (28, 0), (28, 0)]
    many = gr.owners(gr.MANY["cu"], gr.T)
    assert len(gr.MANY["lens"]) == 37 and sorted({o[0] for o in many if o}) == sorted(gr.MANY_Q)
    assert [o is None for o in many] == [True, True] + [False] * 23 + [True] * 3
