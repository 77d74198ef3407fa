"""GPU: grouped-query attention (K, V, dK, dV of shape [B, H_kv, N, d]; query head h attends K/V head h // (H_q // H_kv)).

"Expanded" below = K and V repeat_interleave'd to H_q heads and run through the multi-head entry points; "oracle" =
oracle.attention_forward / attention_backward on the expanded fp32 copies, its dK / dV summed over each group on the host in
float64.  Gates: the project's bf16 ones (rel-L2 <= 5e-3 on O, dQ, dK, dV; max |dL| <= 1e-4).  A query head's arithmetic does
not depend on where its K/V live, so O, L and dQ are compared BIT FOR BIT with the expanded multi-head call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16_REL = 5e-3
L_ABS = 1e-4
PAIRS = ((8, 1), (8, 2), (16, 4), (14, 2), (6, 3), (5, 5))      # both branches of map_block, G = 7, multi-query, G = 1
SINGLE = ((128, 256), (128, 1536), (128, 2000), (64, 1024))     # (d, N) the routing rule gives to the single kernel


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _f(t):
    return t.float().cpu().numpy()


def _lib():
    import cuda_flashattention_amd as fa
    return fa._capi.lib()


def _plan(B, Hq, Hkv, N, d, causal):
    lib = _lib()
    none = ctypes.POINTER(ctypes.c_char_p)()
    got = lib.fa2_backward_gqa_plan(B, Hq, Hkv, N, d, 0, int(causal), none)
    assert got == lib.fa2_backward_plan(B, Hq, N, d, 0, int(causal), none), (B, Hq, Hkv, N, d, causal)
    return got


@functools.lru_cache(maxsize=None)
def _cases():
    """(B, H_q, H_kv, N, d, causal): every pair x head_dim twice with N drawn from 1..700 (causal on and off between them),
    N = 1024 and 2304 for a few pairs, and the single-kernel lengths."""
    rng = np.random.default_rng(31337)
    out = []
    for hq, hkv in PAIRS:
        for d in (64, 128):
            flip = bool(rng.integers(0, 2))
            for k in range(2):
                out.append((int(rng.integers(1, 3)), hq, hkv, int(rng.integers(1, 701)), d, flip ^ bool(k)))
    for (hq, hkv), d, N, causal, B in (((8, 2), 128, 1024, True, 2), ((14, 2), 64, 1024, False, 1), ((8, 1), 128, 2304, False, 1),
                                       ((6, 3), 64, 2304, True, 1), ((16, 4), 128, 1024, False, 1), ((6, 3), 128, 2304, True, 2)):
        out.append((B, hq, hkv, N, d, causal))
    for i, (d, N) in enumerate(SINGLE):
        hq, hkv = PAIRS[i % 4]
        out.append((1 + i % 2, hq, hkv, N, d, False))
        out.append((1, hq, hkv, N, d, True))
    return tuple(out)


def _inputs(i):
    B, Hq, Hkv, N, d, causal = _cases()[i]
    g = torch.Generator().manual_seed(7000 + i)
    mk = lambda h, s: ((torch.rand(B, h, N, d, generator=g) - 0.5) * s).bfloat16()
    return mk(Hq, 1.0), mk(Hkv, 1.0), mk(Hkv, 1.0), mk(Hq, 0.4)


def _expand(x, G):
    return x.repeat_interleave(G, dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def _oracle_case(i):
    """Oracle O, L, dQ and the group sums of dK, dV for case i (computed once, used by several tests)."""
    import oracle
    B, Hq, Hkv, N, d, causal = _cases()[i]
    Q, K, V, dO = _inputs(i)
    G = Hq // Hkv
    Ke, Ve = _f(_expand(K, G)), _f(_expand(V, G))
    s = 1.0 / d ** 0.5
    Or, Lr = oracle.attention_forward(_f(Q), Ke, Ve, s, causal=causal)
    dQr, dKr, dVr = oracle.attention_backward(_f(Q), Ke, Ve, _f(dO), s, causal=causal)
    gsum = lambda x: x.reshape(B, Hkv, G, N, d).astype(np.float64).sum(axis=2)
    return Or, Lr, dQr, gsum(dKr), gsum(dVr)


def _backward(Q, K, V, O, L, dO, s, causal, how):
    """how: 'rule' = phases 7, 'two' = D, then the two kernels whatever the shape (phases 1, then 6), 'single' = 8 | 1.
    Returns dQ, dK, dV and the workspace."""
    import cuda_flashattention_amd as fa
    B, Hq, N, d = Q.shape
    ws = torch.empty(_lib().fa2_backward_gqa_workspace_bytes(B, Hq, K.shape[1], N, d, 0), dtype=torch.uint8, device="cuda")
    out = None
    for ph in {"rule": (7,), "two": (1, 6), "single": (9,)}[how]:
        out = fa.flash_attention_2_backward(Q, K, V, O, L, dO, s, causal=causal, workspace=ws, phases=ph,
                                            **({} if out is None else dict(dQ=out[0], dK=out[1], dV=out[2])))
    return out + (ws,)


def _status(ws, B, Hq, N, d):
    """fa2_backward_status with the MULTI-HEAD arguments (B, H_q, N, d) on the workspace of a grouped launch."""
    return _lib().fa2_backward_status(ws.data_ptr(), ws.numel(), B, Hq, N, d, 0, torch.cuda.current_stream().cuda_stream)


def test_forward_is_bit_identical_to_the_expanded_call_and_meets_the_gates():
    import cuda_flashattention_amd as fa
    for i, (B, Hq, Hkv, N, d, causal) in enumerate(_cases()):
        tag = f"case {i}: B{B} Hq{Hq} Hkv{Hkv} N{N} d{d} causal={causal}"
        Q, K, V, _ = (t.cuda() for t in _inputs(i))
        s = 1.0 / d ** 0.5
        O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
        Oe, Le = fa.flash_attention_2_forward(Q, _expand(K, Hq // Hkv), _expand(V, Hq // Hkv), s, causal=causal)
        torch.cuda.synchronize()
        assert O.shape == Q.shape and L.shape == Q.shape[:-1], tag
        assert torch.isfinite(O.float()).all() and torch.isfinite(L).all(), tag
        assert torch.equal(O, Oe), tag
        assert torch.equal(L, Le), tag
        Or, Lr = _oracle_case(i)[:2]
        eo, el = _rel(_f(O), Or), float(np.abs(L.cpu().numpy() - Lr).max())
        print(f"{tag}: O {eo:.3e} L {el:.3e}")
        assert eo <= BF16_REL, (tag, eo)
        assert el <= L_ABS, (tag, el)


def test_backward_dq_bit_identical_and_dk_dv_within_the_gates_on_every_route():
    """Per case: the routing rule's choice (phases 7), the two kernels forced, and -- where the plan says 1 -- the single kernel
    forced (8 | 1).  dQ is bit-identical to the expanded multi-head backward on the same route; dK / dV meet the gates against
    the oracle's group sums; fa2_backward_status (multi-head arguments) says 0 after the single-kernel runs."""
    import cuda_flashattention_amd as fa
    for i, (B, Hq, Hkv, N, d, causal) in enumerate(_cases()):
        tag = f"case {i}: B{B} Hq{Hq} Hkv{Hkv} N{N} d{d} causal={causal}"
        G = Hq // Hkv
        Q, K, V, dO = (t.cuda() for t in _inputs(i))
        Ke, Ve = _expand(K, G), _expand(V, G)
        s = 1.0 / d ** 0.5
        O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
        plan = _plan(B, Hq, Hkv, N, d, causal)
        if (d, N) in SINGLE:
            assert plan == 1, tag
        _, _, dQr, dKr, dVr = _oracle_case(i)
        for how in ("rule", "two") + (("single",) if plan == 1 else ()):
            dQ, dK, dV, ws = _backward(Q, K, V, O, L, dO, s, causal, how)
            dQe = _backward(Q, Ke, Ve, O, L, dO, s, causal, how)[0]
            torch.cuda.synchronize()
            assert dK.shape == K.shape and dV.shape == V.shape, tag
            assert torch.equal(dQ, dQe), (tag, how)
            if how == "single" or (how == "rule" and plan == 1):
                assert _status(ws, B, Hq, N, d) == 0, (tag, how)
            errs = {}
            for name, got, ref in (("dQ", dQ, dQr), ("dK", dK, dKr), ("dV", dV, dVr)):
                assert np.isfinite(_f(got)).all(), (tag, how, name)
                errs[name] = _rel(_f(got), ref)
            print(f"{tag} {how}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
            for name, e in errs.items():
                assert e <= BF16_REL, (tag, how, name, e)


def _raw_gqa(Q, K, V, dO, Hkv, s, causal):
    """Forward and backward through fa2_forward_gqa / fa2_backward_gqa themselves (ops sends H_kv == H_q to the multi-head calls)."""
    lib = _lib()
    B, Hq, N, d = Q.shape
    st = torch.cuda.current_stream().cuda_stream
    O, L = torch.empty_like(Q), torch.empty(B, Hq, N, dtype=torch.float32, device="cuda")
    assert lib.fa2_forward_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), B, Hq, Hkv, N, d, s, 0,
                               int(causal), st) == 0
    need = lib.fa2_backward_gqa_workspace_bytes(B, Hq, Hkv, N, d, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    assert lib.fa2_backward_gqa(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), dO.data_ptr(), dQ.data_ptr(),
                                dK.data_ptr(), dV.data_ptr(), B, Hq, Hkv, N, d, s, 0, int(causal), ws.data_ptr(), need, st, 7) == 0
    return O, L, dQ, dK, dV


@pytest.mark.parametrize("N", [1024, 300])                # a single-kernel shape and a two-kernel shape
@pytest.mark.parametrize("causal", [False, True])
def test_equal_head_counts_through_the_gqa_entry_points(N, causal):
    import cuda_flashattention_amd as fa
    B, H, d = 2, 4, 128
    assert _plan(B, H, H, N, d, causal) == (1 if N == 1024 else 2)
    assert _lib().fa2_backward_gqa_workspace_bytes(B, H, H, N, d, 0) == _lib().fa2_backward_workspace_bytes(B, H, N, d, 0)
    g = torch.Generator().manual_seed(8100 + N + int(causal))
    mk = lambda sc: ((torch.rand(B, H, N, d, generator=g) - 0.5) * sc).bfloat16().cuda()
    Q, K, V, dO = mk(1.0), mk(1.0), mk(1.0), mk(0.4)
    s = 1.0 / d ** 0.5
    got = _raw_gqa(Q, K, V, dO, H, s, causal)
    O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
    want = (O, L) + tuple(fa.flash_attention_2_backward(Q, K, V, O, L, dO, s, causal=causal))
    torch.cuda.synchronize()
    for name, a, b in zip(("O", "L", "dQ", "dK", "dV"), got, want):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("d,N,how", [(128, 1536, "rule"), (64, 1024, "rule"), (128, 2000, "single"), (128, 1536, "two"), (64, 417, "rule")])
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_backward_is_deterministic(d, N, how, causal):
    import cuda_flashattention_amd as fa
    B, Hq, Hkv = 2, 14, 2
    assert _plan(B, Hq, Hkv, N, d, causal) == (2 if N == 417 else 1)
    g = torch.Generator().manual_seed(8200 + N + d)
    mk = lambda h, sc: ((torch.rand(B, h, N, d, generator=g) - 0.5) * sc).bfloat16().cuda()
    Q, K, V, dO = mk(Hq, 1.0), mk(Hkv, 1.0), mk(Hkv, 1.0), mk(Hq, 0.4)
    s = 1.0 / d ** 0.5
    O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
    first = _backward(Q, K, V, O, L, dO, s, causal, how)[:3]
    again = _backward(Q, K, V, O, L, dO, s, causal, how)[:3]
    torch.cuda.synchronize()
    for name, a, b in zip(("dQ", "dK", "dV"), first, again):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), name


def test_autograd_gives_gradients_of_the_tensors_shapes():
    import cuda_flashattention_amd as fa
    B, Hq, Hkv, N, d = 2, 8, 2, 640, 128
    g = torch.Generator().manual_seed(8300)
    mk = lambda h, sc: ((torch.rand(B, h, N, d, generator=g) - 0.5) * sc).bfloat16().cuda()
    Q, K, V, dO = mk(Hq, 1.0), mk(Hkv, 1.0), mk(Hkv, 1.0), mk(Hq, 0.4)
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = fa.attention(q, k, v, causal=True)
    out.backward(dO)
    s = 1.0 / d ** 0.5
    O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=True)
    dQ, dK, dV = fa.flash_attention_2_backward(Q, K, V, O, L, dO, s, causal=True)
    torch.cuda.synchronize()
    assert k.grad.shape == K.shape and v.grad.shape == V.shape and q.grad.shape == Q.shape
    assert torch.equal(out.detach(), O)
    for name, a, b in (("dQ", q.grad, dQ), ("dK", k.grad, dK), ("dV", v.grad, dV)):
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("causal", [False, True])
def test_gqa_backward_at_size_whole_group_vs_oracle(causal):
    """(1, 8 -> 2, 8192, 128) through the single kernel: dK / dV of K/V head 1 against the sum of the oracle's whole-head
    backward over the group's four query heads (4 .. 7), dQ of query head 5 against the same oracle calls -- the full 256-tile
    sweep, the per-query-head partials and their reduction at a length of the bench shape."""
    import cuda_flashattention_amd as fa
    import oracle
    B, Hq, Hkv, N, d = 1, 8, 2, 8192, 128
    G = Hq // Hkv
    assert _plan(B, Hq, Hkv, N, d, causal) == 1
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(321 + int(causal))
    mk = lambda h, sc: ((torch.rand(B, h, N, d, device=dev, generator=g) - 0.5) * sc).bfloat16()
    Q, K, V, dO = mk(Hq, 1.0), mk(Hkv, 1.0), mk(Hkv, 1.0), mk(Hq, 0.4)
    s = 1.0 / d ** 0.5
    O, L = fa.flash_attention_2_forward(Q, K, V, s, causal=causal)
    dQ, dK, dV, ws = _backward(Q, K, V, O, L, dO, s, causal, "rule")
    torch.cuda.synchronize()
    assert _status(ws, B, Hq, N, d) == 0
    kv = 1
    dKr, dVr = np.zeros((N, d), np.float64), np.zeros((N, d), np.float64)
    for h in range(kv * G, (kv + 1) * G):
        rq, rk, rv = oracle.attention_backward_head(_f(Q[0, h]), _f(K[0, kv]), _f(V[0, kv]), _f(dO[0, h]), s, causal=causal)
        dKr += rk
        dVr += rv
        if h == kv * G + 1:
            e = _rel(_f(dQ[0, h]), rq)
            print(f"causal={causal} dQ head {h}: {e:.3e}")
            assert e <= BF16_REL, ("dQ", e)
    for name, got, want in (("dK", dK[0, kv], dKr), ("dV", dV[0, kv], dVr)):
        assert np.isfinite(_f(got)).all(), name
        e = _rel(_f(got), want)
        print(f"causal={causal} {name} head {kv}: {e:.3e}")
        assert e <= BF16_REL, (name, e)
