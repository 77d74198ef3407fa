"""CPU: what tests/test_gpu_decode.py rests on (tests/decode_ref.py) and everything of the decode call that needs no GPU.

(i) The emulation of the kernels' data flow against the float64 reference on every case and split count the GPU file runs: the
inputs leave the kernels room under the gates.  test_worst_emulation_figures prints the worst figures over all cases (quoted in
DESIGN.md section 3g).
(ii) fa2_forward_decode's status codes, in the documented order, with pointers that are never dereferenced.
(iii) fa2_decode_num_splits and fa2_decode_workspace_bytes on fixed examples.
(iv) Every ValueError of cuda_flashattention_amd.flash_attention_2_decode, on CPU tensors and wrong shapes."""
import ctypes

import numpy as np
import pytest
import torch

import decode_ref as dr

WORST = {}


def _lib():
    from cuda_flashattention_amd import _capi
    return _capi.lib()


# ------------------------------------------------------------------------------------------------ (i)
@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=[dr.case_id(c) for c in dr.CASES])
def test_emulation_is_within_the_gates(i):
    c = dr.CASES[i]
    Q, K, V, scale, lens, sink = dr.inputs(i)
    ref = dr.reference(i)
    for n_splits in c["splits"]:
        ns = dr.resolved_splits(c, n_splits)
        O, L = dr.emulate(Q, K, V, lens, scale, c["causal"], sink, ns)
        e = dr.errors(O, L, ref)
        print(dr.case_id(c), f"splits {n_splits} -> {ns}: O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e}")
        assert dr.within_gates(e), (dr.case_id(c), n_splits, e)
        for k, v in zip(("O", "L", "L_large"), e):
            WORST[k] = max(WORST.get(k, 0.0), v)


def test_worst_emulation_figures():
    """Over the cases above that ran before this test: the figures DESIGN.md section 3g quotes (run the whole file with -s)."""
    print("worst emulation figures:", WORST)
    assert all(v <= g for v, g in ((WORST.get("O", 0.0), dr.BF16_REL), (WORST.get("L", 0.0), dr.L_ABS), (WORST.get("L_large", 0.0), dr.L_ABS_LARGE)))


def test_reference_rows_without_a_key():
    """The cases do hold rows without a key, and with a sink those rows have L = sink."""
    seen_plain = seen_sink = False
    for i, c in enumerate(dr.CASES):
        _, L = dr.reference(i)
        sink = dr.inputs(i)[5]
        for b, n in enumerate(c["lens"]):
            keyless = np.array([n == 0 or (c["causal"] and q + n - c["nq"] < 0) for q in range(c["nq"])])
            if not keyless.any():
                continue
            if sink is None:
                assert np.isneginf(L[b][:, keyless]).all() and np.isfinite(L[b][:, ~keyless]).all()
                seen_plain = True
            else:
                np.testing.assert_array_equal(L[b][:, keyless], np.broadcast_to(sink.double().numpy()[:, None], L[b].shape)[:, keyless])
                seen_sink = True
    assert seen_plain and seen_sink


def test_split_rule():
    assert dr.split_range(2500, 7, 0) == (0, 384) and dr.split_range(2500, 7, 6) == (2304, 2500)
    assert dr.split_range(129, 64, 1) == (128, 129) and dr.split_range(129, 64, 2)[0] >= 129      # later splits are empty
    assert dr.split_range(0, 2, 0) == (0, 0)


# ------------------------------------------------------------------------------------------------ (ii)
def test_status_codes_in_order():
    lib = _lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first
    ok = dict(B=1, Hq=8, Hkv=2, q=1, cap=4096, d=128, scale=0.125, dtype=0, causal=1, ns=1, ws=None, wsb=0)

    def call(ptrs=(one,) * 7, **kw):
        a = dict(ok, **kw)
        return lib.fa2_forward_decode(*ptrs, a["B"], a["Hq"], a["Hkv"], a["q"], a["cap"], a["d"], a["scale"], a["dtype"], a["causal"],
                                      a["ns"], a["ws"], a["wsb"], None)

    for missing in (0, 1, 2, 5, 6):          # Q, K_cache, V_cache, O, L
        ptrs = [one] * 7
        ptrs[missing] = None
        assert call(tuple(ptrs), d=96, dtype=7, B=0) == -1            # a NULL tensor comes before everything else
    # seqlens_k and sink may be NULL: the call gets past the pointers and fails on what follows
    assert call((one, one, one, None, None, one, one), B=0) == -2
    for bad in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(q=0), dict(cap=0), dict(scale=0.0), dict(scale=-1.0), dict(Hq=8, Hkv=3),
                dict(ns=-1), dict(ns=257), dict(cap=1 << 23, d=128), dict(cap=1 << 24, d=64)):
        assert call(**dict(bad, dtype=7)) == -2, bad                  # shapes before head_dim and dtype
    assert call(cap=(1 << 23) - 1, dtype=7) == -4                     # the largest slab below 2 GiB passes the shape checks
    assert call(d=96, dtype=7) == -3                                   # head_dim before dtype
    assert call(d=256) == -3
    for dtype in (1, 2, 7):
        assert call(dtype=dtype, ns=4, q=64) == -4                     # dtype before the workspace and the row limit
    need = lib.fa2_decode_workspace_bytes(1, 8, 2, 1, 4096, 128, 4)
    assert call(ns=4, q=64) == -5                                      # the workspace before the row limit
    assert call(ns=4, ws=one, wsb=need - 1) == -5
    assert call(ns=0, ws=None) == -5                                   # 0 resolves to 16 splits here: a workspace is needed
    assert call(ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5          # 16-byte alignment
    assert call(ns=1, q=9) == -6                                       # G q_len = 4 x 9 = 36 rows
    assert call(ns=4, q=9, ws=one, wsb=lib.fa2_decode_workspace_bytes(1, 8, 2, 9, 4096, 128, 4)) == -6
    assert call(Hq=64, Hkv=1) == -6
    assert b"unsupported combination" in lib.fa2_status_string(-6)


# ------------------------------------------------------------------------------------------------ (iii)
def test_num_splits_examples():
    f = _lib().fa2_decode_num_splits
    assert f(1, 8, 131072, 128) == 32          # fills 256 workgroups
    assert f(1, 8, 4096, 128) == 16            # ... but a split keeps MIN_SPLIT_KEYS keys
    assert f(1, 8, 4096, 128) == 4096 // dr.MIN_SPLIT_KEYS
    assert f(1, 1, 1 << 20, 64) == 256         # the cap
    assert f(8, 8, 8192, 128) == 4
    assert f(64, 8, 2048, 128) == 1            # enough groups already
    assert f(3, 5, 100000, 128) == 18          # ceil(256 / 15)
    assert f(1, 8, 100, 128) == 1              # a cache shorter than one split
    assert f(1, 8, 4096, 64) == f(1, 8, 4096, 128)
    assert f(0, 8, 4096, 128) == 1 and f(1, 0, 4096, 128) == 1 and f(1, 8, 0, 128) == 1
    for c in dr.CASES:
        assert f(len(c["lens"]), c["hkv"], c["ncap"], c["d"]) == dr.resolved_splits(c, 0)


def test_workspace_bytes_examples():
    lib = _lib()
    w = lib.fa2_decode_workspace_bytes
    assert w(1, 8, 2, 1, 4096, 128, 1) == 0
    assert w(64, 8, 8, 1, 2048, 128, 0) == 0                            # 0 resolves to one split
    assert w(1, 8, 2, 1, 4096, 128, 4) == 4 * 8 * 129 * 4 + (-(4 * 8 * 129 * 4)) % 256
    assert w(2, 8, 2, 4, 4096, 64, 7) == (7 * 2 * 8 * 4 * 65 * 4 + 255) // 256 * 256
    for B, Hq, Hkv, q, cap, d in ((1, 8, 2, 1, 4096, 128), (1, 64, 8, 1, 131072, 128), (8, 32, 8, 4, 8192, 64), (9, 3, 3, 4, 2560, 64)):
        ns = lib.fa2_decode_num_splits(B, Hkv, cap, d)
        assert w(B, Hq, Hkv, q, cap, d, 0) == w(B, Hq, Hkv, q, cap, d, ns)      # the two functions resolve 0 alike
        assert ns == 1 or w(B, Hq, Hkv, q, cap, d, 0) >= ns * B * Hq * q * (d + 1) * 4
    assert w(0, 8, 2, 1, 4096, 128, 4) == 0 and w(1, 8, 2, 1, 4096, 128, 257) == 0 and w(1, 8, 2, 1, 4096, 128, -1) == 0


# ------------------------------------------------------------------------------------------------ (iv)
def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


@pytest.mark.parametrize("what,kw,match", [
    ("Q rank", dict(Q=_t(8, 1, 128)), r"Q: expected a \[B, H, N, d\] tensor"),
    ("K rank", dict(K=_t(2, 300, 128)), r"K_cache: expected a \[B, H, N, d\] tensor"),
    ("V no tensor", dict(V=[1.0]), r"V_cache: expected a \[B, H, N, d\] tensor"),
    ("batch", dict(K=_t(3, 2, 300, 128), V=_t(3, 2, 300, 128)), "K_cache: shape .* does not match Q"),
    ("head_dim differs", dict(K=_t(2, 2, 300, 64), V=_t(2, 2, 300, 64)), "K_cache: shape .* does not match Q"),
    ("heads do not divide", dict(K=_t(2, 3, 300, 128), V=_t(2, 3, 300, 128)), "H_kv dividing H = 8"),
    ("empty cache", dict(K=_t(2, 2, 0, 128), V=_t(2, 2, 0, 128)), "N_cap >= 1"),
    ("V shape", dict(V=_t(2, 2, 301, 128)), "V_cache: shape .* does not match K_cache"),
    ("Q dtype", dict(Q=_t(2, 8, 1, 128, dtype=torch.float32)), "Q: dtype torch.float32, expected torch.bfloat16"),
    ("K dtype", dict(K=_t(2, 2, 300, 128, dtype=torch.float16)), "K_cache: dtype torch.float16"),
    ("V dtype", dict(V=_t(2, 2, 300, 128, dtype=torch.float32)), "V_cache: dtype torch.float32"),
    ("head_dim", dict(Q=_t(2, 8, 1, 96), K=_t(2, 2, 300, 96), V=_t(2, 2, 300, 96)), "head_dim 96, expected 64 or 128"),
    ("too many rows", dict(Q=_t(2, 8, 9, 128)), "36 rows, decode takes at most 32.*flash_attention_2_qk_forward"),
    ("n_splits range", dict(n_splits=257), "n_splits: 257"),
    ("n_splits negative", dict(n_splits=-1), "n_splits: -1"),
    ("n_splits type", dict(n_splits=2.0), "n_splits: 2.0"),
    ("seqlens list", dict(seqlens_k=[300, 200]), "seqlens_k must be an int32 device tensor.*got list.*the host never does"),
    ("seqlens dtype", dict(seqlens_k=torch.tensor([300, 200])), "seqlens_k: dtype torch.int64, expected torch.int32"),
    ("seqlens count", dict(seqlens_k=torch.tensor([300, 200, 1], dtype=torch.int32)), r"seqlens_k: shape \(3,\), expected \(2,\)"),
    ("seqlens rank", dict(seqlens_k=torch.tensor([[300, 200]], dtype=torch.int32)), r"seqlens_k: shape \(1, 2\)"),
    ("seqlens strided", dict(seqlens_k=torch.zeros(4, dtype=torch.int32)[::2]), "seqlens_k must be contiguous"),
    ("seqlens on the host", dict(seqlens_k=torch.tensor([300, 200], dtype=torch.int32)), "seqlens_k is a CPU tensor.*on the device"),
    ("sink no tensor", dict(sink=[0.0] * 8), "sink must be a torch tensor"),
    ("sink dtype", dict(sink=_t(8)), "sink: dtype torch.bfloat16, expected torch.float32"),
    ("sink count", dict(sink=_t(2, dtype=torch.float32)), r"sink: shape \(2,\), expected \(8,\)"),
    ("sink on the host", dict(sink=_t(8, dtype=torch.float32)), "sink must be a device tensor"),
    ("Q on the host", dict(), "Q must be a device tensor"),
    ("Q strided", dict(Q=_t(2, 8, 2, 128)[:, :, ::2]), "Q must be a device tensor|Q must be contiguous"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Q=_t(2, 8, 1, 128), K=_t(2, 2, 300, 128), V=_t(2, 2, 300, 128))
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        fa.flash_attention_2_decode(a.pop("Q"), a.pop("K"), a.pop("V"), **a)


def test_wrapper_is_exported_and_documented():
    import cuda_flashattention_amd as fa
    doc = fa.flash_attention_2_decode.__doc__
    assert "INFERENCE ONLY" in doc and "GRAPH CAPTURE" in doc and "merge_states_forward" in doc
    assert fa.decode_num_splits(1, 8, 131072, 128) == 32
    assert fa.ops.DECODE_MAX_ROWS == dr.MAX_ROWS
