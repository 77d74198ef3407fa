"""CPU: the argument checks of paged decode, without a GPU.
(i) Every ValueError of cuda_flashattention_amd.flash_attention_2_decode_paged that CPU tensors and wrong shapes can reach, one test
per check, each naming its argument.
(ii) fa2_forward_decode_paged's status codes, in the documented order, with pointers that are never dereferenced."""
import ctypes

import pytest
import torch

import decode_ref as dr


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _table(*shape, dtype=torch.int32):
    return torch.zeros(*shape, dtype=dtype)


@pytest.mark.parametrize("what,kw,match", [
    ("Q rank", dict(Q=_t(8, 1, 128)), r"Q: expected a 4-d tensor \(\[B, H, N_q, d\]\)"),
    ("K rank", dict(K=_t(2, 64, 128)), r"K_pages: expected a 4-d tensor \(\[n_pages, H_kv, page_size, d\]\)"),
    ("V no tensor", dict(V=[1.0]), r"V_pages: expected a 4-d tensor"),
    ("head_dim differs", dict(K=_t(12, 2, 64, 64), V=_t(12, 2, 64, 64)), "K_pages: shape .* does not match Q"),
    ("heads do not divide", dict(K=_t(12, 3, 64, 128), V=_t(12, 3, 64, 128)), "H_kv dividing H = 8"),
    ("no pages", dict(K=_t(0, 2, 64, 128), V=_t(0, 2, 64, 128)), "n_pages, page_size >= 1"),
    ("empty pages", dict(K=_t(12, 2, 0, 128), V=_t(12, 2, 0, 128)), "n_pages, page_size >= 1"),
    ("page_size 48", dict(K=_t(12, 2, 48, 128), V=_t(12, 2, 48, 128)), "K_pages: page_size 48 is not a multiple of 32"),
    ("page_size 16", dict(K=_t(12, 2, 16, 128), V=_t(12, 2, 16, 128)), "K_pages: page_size 16 is not a multiple of 32"),
    ("V shape", dict(V=_t(13, 2, 64, 128)), "V_pages: shape .* does not match K_pages"),
    ("Q dtype", dict(Q=_t(2, 8, 1, 128, dtype=torch.float32)), "Q: dtype torch.float32, expected torch.bfloat16"),
    ("K dtype", dict(K=_t(12, 2, 64, 128, dtype=torch.float16)), "K_pages: dtype torch.float16"),
    ("V dtype", dict(V=_t(12, 2, 64, 128, dtype=torch.float32)), "V_pages: dtype torch.float32"),
    ("head_dim", dict(Q=_t(2, 8, 1, 96), K=_t(12, 2, 64, 96), V=_t(12, 2, 64, 96)), "head_dim 96, expected 64 or 128"),
    ("too many rows", dict(Q=_t(2, 8, 9, 128)), "36 rows, decode takes at most 32.*flash_attention_2_qk_forward"),
    ("n_splits range", dict(n_splits=257), "n_splits: 257"),
    ("n_splits negative", dict(n_splits=-1), "n_splits: -1"),
    ("n_splits type", dict(n_splits=2.0), "n_splits: 2.0"),
    ("table list", dict(T=[[0, 1], [2, 3]]), "block_table must be an int32 device tensor.*got list.*the host never does"),
    ("table dtype", dict(T=_table(2, 5, dtype=torch.int64)), "block_table: dtype torch.int64, expected torch.int32"),
    ("table batch", dict(T=_table(3, 5)), r"block_table: shape \(3, 5\), expected \(2, max_pages\)"),
    ("table rank", dict(T=_table(10)), r"block_table: shape \(10,\), expected \(2, max_pages\)"),
    ("table empty", dict(T=_table(2, 0)), r"block_table: shape \(2, 0\)"),
    ("table strided", dict(T=_table(2, 10)[:, ::2]), "block_table must be contiguous"),
    ("table on the host", dict(), "block_table is a CPU tensor.*on the device"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_wrapper_refuses(what, kw, match):
    """(What follows the table's device check -- seqlens_k, sink, the tensors' devices, the workspace -- are flash_attention_2_decode's
    own helpers, tested with it; tests/test_gpu_decode_paged.py runs them on device tensors.)"""
    import cuda_flashattention_amd as fa
    a = dict(Q=_t(2, 8, 1, 128), K=_t(12, 2, 64, 128), V=_t(12, 2, 64, 128), T=_table(2, 5))
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        fa.flash_attention_2_decode_paged(a.pop("Q"), a.pop("K"), a.pop("V"), a.pop("T"), **a)


def test_wrapper_is_exported_and_documented():
    import cuda_flashattention_amd as fa
    doc = fa.flash_attention_2_decode_paged.__doc__
    assert "INFERENCE ONLY" in doc and "GRAPH CAPTURE" in doc and "decode_workspace" in doc and "decode_num_splits" in doc
    assert "max_pages * page_size" in doc and "token-major" in doc
    assert fa.ops.DECODE_PAGE_GRAIN == dr.TILE


def test_status_codes_in_order():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first
    ok = dict(B=1, Hq=8, Hkv=2, q=1, pages=100, P=64, mp=64, d=128, scale=0.125, dtype=0, causal=1, ns=1, ws=None, wsb=0)

    def call(ptrs=(one,) * 8, **kw):
        a = dict(ok, **kw)
        return lib.fa2_forward_decode_paged(*ptrs, a["B"], a["Hq"], a["Hkv"], a["q"], a["pages"], a["P"], a["mp"], a["d"], a["scale"],
                                            a["dtype"], a["causal"], a["ns"], a["ws"], a["wsb"], None)

    for missing in (0, 1, 2, 3, 6, 7):       # Q, K_pages, V_pages, block_table, O, L
        ptrs = [one] * 8
        ptrs[missing] = None
        assert call(tuple(ptrs), d=96, dtype=7, B=0) == -1            # a NULL tensor comes before everything else
    # seqlens_k and sink may be NULL: the call gets past the pointers and fails on what follows
    assert call((one, one, one, one, None, None, one, one), B=0) == -2
    for bad in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(q=0), dict(pages=0), dict(pages=-1), dict(P=0), dict(mp=0), dict(scale=0.0),
                dict(scale=-1.0), dict(Hq=8, Hkv=3), dict(P=48), dict(P=16), dict(P=33), dict(P=-32),
                dict(P=1 << 16, mp=1 << 15), dict(P=1 << 20, mp=1 << 20),      # the capacity: 2^31 keys, and 2^40
                dict(ns=-1), dict(ns=257),
                dict(B=1 << 24, Hq=1, Hkv=1, ns=256)):                          # the grid: 2^32 workgroups
        assert call(**dict(bad, d=96, dtype=7)) == -2, bad            # shapes before head_dim and dtype
    assert call(P=1 << 15, mp=(1 << 15), dtype=7) == -4               # 2^30 keys pass the shape checks
    assert call(P=96, dtype=7) == -4                                   # a page size that is no power of two
    assert call(d=96, dtype=7) == -3                                   # head_dim before dtype
    assert call(d=256) == -3
    for dtype in (1, 2, 7):
        assert call(dtype=dtype, ns=4, q=64) == -4                     # dtype before the workspace and the row limit
    need = lib.fa2_decode_workspace_bytes(1, 8, 2, 1, 64 * 64, 128, 4)
    assert need > 0
    assert call(ns=4, q=64) == -5                                      # the workspace before the row limit
    assert call(ns=4, ws=one, wsb=need - 1) == -5
    assert call(ns=0, ws=None) == -5                                   # 0 resolves to 16 splits at a capacity of 4096
    assert call(ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5          # 16-byte alignment
    assert call(ns=1, q=9) == -6                                       # M = 4 x 9 = 36 rows
    assert call(ns=4, q=9, ws=one, wsb=lib.fa2_decode_workspace_bytes(1, 8, 2, 9, 64 * 64, 128, 4)) == -6
    assert call(Hq=64, Hkv=1) == -6
