"""CPU: the argument checks of MLA decode attention (include/fa2_mla_mi355x.h), without a GPU: the four symbols are declared,
exported and bound through _capi.MLA_SIGNATURES; the status codes come in the documented order with pointers that are never
dereferenced; fa2_mla_decode_num_splits and _workspace_bytes follow their stated arithmetic."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fa2_forward_mla_decode", "fa2_forward_mla_decode_paged", "fa2_mla_decode_num_splits", "fa2_mla_decode_workspace_bytes")
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.MLA_HEADER_PATH).read(), flags=re.S)
    so, bound = ctypes.CDLL(_capi.LIB_PATH), _capi.lib()
    assert sorted(_capi.MLA_SIGNATURES) == sorted(NEW) == sorted(set(re.findall(r"\b(fa2_\w+)\s*\(", text)))
    for name in NEW:
        assert hasattr(so, name) and name not in _capi.SIGNATURES, name      # SIGNATURES stays pinned to fa2_mi355x.h
        res, args = _capi.MLA_SIGNATURES[name]
        params = [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_float if "float" in p else ctypes.c_int
                for p in params]
        assert list(args) == want == list(getattr(bound, name).argtypes), name
        assert res is (ctypes.c_size_t if name.endswith("bytes") else ctypes.c_int)


def _contiguous(lib, ptrs=(ONE, ONE, None, ONE, ONE), **kw):
    a = dict(B=2, H=16, q=1, cap=4096, rank=512, rope=64, scale=0.1, causal=1, ns=1, ws=None, wsb=0)
    a.update(kw)
    return lib.fa2_forward_mla_decode(*ptrs, a["B"], a["H"], a["q"], a["cap"], a["rank"], a["rope"], a["scale"], a["causal"], a["ns"],
                                      a["ws"], a["wsb"], None)


def _paged(lib, ptrs=(ONE, ONE, ONE, None, ONE, ONE), **kw):
    a = dict(B=2, H=16, q=1, pages=200, P=64, mp=64, rank=512, rope=64, scale=0.1, causal=1, ns=1, ws=None, wsb=0)
    a.update(kw)
    return lib.fa2_forward_mla_decode_paged(*ptrs, a["B"], a["H"], a["q"], a["pages"], a["P"], a["mp"], a["rank"], a["rope"], a["scale"],
                                            a["causal"], a["ns"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("call,required", ((_contiguous, (0, 1, 3, 4)), (_paged, (0, 1, 2, 4, 5))), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, required):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    n_ptrs = 5 if call is _contiguous else 6
    for missing in required:      # Q, the cache, (block_table,) O, L: NULL comes before everything else; seqlens_k may be NULL
        ptrs = [ONE] * n_ptrs
        ptrs[missing] = None
        assert call(lib, tuple(ptrs), B=0, rank=256) == -1, missing
    shapes = [dict(B=0), dict(H=0), dict(q=0), dict(scale=0.0), dict(scale=-1.0), dict(ns=-1), dict(ns=257), dict(B=1 << 14, H=1 << 12, q=1 << 6)]
    shapes += [dict(cap=0), dict(cap=1 << 21)] if call is _contiguous else [dict(pages=0), dict(P=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15)]
    for bad in shapes:            # shapes before the widths
        assert call(lib, **dict(bad, rank=256)) == -2, bad
    for rank, rope in ((256, 64), (512, 128), (576, 0), (64, 512), (0, 0)):      # only (512, 64); before the workspace
        assert call(lib, rank=rank, rope=rope, ns=4) == -3, (rank, rope)
    assert call(lib, B=1 << 20, H=32, q=32, ns=256) == -2      # the grid B ceil(M / 32) n_splits
    need = lib.fa2_mla_decode_workspace_bytes(2, 16, 1, 4096, 512, 64, 4)
    assert need == (4 * 2 * 16 * 513 * 4 + 255) // 256 * 256
    assert call(lib, ns=4) == -5 and call(lib, ns=4, ws=ONE, wsb=need - 1) == -5 and call(lib, ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    assert call(lib, ns=0) == -5      # n_splits = 0 resolves by the rule: 2 workgroups on 4096 keys are 16 splits


@pytest.mark.parametrize("B,H,q,cap", ((1, 16, 1, 4096), (1, 128, 1, 32768), (8, 16, 2, 8192), (64, 128, 1, 2048), (3, 5, 3, 300), (1, 40, 1, 255),
                                       (1, 1, 1, 1 << 20), (300, 16, 1, 4096)))
def test_num_splits_and_workspace_follow_the_rule(B, H, q, cap):
    from cuda_flashattention_amd import _capi
    import cuda_flashattention_amd as fa
    lib = _capi.lib()
    want = min(-(-256 // (B * -(-H * q // 32))), max(1, cap // 256), 256)
    assert lib.fa2_mla_decode_num_splits(B, H, q, cap, 512, 64) == fa.mla_decode_num_splits(B, H, q, cap) == want
    for ns in (0, 1, 2, 5, 256):
        n = ns or want
        size = 0 if n == 1 else (n * B * H * q * 513 * 4 + 255) // 256 * 256
        assert lib.fa2_mla_decode_workspace_bytes(B, H, q, cap, 512, 64, ns) == fa.mla_decode_workspace(B, H, q, cap, ns, device="cpu").numel() == size
    assert lib.fa2_mla_decode_num_splits(B, H, q, cap, 256, 64) == 1 and lib.fa2_mla_decode_workspace_bytes(B, H, q, cap, 512, 32, 4) == 0
    assert lib.fa2_mla_decode_workspace_bytes(B, H, q, cap, 512, 64, 257) == 0 and lib.fa2_mla_decode_workspace_bytes(0, H, q, cap, 512, 64, 2) == 0
