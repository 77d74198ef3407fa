"""CPU: the argument checks of the MLA latent-cache append (include/fa2_mla_append_mi355x.h), without a GPU: the two symbols are
declared in the header, exported and bound through _capi.MLA_APPEND_SIGNATURES (and in neither pinned table); the status codes
come in the documented order with pointers that are never dereferenced."""
import ctypes
import re

import pytest

NEW = ("fa2_mla_kv_append", "fa2_mla_kv_append_paged")
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first
INT_MAX = 0x7fffffff


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.MLA_APPEND_HEADER_PATH).read(), flags=re.S)
    so, bound = ctypes.CDLL(_capi.LIB_PATH), _capi.lib()
    assert sorted(_capi.MLA_APPEND_SIGNATURES) == sorted(NEW) == sorted(set(re.findall(r"\b(fa2_\w+)\s*\(", text)))
    for name in NEW:
        assert hasattr(so, name) and name not in _capi.SIGNATURES and name not in _capi.MLA_SIGNATURES, name
        res, args = _capi.MLA_APPEND_SIGNATURES[name]
        params = [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctypes.c_longlong if "long long" in p else ctypes.c_float if "float" in p else ctypes.c_int
                for p in params]
        assert list(args) == want == list(getattr(bound, name).argtypes), name
        assert res is ctypes.c_int


# the pointers in the order of the declaration: q_nope, q_pe, Q_out, kv_new, the cache, (block_table,) cos, sin, kv_weight, seqlens_k
def _contiguous(lib, ptrs=(ONE,) * 9, **kw):
    a = dict(eps=1e-6, B=2, H=16, n=1, cap=4096, rank=512, rope=64, npos=4096, il=0, strides=(8192, 512, 512, 3072, 192, 3072, 576, 576))
    a.update(kw)
    return lib.fa2_mla_kv_append(*ptrs[:8], a["eps"], ptrs[8], a["B"], a["H"], a["n"], a["cap"], a["rank"], a["rope"], a["npos"], a["il"],
                                 *a["strides"], None)


def _paged(lib, ptrs=(ONE,) * 10, **kw):
    a = dict(eps=1e-6, B=2, H=16, n=1, pages=200, P=64, mp=64, rank=512, rope=64, npos=4096, il=0,
             strides=(8192, 512, 512, 3072, 192, 3072, 576, 576))
    a.update(kw)
    return lib.fa2_mla_kv_append_paged(*ptrs[:9], a["eps"], ptrs[9], a["B"], a["H"], a["n"], a["pages"], a["P"], a["mp"], a["rank"], a["rope"],
                                       a["npos"], a["il"], *a["strides"], None)


@pytest.mark.parametrize("call", (_contiguous, _paged), ids=("contiguous", "paged"))
def test_status_codes_in_order(call):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    n_ptrs = 9 if call is _contiguous else 10
    bad_everything = dict(B=0, rank=256)
    for missing in range(3, n_ptrs):      # kv_new, the cache, (block_table,) cos, sin, kv_weight, seqlens_k: NULL comes before everything else
        ptrs = [ONE] * n_ptrs
        ptrs[missing] = None
        assert call(lib, tuple(ptrs), **bad_everything) == -1, missing
    for gone in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):      # q_nope, q_pe and Q_out come as a triple
        assert call(lib, tuple(None if i in gone else ONE for i in range(n_ptrs)), **bad_everything) == -1, gone
    cache_only = (None,) * 3 + (ONE,) * (n_ptrs - 3)
    assert call(lib, cache_only, **bad_everything) == -1      # all three NULL with H != 0
    assert call(lib, cache_only, H=0, rank=256) == -3         # H = 0: the cache-only call passes every check but the widths
    nan, inf = float("nan"), float("inf")
    shapes = [dict(B=0), dict(n=0), dict(H=-1), dict(B=1 << 14, H=(1 << 12) - 1, n=1 << 5), dict(B=INT_MAX, H=1),
              dict(eps=0.0), dict(eps=-1e-6), dict(eps=nan), dict(eps=inf), dict(il=2), dict(il=-1), dict(npos=4095)]
    shapes += [dict(cap=0), dict(cap=1 << 21, npos=1 << 21)] if call is _contiguous else \
        [dict(pages=0), dict(P=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15, npos=INT_MAX)]
    good = (8192, 512, 512, 3072, 192, 3072, 576, 576)
    shapes += [dict(strides=good[:i] + (s,) + good[i + 1:]) for i in range(8) for s in (-8, 12)]
    for bad in shapes:            # shapes before the widths
        assert call(lib, **dict(bad, rank=256)) == -2, bad
    for at in range(n_ptrs):      # a misaligned pointer, the table and the lengths (int32: 4-byte aligned) apart
        if at == n_ptrs - 1 or (call is _paged and at == 5):
            continue
        ptrs = [ONE] * n_ptrs
        ptrs[at] = ctypes.c_void_p(24)
        assert call(lib, tuple(ptrs), rank=256) == -2, at
    for rank, rope in ((256, 64), (512, 128), (576, 0), (64, 512), (0, 0)):      # only (512, 64), and last
        assert call(lib, rank=rank, rope=rope) == -3, (rank, rope)
