"""CPU: the argument checks of the MLA decode and append over e4m3 latent caches (include/fa2_mla_fp8_mi355x.h), without a GPU: the
four symbols are declared in the header, exported and bound through _capi.MLA_FP8_SIGNATURES and stand in no other table; the
status codes come in the bf16 calls' order, with the 640-byte row in the contiguous limit, from pointers never dereferenced."""
import ctypes
import re

import pytest

NEW = ("fa2_forward_mla_decode_fp8kv", "fa2_forward_mla_decode_paged_fp8kv", "fa2_mla_kv_append_fp8kv", "fa2_mla_kv_append_paged_fp8kv")
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first
INT_MAX, STRIDES = 0x7fffffff, (8192, 512, 512, 3072, 192, 3072, 576, 576)
DECODE = dict(B=2, H=16, q=1, cap=4096, pages=200, P=64, mp=64, rank=512, rope=64, scale=0.1, causal=1, ns=1, ws=None, wsb=0)
APPEND = dict(eps=1e-6, B=2, H=16, n=1, cap=4096, pages=200, P=64, mp=64, rank=512, rope=64, npos=4096, il=0, strides=STRIDES)


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.MLA_FP8_HEADER_PATH).read(), flags=re.S)
    so, bound = ctypes.CDLL(_capi.LIB_PATH), _capi.lib()
    assert sorted(_capi.MLA_FP8_SIGNATURES) == sorted(NEW) == sorted(set(re.findall(r"\b(fa2_\w+)\s*\(", text)))
    others = [getattr(_capi, t) for t in dir(_capi) if t.endswith("SIGNATURES") and t != "MLA_FP8_SIGNATURES"]
    for name in NEW:
        assert hasattr(so, name) and len(others) >= 9 and not any(name in t for t in others), name
        res, args = _capi.MLA_FP8_SIGNATURES[name]
        params = [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_longlong if "long long" in p else
                ctypes.c_float if "float" in p else ctypes.c_int for p in params]
        assert list(args) == want == list(getattr(bound, name).argtypes) and res is ctypes.c_int, name


def _call(lib, name, ptrs, **kw):
    a = dict(APPEND if "append" in name else DECODE, **kw)
    size = (a["pages"], a["P"], a["mp"]) if "paged" in name else (a["cap"],)
    if "append" in name:      # eps stands between kv_weight and latent_descale
        return getattr(lib, name)(*ptrs[:-2], a["eps"], *ptrs[-2:], a["B"], a["H"], a["n"], *size, a["rank"], a["rope"], a["npos"], a["il"],
                                  *a["strides"], None)
    return getattr(lib, name)(*ptrs, a["B"], a["H"], a["q"], *size, a["rank"], a["rope"], a["scale"], a["causal"], a["ns"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("name", NEW)
def test_status_codes_in_order(name):
    """The pointers in front of the integers: decode Q, cache, (block_table,) latent_descale, seqlens_k, O, L; append q_nope, q_pe,
    Q_out, kv_new, cache, (block_table,) cos, sin, kv_weight, latent_descale, seqlens_k (a lone NULL of the first three: no triple)."""
    from cuda_flashattention_amd import _capi
    lib, append, paged = _capi.lib(), "append" in name, "paged" in name
    n_ptrs, optional = (10 + paged, {8 + paged}) if append else (6 + paged, {2 + paged, 3 + paged})
    full = [ONE] * n_ptrs
    for missing in range(n_ptrs):      # NULL comes before everything else; latent_descale (and the decode's seqlens_k) may be NULL
        ptrs = full[:missing] + [None] + full[missing + 1:]
        assert _call(lib, name, ptrs, B=0, rank=256) == (-2 if missing in optional else -1), missing
        assert _call(lib, name, ptrs, rank=256) == (-3 if missing in optional else -1), missing
    shapes = [dict(B=0), dict(n=0), dict(H=-1), dict(eps=0.0), dict(il=2), dict(npos=4095), dict(strides=(12,) + STRIDES[1:])] if append else \
        [dict(B=0), dict(H=0), dict(q=0), dict(scale=0.0), dict(ns=-1), dict(ns=257), dict(B=1 << 14, H=1 << 12, q=1 << 6)]
    row_limit = INT_MAX // 640      # a contiguous sequence is one buffer resource of 640-byte rows
    shapes += [dict(pages=0), dict(P=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15, npos=INT_MAX)] if paged else \
        [dict(cap=0), dict(cap=row_limit + 1, npos=row_limit + 1)]
    for bad in shapes:                 # shapes before the widths
        assert _call(lib, name, full, **dict(bad, rank=256)) == -2, bad
    if not paged:                      # the last capacity that fits, and the bf16 calls' first refused one, pass on to the widths
        assert _call(lib, name, full, cap=row_limit, npos=row_limit, rank=256) == _call(lib, name, full, cap=1 << 21, npos=1 << 21, rank=256) == -3
    for rank, rope in ((256, 64), (512, 128), (576, 0), (0, 0)):      # only (512, 64): the append's last check, before the decode's workspace
        assert _call(lib, name, full, rank=rank, rope=rope, **({} if append else dict(ns=4))) == -3, (rank, rope)
    if append:
        assert _call(lib, name, full[:4] + [ctypes.c_void_p(24)] + full[5:], rank=256) == -2      # a misaligned cache
        return
    assert _call(lib, name, full, B=1 << 20, H=32, q=32, ns=256) == -2      # the grid B ceil(M / 32) n_splits
    need = lib.fa2_mla_decode_workspace_bytes(2, 16, 1, 4096, 512, 64, 4)      # the bf16 calls' function: the partials are the same
    assert _call(lib, name, full, ns=4) == _call(lib, name, full, ns=4, ws=ONE, wsb=need - 1) == _call(lib, name, full, ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    assert _call(lib, name, full, ns=0) == -5      # n_splits = 0 resolves by the rule: 2 workgroups on 4096 keys are 16 splits
