"""CPU: the argument checks of the sparse MLA decode (include/fa2_mla_sparse_mi355x.h), without a GPU: the four symbols are
declared, exported, bound through _capi.MLA_SPARSE_SIGNATURES and stand in no other table; the status codes come in the documented
order with pointers that are never dereferenced; the workspace is the dense MLA decode's."""
import ctypes
import re

import pytest

NEW = ("fa2_forward_mla_decode_sparse", "fa2_forward_mla_decode_sparse_paged", "fa2_mla_sparse_num_splits", "fa2_mla_sparse_workspace_bytes")
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.MLA_SPARSE_HEADER_PATH).read(), flags=re.S)
    so, bound = ctypes.CDLL(_capi.LIB_PATH), _capi.lib()
    assert sorted(_capi.MLA_SPARSE_SIGNATURES) == sorted(NEW) == sorted(set(re.findall(r"\b(fa2_\w+)\s*\(", text)))
    others = [t for n, t in vars(_capi).items() if n.endswith("SIGNATURES") and n != "MLA_SPARSE_SIGNATURES"]
    for name in NEW:
        assert hasattr(so, name) and not any(name in t for t in others), name
        res, args = _capi.MLA_SPARSE_SIGNATURES[name]
        params = [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_float if "float" in p else ctypes.c_int
                for p in params]
        assert list(args) == want == list(getattr(bound, name).argtypes), name
        assert res is (ctypes.c_size_t if name.endswith("bytes") else ctypes.c_int)


def _contiguous(lib, ptrs=(ONE, ONE, ONE, None, ONE, ONE), **kw):
    a = dict(B=2, H=16, q=1, topk=2048, cap=4096, rank=512, rope=64, scale=0.1, causal=1, ns=1, ws=None, wsb=0)
    a.update(kw)
    return lib.fa2_forward_mla_decode_sparse(*ptrs, a["B"], a["H"], a["q"], a["topk"], a["cap"], a["rank"], a["rope"], a["scale"],
                                             a["causal"], a["ns"], a["ws"], a["wsb"], None)


def _paged(lib, ptrs=(ONE, ONE, ONE, ONE, None, ONE, ONE), **kw):
    a = dict(B=2, H=16, q=1, topk=2048, pages=200, P=64, mp=64, rank=512, rope=64, scale=0.1, causal=1, ns=1, ws=None, wsb=0)
    a.update(kw)
    return lib.fa2_forward_mla_decode_sparse_paged(*ptrs, a["B"], a["H"], a["q"], a["topk"], a["pages"], a["P"], a["mp"], a["rank"],
                                                   a["rope"], a["scale"], a["causal"], a["ns"], a["ws"], a["wsb"], None)


@pytest.mark.parametrize("call,required", ((_contiguous, (0, 1, 2, 4, 5)), (_paged, (0, 1, 2, 3, 5, 6))), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, required):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    n_ptrs = 6 if call is _contiguous else 7
    for missing in required:      # Q, the cache, (block_table,) indices, O, L: NULL comes first; seqlens_k may be NULL
        ptrs = [ONE] * n_ptrs
        ptrs[missing] = None
        assert call(lib, tuple(ptrs), B=0, rank=256) == -1, missing
    shapes = [dict(B=0), dict(H=0), dict(q=0), dict(topk=0), dict(topk=-1), dict(topk=2 ** 31 - 33023), dict(scale=0.0), dict(scale=-1.0),
              dict(ns=-1), dict(ns=257), dict(B=1 << 14, H=1 << 12, q=1 << 6)]
    shapes += [dict(cap=0), dict(cap=1 << 21)] if call is _contiguous else [dict(pages=0), dict(P=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15)]
    for bad in shapes:            # shapes before the widths
        assert call(lib, **dict(bad, rank=256)) == -2, bad
    for rank, rope in ((256, 64), (512, 128), (576, 0), (64, 512), (0, 0)):      # only (512, 64); before the workspace
        assert call(lib, rank=rank, rope=rope, ns=4) == -3, (rank, rope)
    assert call(lib, B=1 << 16, H=64, q=1 << 8, ns=256) == -2      # the grid B q_len ceil(H / 32) n_splits
    need = lib.fa2_mla_sparse_workspace_bytes(2, 16, 1, 2048, 512, 64, 4)
    assert need == (4 * 2 * 16 * 513 * 4 + 255) // 256 * 256
    assert call(lib, ns=4) == -5 and call(lib, ns=4, ws=ONE, wsb=need - 1) == -5 and call(lib, ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    assert call(lib, ns=0) == -5      # n_splits = 0 resolves by the rule: 2 workgroups on 2048 slots are 8 splits


@pytest.mark.parametrize("B,H,q,topk", ((1, 16, 1, 2048), (1, 128, 1, 2048), (8, 16, 2, 512), (64, 128, 1, 2048), (3, 5, 3, 33), (1, 40, 1, 255),
                                        (300, 16, 1, 4096)))
def test_num_splits_and_workspace_follow_the_rule(B, H, q, topk):
    from cuda_flashattention_amd import _capi
    import cuda_flashattention_amd as fa
    lib = _capi.lib()
    want = min(-(-256 // (B * q * -(-H // 32))), max(1, topk // 256), 256)
    assert lib.fa2_mla_sparse_num_splits(B, H, q, topk, 512, 64) == fa.mla_sparse_num_splits(B, H, q, topk) == want
    assert fa.mla_sparse_workspace(B, H, q, topk, 0, device="cpu").numel() == lib.fa2_mla_sparse_workspace_bytes(B, H, q, topk, 512, 64, want)
    for ns in (2, 5, 256):        # the dense MLA decode's partial layout at the same explicit split count
        assert lib.fa2_mla_sparse_workspace_bytes(B, H, q, topk, 512, 64, ns) == lib.fa2_mla_decode_workspace_bytes(B, H, q, 4096, 512, 64, ns) > 0
    assert lib.fa2_mla_sparse_workspace_bytes(B, H, q, topk, 512, 64, 1) == 0 and lib.fa2_mla_sparse_num_splits(B, H, q, topk, 256, 64) == 1
    assert lib.fa2_mla_sparse_workspace_bytes(B, H, q, topk, 512, 64, 257) == 0 and lib.fa2_mla_sparse_workspace_bytes(B, H, q, 0, 512, 64, 2) == 0
