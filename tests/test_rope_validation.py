"""CPU: the argument checks of the rotary-embedding KV-cache append, without a GPU.
(i) include/fa2_rope_mi355x.h's symbols are exported by libfa2_mi355x.so and _capi.ROPE_SIGNATURES mirrors the header.
(ii) The status codes of fa2_rope_kv_append and fa2_rope_kv_append_paged, in the documented order, with pointers that are never
dereferenced (every one of them is decided before any HIP call).
(iii) Every ValueError of rope_kv_cache_append / rope_kv_cache_append_paged that CPU tensors can reach, each naming its argument."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", "", text, flags=re.M)      # preprocessor lines (function-like macros are not exports)
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))


def test_header_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    names = _declared("fa2_rope_mi355x.h")
    assert names == ["fa2_rope_kv_append", "fa2_rope_kv_append_paged"]
    lib = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/fa2_rope_mi355x.h but not exported"
    assert sorted(_capi.ROPE_SIGNATURES) == names
    assert not set(_capi.ROPE_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.KVCACHE_SIGNATURES))
    bound = _capi.lib()
    for n, (res, args) in _capi.ROPE_SIGNATURES.items():
        assert list(getattr(bound, n).argtypes) == list(args) and getattr(bound, n).restype == res


def test_binding_table_counts_the_headers_arguments():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.ROPE_HEADER_PATH).read(), flags=re.S)
    for name, (_, args) in _capi.ROPE_SIGNATURES.items():
        params = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_longlong if "long long" in p else ctypes.c_int
            assert a is want, (name, p.strip())


def test_the_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "fa2_rope_mi355x.h")).read()
    for words in ("POSITION.", "TABLES.", "PAIRS.", "ARITHMETIC.", "Q_OUT.", "STATUS CODES", "NOT COVERED", "HF's all-bf16 arithmetic",
                  "is not\n * reproduced", "position_ids", "a backward", "ragged n_new", "ONE SEQUENCE EACH", "only NaN-ness"):
        assert words in text, words


ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first
NULL, SHAPE, HEAD_DIM, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -6
BF16, F32, E4M3 = 0, 1, 2
BASE = dict(Q=ONE, Qo=ONE, Kn=ONE, Vn=ONE, K=ONE, V=ONE, cos=ONE, sin=ONE, lens=ONE, kd=None, vd=None, B=2, Hq=4, H=2, n=1, d=128,
            rot=64, npos=96, il=0, qb=512, qh=128, qt=512, sb=256, sh=128, st=256, dtype=BF16, kv=BF16)


def _contiguous(lib, **kw):
    a = dict(BASE, cap=96)
    a.update(kw)
    return lib.fa2_rope_kv_append(a["Q"], a["Qo"], a["Kn"], a["Vn"], a["K"], a["V"], a["cos"], a["sin"], a["lens"], a["kd"], a["vd"],
                                  a["B"], a["Hq"], a["H"], a["n"], a["cap"], a["d"], a["rot"], a["npos"], a["il"],
                                  a["qb"], a["qh"], a["qt"], a["sb"], a["sh"], a["st"], a["dtype"], a["kv"], None)


def _paged(lib, **kw):
    a = dict(BASE, T=ONE, pages=8, P=32, mp=3)
    a.update(kw)
    return lib.fa2_rope_kv_append_paged(a["Q"], a["Qo"], a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["cos"], a["sin"], a["lens"], a["kd"],
                                        a["vd"], a["B"], a["Hq"], a["H"], a["n"], a["pages"], a["P"], a["mp"], a["d"], a["rot"], a["npos"],
                                        a["il"], a["qb"], a["qh"], a["qt"], a["sb"], a["sh"], a["st"], a["dtype"], a["kv"], None)


# one invalid value per class of the status table, in the table's order
NULLS = [dict(Kn=None), dict(Vn=None), dict(K=None), dict(V=None), dict(lens=None), dict(cos=None), dict(sin=None), dict(Q=None),
         dict(Qo=None), dict(Q=None, Qo=None)]
SHAPES = [dict(B=0), dict(H=0), dict(n=0), dict(n=-1), dict(d=0), dict(Hq=-1), dict(rot=0), dict(rot=8), dict(rot=24), dict(rot=144),
          dict(rot=-16), dict(npos=95), dict(npos=0), dict(il=2), dict(il=-1), dict(qb=-8), dict(qh=4), dict(qt=12), dict(sb=-8), dict(sh=4),
          dict(st=12), dict(Q=ctypes.c_void_p(24)), dict(Qo=ctypes.c_void_p(8)), dict(cos=ctypes.c_void_p(4)), dict(sin=ctypes.c_void_p(40)),
          dict(Kn=ctypes.c_void_p(24)), dict(Vn=ctypes.c_void_p(8)), dict(K=ctypes.c_void_p(4)), dict(V=ctypes.c_void_p(2)),
          dict(B=1 << 20, H=1 << 10, n=4), dict(B=1 << 20, Hq=(1 << 10) - 2, n=2)]
SHAPES_CONTIGUOUS = [dict(cap=0), dict(cap=1 << 25, kv=BF16), dict(cap=1 << 26, kv=E4M3)]
SHAPES_PAGED = [dict(pages=0), dict(P=0), dict(mp=0), dict(P=48), dict(P=16), dict(P=1 << 16, mp=1 << 15)]
LATER = [(dict(d=96), HEAD_DIM), (dict(dtype=F32), DTYPE), (dict(dtype=E4M3), DTYPE), (dict(kv=F32), DTYPE), (dict(kv=7), DTYPE),
         (dict(kd=ONE), UNSUPPORTED), (dict(vd=ONE), UNSUPPORTED)]


@pytest.mark.parametrize("call,shapes", ((_contiguous, SHAPES_CONTIGUOUS), (_paged, SHAPES_PAGED)), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, shapes):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    nulls = NULLS + ([dict(T=None)] if call is _paged else [])
    for kw in nulls:
        assert call(lib, **kw) == NULL, kw
    for kw in SHAPES + shapes:
        assert call(lib, **kw) == SHAPE, kw
    for kw, status in LATER:
        assert call(lib, **kw) == status, kw
    # the order: an earlier class wins over every later one
    later = [kw for kw, _ in LATER]
    for first, status, rest in ((nulls, NULL, SHAPES + shapes + later), (SHAPES + shapes, SHAPE, later)):
        for a in first:
            for b in rest:
                if not set(a) & set(b):
                    assert call(lib, **a, **b) == status, (a, b)
    for i, (a, status) in enumerate(LATER):
        for b in later[i + 1:]:
            if not set(a) & set(b):
                assert call(lib, **a, **b) == status, (a, b)
    # what passes the shape checks stops at a later one (d = 96: no launch): the K/V-only form, both pair forms, full, partial and
    # minimal rot_dim, tables longer than the cache, descales beside an e4m3 cache
    assert call(lib, d=96) == HEAD_DIM
    assert call(lib, d=96, Q=None, Qo=None, Hq=0) == HEAD_DIM and call(lib, d=96, Hq=0) == HEAD_DIM
    assert call(lib, d=96, il=1) == HEAD_DIM and call(lib, d=96, rot=96) == HEAD_DIM and call(lib, d=96, rot=16) == HEAD_DIM
    assert call(lib, d=96, rot=112) == SHAPE and call(lib, d=64, rot=128) == SHAPE
    assert call(lib, d=96, npos=1 << 20) == HEAD_DIM
    assert call(lib, kv=E4M3, kd=ONE, vd=ONE, d=96) == HEAD_DIM
    if call is _contiguous:
        assert call(lib, cap=1 << 23, npos=1 << 23) == SHAPE and call(lib, cap=(1 << 23) - 1, npos=1 << 23, dtype=F32) == DTYPE
        assert call(lib, cap=97) == SHAPE and call(lib, cap=97, npos=97, d=96) == HEAD_DIM        # n_positions >= kv_capacity
    else:
        limit = 0x7fffffff - 33024
        assert call(lib, P=32, mp=limit // 32, npos=limit, d=96) == HEAD_DIM and call(lib, P=32, mp=limit // 32 + 1, npos=0x7fffffff, d=96) == SHAPE
        assert call(lib, mp=4) == SHAPE and call(lib, mp=4, npos=128, d=96) == HEAD_DIM             # ... >= max_pages x page_size


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _fused(B=2, n=3, Hq=4, Hkv=2, d=128):
    """Q, K and V [B, H, n, d] views of one fused [B, n, H_q + 2 H_kv, d] projection output."""
    x = _t(B, n, Hq + 2 * Hkv, d)
    return tuple(t.permute(0, 2, 1, 3) for t in (x[:, :, :Hq], x[:, :, Hq:Hq + Hkv], x[:, :, Hq + Hkv:]))


QV, KN, VN = _fused()
LENS = torch.zeros(2, dtype=torch.int32)
COS, SIN = torch.zeros(96, 32), torch.zeros(96, 32)
F8 = torch.float8_e4m3fn

SHARED = [
    ("K_new rank", dict(Kn=_t(2, 3, 128)), r"K_new: expected a 4-d tensor \[B, H_kv, n_new, d\].*permute"),
    ("V_new dtype", dict(Vn=_t(2, 2, 3, 128, dtype=torch.float16)), "V_new: dtype torch.float16, expected torch.bfloat16"),
    ("head_dim", dict(Kn=_t(2, 2, 3, 96), Vn=_t(2, 2, 3, 96)), "K_new: head_dim 96, expected 64 or 128"),
    ("strides differ", dict(Vn=_t(2, 2, 3, 128)), "V_new: strides .* differ from K_new's"),
    ("Q rank", dict(Q=_t(2, 3, 128)), r"Q: expected a 4-d tensor \[B, H_q, n_new, d\].*permute"),
    ("Q no tensor", dict(Q=[1.0]), "Q: expected a 4-d tensor.*got list"),
    ("Q dtype", dict(Q=_t(2, 4, 3, 128, dtype=torch.float32)), "Q: dtype torch.float32, expected torch.bfloat16"),
    ("Q batch", dict(Q=_t(3, 4, 3, 128)), r"Q: shape .* does not match K_new.*\[2, H_q, 3, 128\]"),
    ("Q tokens", dict(Q=_t(2, 4, 2, 128)), "Q: shape .* does not match K_new"),
    ("Q head_dim", dict(Q=_t(2, 4, 3, 64)), "Q: shape .* does not match K_new"),
    ("Q no heads", dict(Q=_t(2, 0, 3, 128)), "Q: shape .* H_q >= 1"),
    ("Q last stride", dict(Q=_t(2, 4, 3, 256)[..., ::2]), r"Q: stride .*stride\(-1\) == 1.*permute"),
    ("Q stride not 8n", dict(Q=_t(2, 4, 3, 132)[..., :128]), "Q: strides .* multiples of 8 elements"),
    ("Q offset", dict(Q=_t(2, 4, 3, 136)[..., 4:132]), "Q: storage offset 4 elements is not 16-byte aligned"),
    ("cos rank", dict(cos=torch.zeros(96)), r"cos: expected a 2-d tensor \[n_positions, rot_dim / 2\]"),
    ("sin no tensor", dict(sin=None), "sin: expected a 2-d tensor.*got NoneType"),
    ("cos dtype", dict(cos=torch.zeros(96, 32, dtype=torch.float64)), "cos: dtype torch.float64, expected torch.float32"),
    ("sin dtype", dict(sin=torch.zeros(96, 32, dtype=torch.bfloat16)), "sin: dtype torch.bfloat16, expected torch.float32"),
    ("sin shape", dict(sin=torch.zeros(96, 16)), "sin: shape .* does not match cos"),
    ("rot_dim 24", dict(cos=torch.zeros(96, 12), sin=torch.zeros(96, 12)), "cos: shape .* rot_dim of 24, expected a multiple of 16"),
    ("rot_dim 8", dict(cos=torch.zeros(96, 4), sin=torch.zeros(96, 4)), "cos: shape .* rot_dim of 8"),
    ("rot_dim above d", dict(cos=torch.zeros(96, 72), sin=torch.zeros(96, 72)), r"cos: shape .* rot_dim of 144, expected .* \[16, 128\]"),
    ("interleaved", dict(il=1), "interleaved: 1, expected a bool"),
    ("no lengths", dict(lens=None), "seqlens_k is required.*AFTER the"),
]


@pytest.mark.parametrize("what,kw,match", SHARED + [
    ("K_cache rank", dict(K=_t(2, 96, 128)), r"K_cache: expected a 4-d tensor \[B, H_kv, N_cap, d\]"),
    ("K_cache batch", dict(K=_t(3, 2, 96, 128)), r"K_cache: shape .* does not match K_new.*\[2, 2, N_cap, 128\]"),
    ("V_cache shape", dict(V=_t(2, 2, 64, 128)), "V_cache: shape .* does not match K_cache"),
    ("e5m2", dict(K=_t(2, 2, 96, 128, dtype=torch.float8_e5m2)), "K_cache: dtype torch.float8_e5m2; an fp8 cache is OCP e4m3"),
    ("mixed", dict(V=_t(2, 2, 96, 128, dtype=F8)), "V_cache: dtype torch.float8_e4m3fn beside K_cache torch.bfloat16"),
    ("descale beside bf16", dict(kd=torch.ones(2)), "k_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("descale shape", dict(K=_t(2, 2, 96, 128, dtype=F8), V=_t(2, 2, 96, 128, dtype=F8), kd=torch.ones(3)), r"k_descale: shape \(3,\), expected \(2,\)"),
    ("too few positions", dict(cos=torch.zeros(95, 32), sin=torch.zeros(95, 32)), "cos: 95 positions for a cache of 96 rows"),
    ("lengths dtype", dict(lens=torch.zeros(2, dtype=torch.int64)), "seqlens_k: dtype torch.int64"),
    ("lengths on the host", dict(), "seqlens_k is a CPU tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_contiguous_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Q=QV, Kn=KN, Vn=VN, K=_t(2, 2, 96, 128), V=_t(2, 2, 96, 128), cos=COS, sin=SIN, lens=LENS, il=False, kd=None, vd=None)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        fa.rope_kv_cache_append(a["Q"], a["Kn"], a["Vn"], a["K"], a["V"], a["cos"], a["sin"], a["lens"], interleaved=a["il"],
                                k_descale=a["kd"], v_descale=a["vd"])


@pytest.mark.parametrize("what,kw,match", SHARED + [
    ("K_pages rank", dict(K=_t(8, 32, 128)), r"K_pages: expected a 4-d tensor \[n_pages, H_kv, page_size, d\]"),
    ("K_pages heads", dict(K=_t(8, 3, 32, 128)), r"K_pages: shape .* does not match K_new.*\[n_pages, 2, page_size, 128\]"),
    ("page_size 48", dict(K=_t(8, 2, 48, 128), V=_t(8, 2, 48, 128)), "K_pages: page_size 48 is not a multiple of 32"),
    ("V_pages shape", dict(V=_t(9, 2, 32, 128)), "V_pages: shape .* does not match K_pages"),
    ("fnuz", dict(K=_t(8, 2, 32, 128, dtype=torch.float8_e4m3fnuz)), "K_pages: dtype torch.float8_e4m3fnuz; an fp8 cache is OCP e4m3"),
    ("descale beside bf16", dict(vd=torch.ones(2)), "v_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("table list", dict(T=[[0, 1, 2]] * 2), "block_table must be an int32 device tensor.*got list"),
    ("table dtype", dict(T=torch.zeros(2, 3, dtype=torch.int64)), "block_table: dtype torch.int64"),
    ("table batch", dict(T=torch.zeros(3, 3, dtype=torch.int32)), r"block_table: shape \(3, 3\), expected \(2, max_pages\)"),
    ("table on the host", dict(), "block_table is a CPU tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_paged_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Q=QV, Kn=KN, Vn=VN, K=_t(8, 2, 32, 128), V=_t(8, 2, 32, 128), T=torch.zeros(2, 3, dtype=torch.int32), cos=COS, sin=SIN,
             lens=LENS, il=False, kd=None, vd=None)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        fa.rope_kv_cache_append_paged(a["Q"], a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["cos"], a["sin"], a["lens"],
                                      interleaved=a["il"], k_descale=a["kd"], v_descale=a["vd"])


def test_wrappers_are_exported_and_documented():
    import cuda_flashattention_amd as fa
    for f in (fa.rope_kv_cache_append, fa.rope_kv_cache_append_paged):
        assert "returns Q_out" in f.__doc__ and "seqlens_k" in f.__doc__
    doc = fa.rope_kv_cache_append.__doc__
    for words in ("ONLY allocation", "rotate-half", "(2i, 2i + 1)", "no fused multiply-add", "HF's all-bf16 arithmetic", "+0.0 throughout",
                  "flash_attention_2_decode(Q_out"):
        assert words in doc, words
    assert "ONE SEQUENCE EACH" in fa.rope_kv_cache_append_paged.__doc__ and "DROPPED" in fa.rope_kv_cache_append_paged.__doc__
