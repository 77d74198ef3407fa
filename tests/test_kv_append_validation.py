"""CPU: the argument checks of the KV-cache append, without a GPU.
(i) include/fa2_kvcache_mi355x.h's symbols are exported by libfa2_mi355x.so and _capi.KVCACHE_SIGNATURES mirrors the header.
(ii) The status codes of fa2_kv_append and fa2_kv_append_paged, in the documented order, with pointers that are never
dereferenced (every one of them is decided before any HIP call).
(iii) Every ValueError of kv_cache_append / kv_cache_append_paged that CPU tensors can reach, each naming its argument."""
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
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)    # callback tables are not exports
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))


def test_header_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    names = _declared("fa2_kvcache_mi355x.h")
    assert names == ["fa2_kv_append", "fa2_kv_append_paged"]
    lib = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/fa2_kvcache_mi355x.h but not exported"
    assert sorted(_capi.KVCACHE_SIGNATURES) == names
    assert not set(_capi.KVCACHE_SIGNATURES) & set(_capi.SIGNATURES)
    bound = _capi.lib()
    for n, (res, args) in _capi.KVCACHE_SIGNATURES.items():
        assert list(getattr(bound, n).argtypes) == list(args) and getattr(bound, n).restype == res


def test_binding_table_counts_the_headers_arguments():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.KVCACHE_HEADER_PATH).read(), flags=re.S)
    for name, (_, args) in _capi.KVCACHE_SIGNATURES.items():
        params = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_longlong if "long long" in p else ctypes.c_int
            assert a is want, (name, p.strip())


ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first
NULL, SHAPE, HEAD_DIM, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -6
BF16, F32, E4M3 = 0, 1, 2


def _contiguous(lib, **kw):
    a = dict(Kn=ONE, Vn=ONE, K=ONE, V=ONE, lens=ONE, kd=None, vd=None, B=2, H=2, n=1, cap=96, d=128, sb=256, sh=128, st=256,
             dtype=BF16, kv=BF16)
    a.update(kw)
    return lib.fa2_kv_append(a["Kn"], a["Vn"], a["K"], a["V"], a["lens"], a["kd"], a["vd"], a["B"], a["H"], a["n"], a["cap"], a["d"],
                             a["sb"], a["sh"], a["st"], a["dtype"], a["kv"], None)


def _paged(lib, **kw):
    a = dict(Kn=ONE, Vn=ONE, K=ONE, V=ONE, T=ONE, lens=ONE, kd=None, vd=None, B=2, H=2, n=1, pages=8, P=32, mp=3, d=128,
             sb=256, sh=128, st=256, dtype=BF16, kv=BF16)
    a.update(kw)
    return lib.fa2_kv_append_paged(a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["lens"], a["kd"], a["vd"], a["B"], a["H"], a["n"],
                                   a["pages"], a["P"], a["mp"], a["d"], a["sb"], a["sh"], a["st"], a["dtype"], a["kv"], None)


# one invalid value per class of the status table, in the table's order
NULLS = [dict(Kn=None), dict(Vn=None), dict(K=None), dict(V=None), dict(lens=None)]
SHAPES = [dict(B=0), dict(H=0), dict(n=0), dict(n=-1), dict(d=0), dict(sb=-8), dict(sh=4), dict(st=12), dict(Kn=ctypes.c_void_p(24)),
          dict(Vn=ctypes.c_void_p(8)), dict(K=ctypes.c_void_p(4)), dict(V=ctypes.c_void_p(2)), dict(B=1 << 20, H=1 << 10, n=4)]
SHAPES_CONTIGUOUS = [dict(cap=0), dict(cap=1 << 25, kv=BF16), dict(cap=1 << 26, kv=E4M3)]      # a (b, head) slab above 2 GiB at any d
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
    # the slab limit is the decode's: one byte below it passes the shape checks (and stops at a later one)
    assert call(lib, d=96) == HEAD_DIM
    if call is _contiguous:
        assert call(lib, cap=1 << 23) == SHAPE and call(lib, cap=(1 << 23) - 1, dtype=F32) == DTYPE                        # x 128 x 2 bytes
        assert call(lib, cap=1 << 24, kv=E4M3) == SHAPE and call(lib, cap=(1 << 24) - 1, kv=E4M3, dtype=F32) == DTYPE      # x 128 x 1 byte
    else:
        limit = 0x7fffffff - 33024
        assert call(lib, P=32, mp=limit // 32, d=96) == HEAD_DIM and call(lib, P=32, mp=limit // 32 + 1, d=96) == SHAPE
    # descales belong to an e4m3 cache: beside one they pass validation's last check (d = 96 stops the call before any launch)
    assert call(lib, kv=E4M3, kd=ONE, vd=ONE, d=96) == HEAD_DIM


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _fused(B=2, n=3, Hq=4, Hkv=2, d=128):
    """K and V [B, H_kv, n, d] views of one fused [B, n, H_q + 2 H_kv, d] projection output."""
    x = _t(B, n, Hq + 2 * Hkv, d)
    return x[:, :, Hq:Hq + Hkv].permute(0, 2, 1, 3), x[:, :, Hq + Hkv:].permute(0, 2, 1, 3)


KN, VN = _fused()
LENS = torch.zeros(2, dtype=torch.int32)
F8 = torch.float8_e4m3fn

SOURCE = [
    ("K_new rank", dict(Kn=_t(2, 3, 128)), r"K_new: expected a 4-d tensor \[B, H_kv, n_new, d\].*permute"),
    ("V_new no tensor", dict(Vn=[1.0]), "V_new: expected a 4-d tensor.*got list"),
    ("K_new dtype", dict(Kn=_t(2, 2, 3, 128, dtype=torch.float32)), "K_new: dtype torch.float32, expected torch.bfloat16"),
    ("V_new dtype", dict(Vn=_t(2, 2, 3, 128, dtype=torch.float16)), "V_new: dtype torch.float16, expected torch.bfloat16"),
    ("no tokens", dict(Kn=_t(2, 2, 0, 128), Vn=_t(2, 2, 0, 128)), "K_new: shape .* n_new >= 1"),
    ("V_new shape", dict(Vn=_t(2, 2, 4, 128)), "V_new: shape .* does not match K_new"),
    ("head_dim", dict(Kn=_t(2, 2, 3, 96), Vn=_t(2, 2, 3, 96)), "K_new: head_dim 96, expected 64 or 128"),
    ("last stride", dict(Kn=_t(2, 2, 3, 256)[..., ::2], Vn=_t(2, 2, 3, 256)[..., ::2]), r"K_new: stride .*stride\(-1\) == 1.*permute"),
    ("strides differ", dict(Vn=_t(2, 2, 3, 128)), "V_new: strides .* differ from K_new's.*one .* stride triple"),
    ("stride not 8n", dict(Kn=_t(2, 2, 3, 132)[..., :128], Vn=_t(2, 2, 3, 132)[..., :128]), "K_new: strides .* multiples of 8 elements"),
    ("offset", dict(Kn=_t(2, 2, 3, 136)[..., 4:132], Vn=_t(2, 2, 3, 136)[..., 4:132]), "K_new: storage offset 4 elements is not 16-byte aligned"),
]


@pytest.mark.parametrize("what,kw,match", SOURCE + [
    ("K_cache rank", dict(K=_t(2, 96, 128)), r"K_cache: expected a 4-d tensor \[B, H_kv, N_cap, d\]"),
    ("K_cache batch", dict(K=_t(3, 2, 96, 128)), r"K_cache: shape .* does not match K_new.*\[2, 2, N_cap, 128\]"),
    ("K_cache head_dim", dict(K=_t(2, 2, 96, 64)), "K_cache: shape .* does not match K_new"),
    ("V_cache shape", dict(V=_t(2, 2, 64, 128)), "V_cache: shape .* does not match K_cache"),
    ("e5m2", dict(K=_t(2, 2, 96, 128, dtype=torch.float8_e5m2)), "K_cache: dtype torch.float8_e5m2; an fp8 cache is OCP e4m3"),
    ("mixed", dict(V=_t(2, 2, 96, 128, dtype=F8)), "V_cache: dtype torch.float8_e4m3fn beside K_cache torch.bfloat16"),
    ("fp32 cache", dict(K=_t(2, 2, 96, 128, dtype=torch.float32), V=_t(2, 2, 96, 128, dtype=torch.float32)), "K_cache: dtype torch.float32"),
    ("descale beside bf16", dict(kd=torch.ones(2)), "k_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("descale dtype", dict(K=_t(2, 2, 96, 128, dtype=F8), V=_t(2, 2, 96, 128, dtype=F8), vd=torch.ones(2, dtype=torch.float64)),
     "v_descale: dtype torch.float64"),
    ("descale shape", dict(K=_t(2, 2, 96, 128, dtype=F8), V=_t(2, 2, 96, 128, dtype=F8), kd=torch.ones(3)), r"k_descale: shape \(3,\), expected \(2,\)"),
    ("no lengths", dict(lens=None), "seqlens_k is required.*AFTER the append"),
    ("lengths list", dict(lens=[1, 2]), "seqlens_k must be an int32 device tensor.*got list"),
    ("lengths dtype", dict(lens=torch.zeros(2, dtype=torch.int64)), "seqlens_k: dtype torch.int64"),
    ("lengths shape", dict(lens=torch.zeros(3, dtype=torch.int32)), r"seqlens_k: shape \(3,\), expected \(2,\)"),
    ("lengths on the host", dict(), "seqlens_k is a CPU tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_contiguous_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Kn=KN, Vn=VN, K=_t(2, 2, 96, 128), V=_t(2, 2, 96, 128), lens=LENS, kd=None, vd=None)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        fa.kv_cache_append(a["Kn"], a["Vn"], a["K"], a["V"], a["lens"], a["kd"], a["vd"])


@pytest.mark.parametrize("what,kw,match", SOURCE + [
    ("K_pages rank", dict(K=_t(8, 32, 128)), r"K_pages: expected a 4-d tensor \[n_pages, H_kv, page_size, d\]"),
    ("K_pages heads", dict(K=_t(8, 3, 32, 128)), r"K_pages: shape .* does not match K_new.*\[n_pages, 2, page_size, 128\]"),
    ("no pages", dict(K=_t(0, 2, 32, 128), V=_t(0, 2, 32, 128)), "n_pages, page_size >= 1"),
    ("page_size 48", dict(K=_t(8, 2, 48, 128), V=_t(8, 2, 48, 128)), "K_pages: page_size 48 is not a multiple of 32"),
    ("V_pages shape", dict(V=_t(9, 2, 32, 128)), "V_pages: shape .* does not match K_pages"),
    ("fnuz", dict(K=_t(8, 2, 32, 128, dtype=torch.float8_e4m3fnuz)), "K_pages: dtype torch.float8_e4m3fnuz; an fp8 cache is OCP e4m3"),
    ("descale beside bf16", dict(vd=torch.ones(2)), "v_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("no lengths", dict(lens=None), "seqlens_k is required"),
    ("table list", dict(T=[[0, 1, 2]] * 2), "block_table must be an int32 device tensor.*got list"),
    ("table dtype", dict(T=torch.zeros(2, 3, dtype=torch.int64)), "block_table: dtype torch.int64"),
    ("table batch", dict(T=torch.zeros(3, 3, dtype=torch.int32)), r"block_table: shape \(3, 3\), expected \(2, max_pages\)"),
    ("table on the host", dict(), "block_table is a CPU tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_paged_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Kn=KN, Vn=VN, K=_t(8, 2, 32, 128), V=_t(8, 2, 32, 128), T=torch.zeros(2, 3, dtype=torch.int32), lens=LENS, kd=None, vd=None)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        fa.kv_cache_append_paged(a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["lens"], a["kd"], a["vd"])


def test_wrappers_are_exported_and_documented():
    import cuda_flashattention_amd as fa
    for f in (fa.kv_cache_append, fa.kv_cache_append_paged):
        assert "returns None" in f.__doc__ and "seqlens_k" in f.__doc__
    assert "AFTER the append" in fa.kv_cache_append.__doc__ and "clamp(-448, 448)" in fa.kv_cache_append.__doc__
    assert "ONE SEQUENCE EACH" in fa.kv_cache_append_paged.__doc__ and "DROPPED" in fa.kv_cache_append_paged.__doc__
    assert "kv_cache_append" in fa.flash_attention_2_decode.__doc__ and "kv_cache_append_paged" in fa.flash_attention_2_decode_paged.__doc__
