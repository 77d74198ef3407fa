"""CPU: the argument checks of the ragged rotary-embedding KV-cache append, without a GPU.
(i) include/fa2_rope_ragged_mi355x.h's symbols are exported by libfa2_mi355x.so and _capi.ROPE_RAGGED_SIGNATURES mirrors the header.
(ii) The status codes of fa2_rope_kv_append_ragged and fa2_rope_kv_append_ragged_paged, in the documented order, with pointers
that are never dereferenced (every one of them is decided before any HIP call); rot_dim = 0 with NULL tables and rot_dim = 0
with H_q > 0 are accepted; a plan too small or misaligned is FA2_ERR_WORKSPACE, the last of the table.
(iii) Every ValueError of the four wrappers that CPU tensors can reach, each naming its argument."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "fa2_rope_ragged_mi355x.h"


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", "", text, flags=re.M)
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))


def test_header_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    names = _declared(HEADER)
    assert names == ["fa2_rope_kv_append_ragged", "fa2_rope_kv_append_ragged_paged"]
    assert _capi.ROPE_RAGGED_HEADER_PATH == os.path.join(ROOT, "include", HEADER)
    lib = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/{HEADER} but not exported"
    assert sorted(_capi.ROPE_RAGGED_SIGNATURES) == names
    others = (_capi.SIGNATURES, _capi.KVCACHE_SIGNATURES, _capi.ROPE_SIGNATURES, _capi.EXTEND_SIGNATURES, _capi.EXTEND_RAGGED_SIGNATURES)
    assert not any(set(_capi.ROPE_RAGGED_SIGNATURES) & set(o) for o in others)
    bound = _capi.lib()
    for n, (res, args) in _capi.ROPE_RAGGED_SIGNATURES.items():
        assert list(getattr(bound, n).argtypes) == list(args) and getattr(bound, n).restype == res


def test_binding_table_equals_the_headers_declarations():
    from cuda_flashattention_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(_capi.ROPE_RAGGED_HEADER_PATH).read(), flags=re.S)
    for name, (res, args) in _capi.ROPE_RAGGED_SIGNATURES.items():
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
        assert m.group(1) == "int" and res is ctypes.c_int
        params = m.group(2).split(",")
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_longlong if "long long" in p else ctypes.c_size_t if "size_t" in p
                    else ctypes.c_int)
            assert a is want, (name, p.strip())


def test_the_headers_state_the_contract():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for words in ("SEMANTICS.", "THE PLAN.", "Q_OUT.", "STATUS CODES", "NOT COVERED", "THE PLAN IS THE SAFETY CONTRACT", "position_ids",
                  "tree masks", "token-major pools", "per-token scales", "a backward", "ONE SEQUENCE EACH", "rot_dim = 0", "+0.0 throughout",
                  "fa2_rope_ragged_owner.h", "kv_append_pos"):
        assert words in text, words
    # the three headers that named the hole now point here, their pinned phrases kept
    for header, phrase in (("fa2_kvcache_mi355x.h", "ragged n_new"), ("fa2_rope_mi355x.h", "ragged n_new"),
                           ("fa2_extend_ragged_mi355x.h", "ragged KV append")):
        other = open(os.path.join(ROOT, "include", header)).read()
        assert phrase in other and "NOT COVERED" in other and "fa2_rope_ragged_mi355x.h" in other, header


ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first
NULL, SHAPE, HEAD_DIM, DTYPE, UNSUPPORTED, WORKSPACE = -1, -2, -3, -4, -6, -5
BF16, F32, E4M3 = 0, 1, 2
BASE = dict(Q=ONE, Qo=ONE, Kn=ONE, Vn=ONE, K=ONE, V=ONE, cos=ONE, sin=ONE, plan=ONE, pb=(8 + 2 * 2) * 4, lens=ONE, kd=None, vd=None,
            B=2, Hq=4, H=2, n=5, d=128, rot=64, npos=96, il=0, qt=1024, qh=128, st=1024, sh=128, dtype=BF16, kv=BF16)


def _contiguous(lib, **kw):
    a = dict(BASE, cap=96)
    a.update(kw)
    return lib.fa2_rope_kv_append_ragged(a["Q"], a["Qo"], a["Kn"], a["Vn"], a["K"], a["V"], a["cos"], a["sin"], a["plan"], a["pb"], a["lens"],
                                         a["kd"], a["vd"], a["B"], a["Hq"], a["H"], a["n"], a["cap"], a["d"], a["rot"], a["npos"], a["il"],
                                         a["qt"], a["qh"], a["st"], a["sh"], a["dtype"], a["kv"], None)


def _paged(lib, **kw):
    a = dict(BASE, T=ONE, pages=8, P=32, mp=3)
    a.update(kw)
    return lib.fa2_rope_kv_append_ragged_paged(a["Q"], a["Qo"], a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["cos"], a["sin"], a["plan"],
                                               a["pb"], a["lens"], a["kd"], a["vd"], a["B"], a["Hq"], a["H"], a["n"], a["pages"], a["P"],
                                               a["mp"], a["d"], a["rot"], a["npos"], a["il"], a["qt"], a["qh"], a["st"], a["sh"],
                                               a["dtype"], a["kv"], None)


def test_status_values_are_the_librarys():
    from cuda_flashattention_amd import _capi
    s = lambda code: _capi.lib().fa2_status_string(code).decode().lower()
    assert "workspace" in s(WORKSPACE) and "null" in s(NULL) and "shape" in s(SHAPE)


# one invalid value per class of the status table, in the table's order
NULLS = [dict(Kn=None), dict(Vn=None), dict(K=None), dict(V=None), dict(lens=None), dict(plan=None), dict(cos=None), dict(sin=None),
         dict(Q=None), dict(Qo=None), dict(Q=None, Qo=None)]
SHAPES = [dict(B=0), dict(H=0), dict(n=0), dict(n=-1), dict(d=0), dict(Hq=-1), dict(Hq=3), dict(rot=8), dict(rot=24), dict(rot=144),
          dict(rot=-16), dict(npos=95), dict(npos=0), dict(il=2), dict(il=-1), dict(qt=-8), dict(qh=4), dict(st=12), dict(sh=-8),
          dict(Q=ctypes.c_void_p(24)), dict(Qo=ctypes.c_void_p(8)), dict(cos=ctypes.c_void_p(4)), dict(sin=ctypes.c_void_p(40)),
          dict(Kn=ctypes.c_void_p(24)), dict(Vn=ctypes.c_void_p(8)), dict(K=ctypes.c_void_p(4)), dict(V=ctypes.c_void_p(2)),
          dict(n=1 << 29, Hq=2, H=2), dict(n=1 << 30, Hq=0, H=2, Q=None, Qo=None)]
SHAPES_CONTIGUOUS = [dict(cap=0), dict(cap=1 << 25, kv=BF16), dict(cap=1 << 26, kv=E4M3)]
SHAPES_PAGED = [dict(pages=0), dict(P=0), dict(mp=0), dict(P=48), dict(P=16), dict(P=1 << 16, mp=1 << 15)]
LATER = [(dict(d=96), HEAD_DIM), (dict(dtype=F32), DTYPE), (dict(dtype=E4M3), DTYPE), (dict(kv=F32), DTYPE), (dict(kv=7), DTYPE),
         (dict(kd=ONE), UNSUPPORTED), (dict(vd=ONE), UNSUPPORTED), (dict(pb=47), WORKSPACE), (dict(plan=ctypes.c_void_p(24)), WORKSPACE)]


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
    # what passes every earlier check stops at the last one (pb = 47: no launch)
    stop = dict(pb=47)
    assert call(lib, **stop) == WORKSPACE and call(lib, pb=48, plan=ctypes.c_void_p(8)) == WORKSPACE
    assert call(lib, B=3, pb=(8 + 2 * 3) * 4 - 1) == WORKSPACE and call(lib, B=3, pb=(8 + 2 * 3) * 4, d=96) == HEAD_DIM
    # rot_dim = 0: no rotation, the tables may be NULL and n_positions is ignored, with Q heads or without
    assert call(lib, rot=0, cos=None, sin=None, npos=0, **stop) == WORKSPACE
    assert call(lib, rot=0, cos=None, sin=None, npos=-7, Hq=4, **stop) == WORKSPACE
    assert call(lib, rot=0, cos=ctypes.c_void_p(4), sin=None, npos=0, **stop) == WORKSPACE      # (ignored altogether)
    assert call(lib, rot=0, cos=None, sin=None, Q=None, Qo=None, Hq=0, **stop) == WORKSPACE     # the plain ragged append
    assert call(lib, rot=16, cos=None, sin=None) == NULL
    # the K/V-only form, both pair forms, full, partial and minimal rot_dim, tables longer than the cache, descales beside e4m3
    assert call(lib, Q=None, Qo=None, Hq=0, **stop) == WORKSPACE and call(lib, Hq=0, **stop) == WORKSPACE
    assert call(lib, il=1, **stop) == WORKSPACE and call(lib, rot=128, **stop) == WORKSPACE and call(lib, rot=16, **stop) == WORKSPACE
    assert call(lib, d=96, rot=112) == SHAPE and call(lib, d=64, rot=128) == SHAPE
    assert call(lib, npos=1 << 20, **stop) == WORKSPACE and call(lib, kv=E4M3, kd=ONE, vd=ONE, **stop) == WORKSPACE
    assert call(lib, qt=0, qh=0, st=0, sh=0, **stop) == WORKSPACE
    # (H_q + H_kv) x total_q fits an int, exactly
    assert call(lib, n=(1 << 31) // 6 + 1, Hq=4, H=2) == SHAPE and call(lib, n=((1 << 31) - 1) // 6, Hq=4, H=2, **stop) == WORKSPACE
    if call is _contiguous:
        assert call(lib, cap=97) == SHAPE and call(lib, cap=97, npos=97, **stop) == WORKSPACE       # n_positions >= kv_capacity
        assert call(lib, cap=97, rot=0, **stop) == WORKSPACE
    else:
        assert call(lib, mp=4) == SHAPE and call(lib, mp=4, npos=128, **stop) == WORKSPACE          # ... >= max_pages x page_size


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


def _fused(T=5, Hq=4, Hkv=2, d=128):
    """Q, K and V [T, H, d] views of one fused [T, H_q + 2 H_kv, d] projection output."""
    x = _t(T, Hq + 2 * Hkv, d)
    return x[:, :Hq], x[:, Hq:Hq + Hkv], x[:, Hq + Hkv:]


QV, KN, VN = _fused()
LENS = torch.zeros(2, dtype=torch.int32)
CU = torch.zeros(3, dtype=torch.int32)
COS, SIN = torch.zeros(96, 32), torch.zeros(96, 32)
F8 = torch.float8_e4m3fn


def _plan(B=2, Hq=4, Hkv=2, T=5):
    import cuda_flashattention_amd as fa
    return fa.ExtendRaggedPlan(torch.zeros(64, dtype=torch.int32), B, Hq, Hkv, T)


SHARED = [
    ("K_new rank", dict(Kn=_t(2, 2, 5, 128)), r"K_new: expected a 3-d tensor \[T, H_kv, d\] \(token-major\).*fused"),
    ("V_new dtype", dict(Vn=_t(5, 2, 128, dtype=torch.float16)), "V_new: dtype torch.float16, expected torch.bfloat16"),
    ("V_new shape", dict(Vn=_t(5, 3, 128)), "V_new: shape .* does not match K_new"),
    ("head_dim", dict(Kn=_t(5, 2, 96), Vn=_t(5, 2, 96)), "K_new: head_dim 96, expected 64 or 128"),
    ("strides differ", dict(Vn=_t(5, 2, 128)), "V_new: strides .* differ from K_new's"),
    ("K_new last stride", dict(Kn=_t(5, 2, 256)[..., ::2]), r"K_new: stride .*stride\(-1\) == 1"),
    ("K_new offset", dict(Kn=_t(5, 2, 136)[..., 4:132]), "K_new: storage offset 4 elements is not 16-byte aligned"),
    ("Q rank", dict(Q=_t(1, 5, 4, 128)), r"Q: expected a 3-d tensor \[T, H_q, d\]"),
    ("Q no tensor", dict(Q=[1.0]), "Q: expected a 3-d tensor.*got list"),
    ("Q dtype", dict(Q=_t(5, 4, 128, dtype=torch.float32)), "Q: dtype torch.float32, expected torch.bfloat16"),
    ("Q tokens", dict(Q=_t(4, 4, 128)), r"Q: shape .* does not match K_new.*\[5, H_q, 128\]"),
    ("Q head_dim", dict(Q=_t(5, 4, 64)), "Q: shape .* does not match K_new"),
    ("Q heads", dict(Q=_t(5, 3, 128)), "Q: shape .* H_kv = 2 dividing H_q"),
    ("Q stride not 8n", dict(Q=_t(5, 4, 132)[..., :128]), "Q: strides .* multiples of 8 elements"),
    ("one table", dict(sin=None), "cos and sin come as a pair"),
    ("cos rank", dict(cos=torch.zeros(96)), r"cos: expected a 2-d tensor \[n_positions, rot_dim / 2\]"),
    ("cos dtype", dict(cos=torch.zeros(96, 32, dtype=torch.float64)), "cos: dtype torch.float64, expected torch.float32"),
    ("sin shape", dict(sin=torch.zeros(96, 16)), "sin: shape .* does not match cos"),
    ("rot_dim 24", dict(cos=torch.zeros(96, 12), sin=torch.zeros(96, 12)), "cos: shape .* rot_dim of 24, expected a multiple of 16"),
    ("interleaved", dict(il=1), "interleaved: 1, expected a bool"),
    ("no lengths", dict(lens=None, cu="plan"), "seqlens_k is required.*AFTER the"),
    ("cu a list", dict(cu=[0, 2, 5]), "cu_seqlens_q must be an int32 device tensor.*got list"),
    ("cu dtype", dict(cu=torch.zeros(3, dtype=torch.int64)), "cu_seqlens_q: dtype torch.int64"),
    ("cu on the host", dict(), "cu_seqlens_q is a CPU tensor"),
    ("Q_out without Q", dict(Q=None, Qo=_t(5, 4, 128)), "Q_out: given without Q"),
    ("plan for another T", dict(cu="plan T"), "plan: built for H_q / H_kv = 2 and total_q = 6; this step has H_q / H_kv = 2 and total_q = 5"),
    ("plan for another G", dict(cu="plan G"), "plan: built for H_q / H_kv = 1 and total_q = 5"),
]


def _args(a):
    if a["cu"] == "plan":
        a["cu"] = _plan()
    elif a["cu"] == "plan T":
        a["cu"] = _plan(T=6)
    elif a["cu"] == "plan G":
        a["cu"] = _plan(Hq=2)
    return a


@pytest.mark.parametrize("what,kw,match", SHARED + [
    ("K_cache rank", dict(K=_t(2, 96, 128)), r"K_cache: expected a 4-d tensor \[B, H_kv, N_cap, d\]"),
    ("K_cache heads", dict(K=_t(2, 3, 96, 128)), "K_cache: shape .* does not match K_new"),
    ("K_cache batch", dict(K=_t(3, 2, 96, 128), V=_t(3, 2, 96, 128), cu="plan"), r"K_cache: 3 sequences, cu_seqlens_q \(the plan\) has 2"),
    ("V_cache shape", dict(V=_t(2, 2, 64, 128)), "V_cache: shape .* does not match K_cache"),
    ("e5m2", dict(K=_t(2, 2, 96, 128, dtype=torch.float8_e5m2)), "K_cache: dtype torch.float8_e5m2; an fp8 cache is OCP e4m3"),
    ("mixed", dict(V=_t(2, 2, 96, 128, dtype=F8)), "V_cache: dtype torch.float8_e4m3fn beside K_cache torch.bfloat16"),
    ("descale beside bf16", dict(kd=torch.ones(2)), "k_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("descale shape", dict(K=_t(2, 2, 96, 128, dtype=F8), V=_t(2, 2, 96, 128, dtype=F8), kd=torch.ones(3)), r"k_descale: shape \(3,\), expected \(2,\)"),
    ("too few positions", dict(cos=torch.zeros(95, 32), sin=torch.zeros(95, 32), cu="plan"), "cos: 95 positions for a cache of 96 rows"),
    ("lengths dtype", dict(lens=torch.zeros(2, dtype=torch.int64), cu="plan"), "seqlens_k: dtype torch.int64"),
    ("lengths count", dict(lens=torch.zeros(3, dtype=torch.int32), cu="plan"), r"seqlens_k: shape \(3,\), expected \(2,\)"),
    ("lengths on the host", dict(cu="plan"), "seqlens_k is a CPU tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_contiguous_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Q=QV, Kn=KN, Vn=VN, K=_t(2, 2, 96, 128), V=_t(2, 2, 96, 128), cos=COS, sin=SIN, cu=CU, lens=LENS, il=False, kd=None, vd=None,
             Qo=None)
    a.update(kw)
    a = _args(a)
    with pytest.raises(ValueError, match=match):
        fa.rope_kv_cache_append_ragged(a["Q"], a["Kn"], a["Vn"], a["K"], a["V"], a["cos"], a["sin"], a["cu"], a["lens"],
                                       interleaved=a["il"], k_descale=a["kd"], v_descale=a["vd"], Q_out=a["Qo"])


@pytest.mark.parametrize("what,kw,match", SHARED + [
    ("K_pages rank", dict(K=_t(8, 32, 128)), r"K_pages: expected a 4-d tensor \[n_pages, H_kv, page_size, d\]"),
    ("K_pages heads", dict(K=_t(8, 3, 32, 128)), "K_pages: shape .* does not match K_new"),
    ("page_size 48", dict(K=_t(8, 2, 48, 128), V=_t(8, 2, 48, 128)), "K_pages: page_size 48 is not a multiple of 32"),
    ("V_pages shape", dict(V=_t(9, 2, 32, 128)), "V_pages: shape .* does not match K_pages"),
    ("fnuz", dict(K=_t(8, 2, 32, 128, dtype=torch.float8_e4m3fnuz)), "K_pages: dtype torch.float8_e4m3fnuz; an fp8 cache is OCP e4m3"),
    ("descale beside bf16", dict(vd=torch.ones(2)), "v_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("no table", dict(T=None), "block_table must be an int32 device tensor"),
    ("table list", dict(T=[[0, 1, 2]] * 2, cu="plan"), "block_table must be an int32 device tensor.*got list"),
    ("table dtype", dict(T=torch.zeros(2, 3, dtype=torch.int64), cu="plan"), "block_table: dtype torch.int64"),
    ("table batch", dict(T=torch.zeros(3, 3, dtype=torch.int32), cu="plan"), r"block_table: shape \(3, 3\), expected \(2, max_pages\)"),
    ("table on the host", dict(cu="plan"), "block_table is a CPU tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_paged_wrapper_refuses(what, kw, match):
    import cuda_flashattention_amd as fa
    a = dict(Q=QV, Kn=KN, Vn=VN, K=_t(8, 2, 32, 128), V=_t(8, 2, 32, 128), T=torch.zeros(2, 3, dtype=torch.int32), cos=COS, sin=SIN,
             cu=CU, lens=LENS, il=False, kd=None, vd=None, Qo=None)
    a.update(kw)
    a = _args(a)
    with pytest.raises(ValueError, match=match):
        fa.rope_kv_cache_append_ragged_paged(a["Q"], a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["cos"], a["sin"], a["cu"], a["lens"],
                                             interleaved=a["il"], k_descale=a["kd"], v_descale=a["vd"], Q_out=a["Qo"])


def test_plain_ragged_append_wrappers_refuse():
    """kv_cache_append_ragged / _paged are the same checks without Q and tables."""
    import cuda_flashattention_amd as fa
    K, V = _t(2, 2, 96, 128), _t(2, 2, 96, 128)
    with pytest.raises(ValueError, match=r"K_new: expected a 3-d tensor \[T, H_kv, d\]"):
        fa.kv_cache_append_ragged(_t(2, 2, 5, 128), VN, K, V, CU, LENS)
    with pytest.raises(ValueError, match="cu_seqlens_q is a CPU tensor"):
        fa.kv_cache_append_ragged(KN, VN, K, V, CU, LENS)
    with pytest.raises(ValueError, match="seqlens_k is a CPU tensor"):
        fa.kv_cache_append_ragged(KN, VN, K, V, _plan(Hq=8, Hkv=1), LENS)          # a plan of any G serves a K/V-only call
    with pytest.raises(ValueError, match="plan: built for .* total_q = 6; this step has total_q = 5"):
        fa.kv_cache_append_ragged(KN, VN, K, V, _plan(T=6), LENS)
    with pytest.raises(ValueError, match="block_table must be an int32 device tensor"):
        fa.kv_cache_append_ragged_paged(KN, VN, _t(8, 2, 32, 128), _t(8, 2, 32, 128), None, CU, LENS)
    with pytest.raises(ValueError, match="block_table is a CPU tensor"):
        fa.kv_cache_append_ragged_paged(KN, VN, _t(8, 2, 32, 128), _t(8, 2, 32, 128), torch.zeros(2, 3, dtype=torch.int32), _plan(), LENS)


def test_wrappers_are_exported_and_documented():
    import cuda_flashattention_amd as fa
    for f in (fa.rope_kv_cache_append_ragged, fa.rope_kv_cache_append_ragged_paged, fa.kv_cache_append_ragged, fa.kv_cache_append_ragged_paged):
        assert f.__doc__ and "ragged" in f.__doc__
    doc = fa.rope_kv_cache_append_ragged.__doc__
    for words in ("returns Q_out", "extend_ragged_plan", "flash_attention_2_extend_ragged(Q_out", "+0.0 throughout", "never reads cu_seqlens_q",
                  "cos = sin = None", "leave without a store"):
        assert words in doc, words
    assert "ONE SEQUENCE EACH" in fa.rope_kv_cache_append_ragged_paged.__doc__ and "DROPPED" in fa.rope_kv_cache_append_ragged_paged.__doc__
