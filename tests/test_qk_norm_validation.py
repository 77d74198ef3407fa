"""CPU: the argument checks of the ragged rotary append with a per-head QK RMSNorm, without a GPU.
(i) include/fa2_rope_norm_mi355x.h's symbols are exported by libfa2_mi355x.so and _capi.ROPE_NORM_SIGNATURES mirrors the header.
(ii) The status codes of fa2_norm_rope_kv_append_ragged and fa2_norm_rope_kv_append_ragged_paged: the sibling's classes in the
sibling's order (tests/test_rope_ragged_validation.py holds the sibling's own table, reused here value for value), with a NULL
k_weight or a NULL q_weight beside Q heads among the NULL pointers, and eps zero, negative, infinite or NaN or a misaligned weight
among the shapes.  No pointer is ever dereferenced: every status is decided before any HIP call.
(iii) The ValueErrors of the two wrappers: the sibling's (they share its checks) and the weights' and eps's own."""
import ctypes
import math
import os
import re

import pytest
import torch

import test_rope_ragged_validation as sib

ROOT = sib.ROOT
HEADER = "fa2_rope_norm_mi355x.h"
ONE, NULL, SHAPE, HEAD_DIM, DTYPE, UNSUPPORTED, WORKSPACE = sib.ONE, sib.NULL, sib.SHAPE, sib.HEAD_DIM, sib.DTYPE, sib.UNSUPPORTED, sib.WORKSPACE
BASE = dict(sib.BASE, qw=ONE, kw=ONE, eps=1e-6)


def test_header_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    names = sib._declared(HEADER)
    assert names == ["fa2_norm_rope_kv_append_ragged", "fa2_norm_rope_kv_append_ragged_paged"]
    assert _capi.ROPE_NORM_HEADER_PATH == os.path.join(ROOT, "include", HEADER)
    lib = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/{HEADER} but not exported"
    assert sorted(_capi.ROPE_NORM_SIGNATURES) == names
    others = (_capi.SIGNATURES, _capi.KVCACHE_SIGNATURES, _capi.ROPE_SIGNATURES, _capi.EXTEND_SIGNATURES, _capi.EXTEND_RAGGED_SIGNATURES,
              _capi.ROPE_RAGGED_SIGNATURES)
    assert not any(set(_capi.ROPE_NORM_SIGNATURES) & set(o) for o in others)
    bound = _capi.lib()
    for n, (res, args) in _capi.ROPE_NORM_SIGNATURES.items():
        assert list(getattr(bound, n).argtypes) == list(args) and getattr(bound, n).restype == res


def _params(path, name):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^;{]*)\)\s*;", text)
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_binding_table_equals_the_headers_declarations():
    from cuda_flashattention_amd import _capi
    for name, (res, args) in _capi.ROPE_NORM_SIGNATURES.items():
        ret, params = _params(_capi.ROPE_NORM_HEADER_PATH, name)
        assert ret == "int" and res is ctypes.c_int
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_longlong if "long long" in p else ctypes.c_size_t if "size_t" in p
                    else ctypes.c_float if p.startswith("float ") else ctypes.c_int)
            assert a is want, (name, p)


def test_the_declarations_are_the_siblings_with_three_additions_behind_sin_table():
    from cuda_flashattention_amd import _capi
    for name in _capi.ROPE_NORM_SIGNATURES:
        _, mine = _params(_capi.ROPE_NORM_HEADER_PATH, name)
        _, theirs = _params(_capi.ROPE_RAGGED_HEADER_PATH, name.replace("fa2_norm_rope", "fa2_rope"))
        at = theirs.index("const float* sin_table") + 1
        assert mine == theirs[:at] + ["const float* q_weight", "const float* k_weight", "float eps"] + theirs[at:], name


def test_the_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for words in ("SEMANTICS.", "ARITHMETIC.", "STATUS CODES", "NOT COVERED", "THE CALLER BUILDS THE WEIGHTS", "(1 + w)", "Gemma 3's form",
                  "HF Qwen3's", "all-bf16 rotation", "left to right", "lane ^ m", "correctly rounded", "ONE rounding to bf16",
                  "BIT FOR BIT fa2_rope_kv_append_ragged", "stores n itself", "V is copied untouched", "fa2_rope_ragged_owner.h",
                  "fa2_kv_append_addr.h", "+0.0 throughout", "ONE SEQUENCE EACH", "the plan is the safety contract",
                  "the butterfly runs on every lane", "NULL only when H_q == 0"):
        assert words in text, words
    # the sibling's header, which named no norm, now points here
    other = open(os.path.join(ROOT, "include", "fa2_rope_ragged_mi355x.h")).read()
    assert "fa2_rope_norm_mi355x.h" in other[other.index("NOT COVERED"):]


def _contiguous(lib, **kw):
    a = dict(BASE, cap=96)
    a.update(kw)
    return lib.fa2_norm_rope_kv_append_ragged(a["Q"], a["Qo"], a["Kn"], a["Vn"], a["K"], a["V"], a["cos"], a["sin"], a["qw"], a["kw"], a["eps"],
                                              a["plan"], a["pb"], a["lens"], a["kd"], a["vd"], a["B"], a["Hq"], a["H"], a["n"], a["cap"], a["d"],
                                              a["rot"], a["npos"], a["il"], a["qt"], a["qh"], a["st"], a["sh"], a["dtype"], a["kv"], None)


def _paged(lib, **kw):
    a = dict(BASE, T=ONE, pages=8, P=32, mp=3)
    a.update(kw)
    return lib.fa2_norm_rope_kv_append_ragged_paged(a["Q"], a["Qo"], a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["cos"], a["sin"], a["qw"],
                                                    a["kw"], a["eps"], a["plan"], a["pb"], a["lens"], a["kd"], a["vd"], a["B"], a["Hq"], a["H"],
                                                    a["n"], a["pages"], a["P"], a["mp"], a["d"], a["rot"], a["npos"], a["il"], a["qt"], a["qh"],
                                                    a["st"], a["sh"], a["dtype"], a["kv"], None)


NULLS = sib.NULLS + [dict(kw=None), dict(qw=None, Hq=4), dict(qw=None, Hq=2), dict(qw=None, kw=None), dict(kw=None, Q=None, Qo=None, Hq=0)]
SHAPES = sib.SHAPES + [dict(eps=0.0), dict(eps=-1e-6), dict(eps=math.inf), dict(eps=-math.inf), dict(eps=math.nan), dict(eps=-0.0),
                       dict(qw=ctypes.c_void_p(24)), dict(kw=ctypes.c_void_p(4)), dict(kw=ctypes.c_void_p(40))]


@pytest.mark.parametrize("call,shapes", ((_contiguous, sib.SHAPES_CONTIGUOUS), (_paged, sib.SHAPES_PAGED)), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, shapes):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    nulls = NULLS + ([dict(T=None)] if call is _paged else [])
    for kw in nulls:
        assert call(lib, **kw) == NULL, kw
    for kw in SHAPES + shapes:
        assert call(lib, **kw) == SHAPE, kw
    for kw, status in sib.LATER:
        assert call(lib, **kw) == status, kw
    # the order: an earlier class wins over every later one
    later = [kw for kw, _ in sib.LATER]
    for first, status, rest in ((nulls, NULL, SHAPES + shapes + later), (SHAPES + shapes, SHAPE, later)):
        for a in first:
            for b in rest:
                if not set(a) & set(b):
                    assert call(lib, **a, **b) == status, (a, b)
    for i, (a, status) in enumerate(sib.LATER):
        for b in later[i + 1:]:
            if not set(a) & set(b):
                assert call(lib, **a, **b) == status, (a, b)
    # what passes every earlier check stops at the last one (pb = 47: no launch)
    stop = dict(pb=47)
    assert call(lib, **stop) == WORKSPACE and call(lib, pb=48, plan=ctypes.c_void_p(8)) == WORKSPACE
    # a K/V-only call needs no q_weight; with Q heads it does; eps is any finite positive float, a denormal one included
    assert call(lib, Q=None, Qo=None, Hq=0, qw=None, **stop) == WORKSPACE and call(lib, Q=None, Qo=None, Hq=0, **stop) == WORKSPACE
    assert call(lib, Hq=0, qw=None, **stop) == WORKSPACE      # (Q given with H_q = 0: no Q heads, no weight needed)
    assert call(lib, eps=1e-45, **stop) == WORKSPACE and call(lib, eps=3.0e38, **stop) == WORKSPACE and call(lib, eps=1e-46) == SHAPE
    # the sibling's accepted forms stay accepted
    assert call(lib, rot=0, cos=None, sin=None, npos=-7, **stop) == WORKSPACE and call(lib, rot=16, cos=None, sin=None) == NULL
    assert call(lib, il=1, rot=128, **stop) == WORKSPACE and call(lib, kv=sib.E4M3, kd=ONE, vd=ONE, **stop) == WORKSPACE
    assert call(lib, d=96, **stop) == HEAD_DIM and call(lib, d=96, eps=0.0) == SHAPE and call(lib, d=96, kw=None) == NULL


QV, KN, VN, LENS, CU, COS, SIN = sib.QV, sib.KN, sib.VN, sib.LENS, sib.CU, sib.COS, sib.SIN
W = torch.ones(128)

OWN = [
    ("q_weight none", dict(qw=None), r"q_weight: expected a 1-d tensor \[128\].*got NoneType"),
    ("q_weight list", dict(qw=[1.0] * 128), r"q_weight: expected a 1-d tensor \[128\].*got list"),
    ("q_weight length", dict(qw=torch.ones(64)), r"q_weight: expected a 1-d tensor \[128\].*got \(64,\)"),
    ("k_weight rank", dict(kw=torch.ones(1, 128)), r"k_weight: expected a 1-d tensor \[128\]"),
    ("k_weight dtype", dict(kw=torch.ones(128, dtype=torch.bfloat16)), "k_weight: dtype torch.bfloat16, expected torch.float32.*1 \\+ w"),
    ("q_weight dtype", dict(qw=torch.ones(128, dtype=torch.float64)), "q_weight: dtype torch.float64, expected torch.float32"),
    ("k_weight strided", dict(kw=torch.ones(256)[::2]), "k_weight must be contiguous"),
    ("q_weight offset", dict(qw=torch.ones(130)[2:]), "q_weight: storage offset 2 elements is not 16-byte aligned"),
    ("q_weight without Q", dict(Q=None), "q_weight: given without Q"),
    ("eps zero", dict(eps=0.0), "eps: 0.0, expected a finite float > 0"),
    ("eps negative", dict(eps=-1e-6), "eps: -1e-06, expected a finite float > 0"),
    ("eps inf", dict(eps=math.inf), "eps: inf, expected a finite float > 0"),
    ("eps nan", dict(eps=math.nan), "eps: nan, expected a finite float > 0"),
    ("eps none", dict(eps=None), "eps: None, expected a finite float > 0"),
    ("eps zero as float32", dict(eps=1e-46), "eps: 1e-46, expected a finite float > 0"),
    ("eps inf as float32", dict(eps=1e39), r"eps: 1e\+39, expected a finite float > 0"),
    ("eps huge int", dict(eps=10 ** 400), "eps: 1000.*expected a finite float > 0"),
    ("eps tensor", dict(eps=torch.tensor(1e-6)), "eps: .*expected a finite float > 0"),
    # the weights pass, the sibling's next check speaks
    ("weights pass", dict(), "cu_seqlens_q is a CPU tensor"),
    ("k only passes", dict(Q=None, qw=None), "cu_seqlens_q is a CPU tensor"),
]


def _call(paged, a):
    import cuda_flashattention_amd as fa
    a = sib._args(a)
    if paged:
        return fa.norm_rope_kv_cache_append_ragged_paged(a["Q"], a["Kn"], a["Vn"], a["K"], a["V"], a["T"], a["cos"], a["sin"], a["qw"], a["kw"],
                                                         a["eps"], a["cu"], a["lens"], interleaved=a["il"], k_descale=a["kd"],
                                                         v_descale=a["vd"], Q_out=a["Qo"])
    return fa.norm_rope_kv_cache_append_ragged(a["Q"], a["Kn"], a["Vn"], a["K"], a["V"], a["cos"], a["sin"], a["qw"], a["kw"], a["eps"],
                                               a["cu"], a["lens"], interleaved=a["il"], k_descale=a["kd"], v_descale=a["vd"], Q_out=a["Qo"])


@pytest.mark.parametrize("paged", (False, True), ids=("contiguous", "paged"))
@pytest.mark.parametrize("what,kw,match", OWN + sib.SHARED, ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_wrappers_refuse(what, kw, match, paged):
    shape = (8, 2, 32, 128) if paged else (2, 2, 96, 128)
    a = dict(Q=QV, Kn=KN, Vn=VN, K=sib._t(*shape), V=sib._t(*shape), T=torch.zeros(2, 3, dtype=torch.int32), cos=COS, sin=SIN, qw=W, kw=W,
             eps=1e-6, cu=CU, lens=LENS, il=False, kd=None, vd=None, Qo=None)
    a.update(kw)
    if a["Q"] is None and "qw" not in kw and what != "q_weight without Q":
        a["qw"] = None      # (a sibling's case without Q: a K/V-only call has no q_weight either)
    with pytest.raises(ValueError, match=match):
        _call(paged, a)


def test_the_paged_wrapper_needs_a_table():
    a = dict(Q=QV, Kn=KN, Vn=VN, K=sib._t(8, 2, 32, 128), V=sib._t(8, 2, 32, 128), T=None, cos=COS, sin=SIN, qw=W, kw=W, eps=1e-6, cu=CU,
             lens=LENS, il=False, kd=None, vd=None, Qo=None)
    with pytest.raises(ValueError, match="block_table must be an int32 device tensor"):
        _call(True, a)


def test_wrappers_are_exported_and_documented():
    import cuda_flashattention_amd as fa
    doc = fa.norm_rope_kv_cache_append_ragged.__doc__
    for words in ("RMSNorm", "q_weight, k_weight: fp32 [d]", "1 + w", "Gemma 3's form", "HF Qwen3's", "bit for bit", "V is copied untouched",
                  "cos = sin = None stores n itself", "+0.0 throughout"):
        assert words in doc, words
    assert "ONE SEQUENCE EACH" in fa.norm_rope_kv_cache_append_ragged_paged.__doc__ and "DROPPED" in fa.norm_rope_kv_cache_append_ragged_paged.__doc__
