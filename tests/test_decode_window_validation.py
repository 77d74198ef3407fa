"""CPU: the argument checks of the windowed decode, without a GPU.
(i) The three new symbols are declared in include/fa2_mi355x.h, exported by libfa2_mi355x.so and bound by _capi.SIGNATURES with the
header's argument lists (the siblings' plus a trailing int window_left).
(ii) The status codes of fa2_forward_decode_window and fa2_forward_decode_paged_window, the siblings' in their order, with pointers
that are never dereferenced: window_left < -1 is the last shape check, a window without `causal` is reported where M > 32 is.
(iii) fa2_decode_window_num_splits against the rule: fa2_decode_num_splits on min(kv_capacity, window_left + q_len + 127), and
fa2_decode_num_splits itself where the window is absent or at least kv_capacity - 1.
(iv) The wrappers' ValueErrors for a negative window, a window with causal=False and a non-int; None is today's call."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import decode_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fa2_decode_window_num_splits", "fa2_forward_decode_window", "fa2_forward_decode_paged_window")
INT_MAX = 2 ** 31 - 1
BF16, F32, E4M3 = 0, 1, 2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa2_mi355x.h")).read(), flags=re.S)


def _params(text, name):
    return [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text = _header()
    so = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    bound = _capi.lib()
    for name in NEW:
        assert hasattr(so, name), f"{name} not exported"
        res, args = _capi.SIGNATURES[name]
        params = _params(text, name)
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_float if "float" in p else ctypes.c_int
            assert a is want, (name, p)
        assert res is ctypes.c_int
        assert list(getattr(bound, name).argtypes) == list(args)
    # the siblings' lists plus a trailing window_left
    for name, sibling in (("fa2_forward_decode_window", "fa2_forward_decode_fp8kv"),
                          ("fa2_forward_decode_paged_window", "fa2_forward_decode_paged_fp8kv")):
        assert _params(text, name) == _params(text, sibling) + ["int window_left"]
        assert _capi.SIGNATURES[name][1] == _capi.SIGNATURES[sibling][1] + [ctypes.c_int]


def test_header_describes_the_contract():
    text = open(os.path.join(ROOT, "include", "fa2_mi355x.h")).read()
    block = text[text.index("Decode with a sliding window"):text.index("int fa2_decode_window_num_splits")]
    for phrase in ("BEFORE THE WINDOW", "NOT COVERED", "window_left = 127", "never read", "FA2_ERR_UNSUPPORTED"):
        assert phrase in block, phrase


ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first


def _contiguous(lib, ptrs=None, **kw):
    a = dict(B=1, Hq=8, Hkv=2, q=1, cap=4096, d=128, scale=0.125, dtype=BF16, kv=BF16, causal=1, ns=1, ws=None, wsb=0, wl=127,
             kd=None, vd=None)
    a.update(kw)
    p = list(ptrs or (ONE, ONE, ONE, None, None, a["kd"], a["vd"], ONE, ONE))
    return lib.fa2_forward_decode_window(*p, a["B"], a["Hq"], a["Hkv"], a["q"], a["cap"], a["d"], a["scale"], a["dtype"], a["kv"],
                                         a["causal"], a["ns"], a["ws"], a["wsb"], None, a["wl"])


def _paged(lib, ptrs=None, **kw):
    a = dict(B=1, Hq=8, Hkv=2, q=1, pages=100, P=64, mp=64, d=128, scale=0.125, dtype=BF16, kv=BF16, causal=1, ns=1, ws=None, wsb=0,
             wl=127, kd=None, vd=None)
    a.update(kw)
    if "cap" in a:
        a["mp"] = a.pop("cap") // a["P"]
    p = list(ptrs or (ONE, ONE, ONE, ONE, None, None, a["kd"], a["vd"], ONE, ONE))
    return lib.fa2_forward_decode_paged_window(*p, a["B"], a["Hq"], a["Hkv"], a["q"], a["pages"], a["P"], a["mp"], a["d"], a["scale"],
                                               a["dtype"], a["kv"], a["causal"], a["ns"], a["ws"], a["wsb"], None, a["wl"])


@pytest.mark.parametrize("call,required", ((_contiguous, (0, 1, 2, 7, 8)), (_paged, (0, 1, 2, 3, 8, 9))), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, required):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    n_ptrs = 9 if call is _contiguous else 10
    for missing in required:      # Q, K, V, (block_table,) O, L: NULL comes before everything else
        ptrs = [ONE] * n_ptrs
        ptrs[missing] = None
        assert call(lib, tuple(ptrs), B=0, d=96, dtype=7, wl=-5) == -1, missing
    # shapes, window_left < -1 among them, before head_dim, dtype, workspace and the refusals
    shapes = [dict(B=0), dict(Hq=0), dict(Hkv=3), dict(q=0), dict(scale=0.0), dict(ns=-1), dict(ns=257), dict(wl=-2), dict(wl=-INT_MAX - 1)]
    shapes += [dict(cap=0)] if call is _contiguous else [dict(pages=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15)]
    for bad in shapes:
        assert call(lib, **dict(dict(d=96, dtype=7, causal=0, kd=ONE), **bad)) == -2, bad
    if call is _contiguous:      # the slab limit follows the caches' element size, as in the siblings
        assert call(lib, cap=1 << 23, d=128) == -2 and call(lib, cap=(1 << 23) - 1, d=128, dtype=7) == -4
        assert call(lib, cap=1 << 24, d=128, kv=E4M3) == -2 and call(lib, cap=(1 << 24) - 1, d=128, kv=E4M3, dtype=7) == -4
        assert call(lib, cap=1 << 23, d=128, kv=E4M3, dtype=7) == -4
    assert call(lib, d=96, dtype=7, causal=0) == -3                      # head_dim before dtype
    for kw in (dict(dtype=F32), dict(dtype=E4M3), dict(kv=F32), dict(kv=7), dict(kd=ONE), dict(vd=ONE)):      # a descale beside bf16 caches
        assert call(lib, **dict(kw, ns=4, q=64, causal=0)) == -4, kw     # dtype before the workspace and the refusals
    assert call(lib, kv=E4M3, kd=ONE, vd=ONE, ns=4, q=64) == -5          # descales belong to e4m3 caches
    need = lib.fa2_decode_workspace_bytes(1, 8, 2, 1, 4096, 128, 4)
    assert need > 0
    assert call(lib, ns=4, q=64, causal=0) == -5                         # the workspace before the refusals
    assert call(lib, ns=4, ws=ONE, wsb=need - 1) == -5
    assert call(lib, ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    # n_splits = 0 resolves by the window's rule: 127 + 1 + 127 keys are one split and need no workspace (q = 9: the call goes on to
    # the row limit); the plain rule -- window -1, or at least the capacity - 1 -- gives 16 splits of a capacity of 4096
    assert call(lib, ns=0, q=9) == -6
    for wl in (-1, 4095, 4096, INT_MAX):
        assert call(lib, ns=0, q=9, wl=wl) == -5, wl
    assert call(lib, ns=0, q=9, wl=4094) == -5 and lib.fa2_decode_window_num_splits(1, 2, 9, 4096, 128, 4094) == 16
    # the refusals: M > 32, then a window without causal
    assert call(lib, q=9) == -6 and call(lib, Hq=64, Hkv=1) == -6
    assert call(lib, causal=0) == -6 and call(lib, causal=0, wl=0) == -6 and call(lib, causal=0, wl=INT_MAX) == -6
    assert call(lib, causal=0, wl=0, kv=E4M3, kd=ONE) == -6


def test_window_num_splits_follows_the_rule():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    for B, hkv, q, cap, d in ((1, 8, 1, 131072, 128), (8, 8, 1, 8192, 128), (64, 8, 1, 2048, 128), (1, 1, 4, 4096, 64), (9, 2, 4, 1024, 64),
                              (1, 2, 1, 300, 128), (3, 1, 32, 100000, 64)):
        plain = lib.fa2_decode_num_splits(B, hkv, cap, d)
        c = dict(lens=(0,) * B, hkv=hkv, ncap=cap)
        assert plain == dr.resolved_splits(c, 0)
        for wl in (-1, 0, 1, 31, 127, 128, 200, 1000, 4095, cap - 2, cap - 1, cap, cap + 1, INT_MAX):
            got = lib.fa2_decode_window_num_splits(B, hkv, q, cap, d, wl)
            if wl < 0 or wl >= cap - 1:
                assert got == plain, (B, hkv, q, cap, wl)
            else:
                keys = min(cap, wl + q + 127)
                assert got == lib.fa2_decode_num_splits(B, hkv, keys, d) == dr.resolved_splits(dict(c, ncap=keys), 0), (B, hkv, q, cap, wl)
                assert got <= plain
    assert lib.fa2_decode_window_num_splits(1, 8, 1, 131072, 128, 127) == 1            # 255 keys: one split
    assert lib.fa2_decode_window_num_splits(1, 8, 1, 131072, 128, 4095) == 16          # 4223 keys: 16 splits of 256 and more
    assert lib.fa2_decode_window_num_splits(0, 8, 1, 1024, 128, 127) == 1 and lib.fa2_decode_window_num_splits(1, 8, 1, 0, 128, 127) == 1


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


@pytest.mark.parametrize("what,kw,match", [
    ("negative", dict(window_left=-1), "window_left: -1, expected an int >= 0, or None"),
    ("float", dict(window_left=127.0), "window_left: 127.0, expected an int >= 0"),
    ("bool", dict(window_left=True), "window_left: True, expected an int"),
    ("tensor", dict(window_left=torch.tensor(3)), "window_left: .*expected an int"),
    ("not causal", dict(window_left=127, causal=False), "window_left: 127 with causal=False; the window is a causal one"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_wrappers_refuse(what, kw, match):
    import cuda_flashattention_amd as fa
    with pytest.raises(ValueError, match=match):
        fa.flash_attention_2_decode(_t(2, 8, 1, 128), _t(2, 2, 256, 128), _t(2, 2, 256, 128), **kw)
    with pytest.raises(ValueError, match=match):
        fa.flash_attention_2_decode_paged(_t(2, 8, 1, 128), _t(12, 2, 64, 128), _t(12, 2, 64, 128), torch.zeros(2, 5, dtype=torch.int32), **kw)
    if "causal" not in kw:
        with pytest.raises(ValueError, match=match):
            fa.decode_num_splits(2, 2, 256, 128, q_len=1, **kw)
        with pytest.raises(ValueError, match=match):
            fa.decode_workspace(2, 8, 2, 1, 256, 128, 0, device="cpu", **kw)


def test_wrappers_keywords_and_helpers():
    import cuda_flashattention_amd as fa
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    for f in (fa.flash_attention_2_decode, fa.flash_attention_2_decode_paged):
        p = inspect.signature(f).parameters["window_left"]
        assert p.default is None
        assert "SLIDING WINDOW" in f.__doc__ and "BEFORE THE WINDOW" in f.__doc__
    for f in (fa.decode_num_splits, fa.decode_workspace):
        sig = inspect.signature(f).parameters
        assert sig["q_len"].default == 1 and sig["window_left"].default is None
        assert sig["q_len"].kind is inspect.Parameter.KEYWORD_ONLY and sig["window_left"].kind is inspect.Parameter.KEYWORD_ONLY
    # None is today's rule, a window the new one
    assert fa.decode_num_splits(1, 8, 131072, 128) == lib.fa2_decode_num_splits(1, 8, 131072, 128) == 32
    assert fa.decode_num_splits(1, 8, 131072, 128, q_len=1, window_left=4095) == 16
    assert fa.decode_num_splits(1, 8, 131072, 128, window_left=2 ** 40) == 32
    # the workspace of a windowed call with n_splits = 0 is the window's split count's
    ws = fa.decode_workspace(1, 64, 8, 1, 131072, 128, 0, device="cpu", q_len=1, window_left=4095)
    assert ws.numel() == lib.fa2_decode_workspace_bytes(1, 64, 8, 1, 131072, 128, 16) > 0
    assert fa.decode_workspace(1, 64, 8, 1, 131072, 128, 0, device="cpu", window_left=127).numel() == 0
    assert fa.decode_workspace(1, 64, 8, 1, 131072, 128, 0, device="cpu").numel() == lib.fa2_decode_workspace_bytes(1, 64, 8, 1, 131072, 128, 32)
    assert fa.decode_workspace(1, 64, 8, 1, 131072, 128, 4, device="cpu", window_left=127).numel() == lib.fa2_decode_workspace_bytes(1, 64, 8, 1, 131072, 128, 4)
