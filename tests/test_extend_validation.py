"""CPU: the argument checks of extend attention (include/fa2_extend_mi355x.h), without a GPU.
(i) The four symbols are declared in the header, exported by libfa2_mi355x.so and bound through _capi.EXTEND_SIGNATURES; the two
calls take the arguments of fa2_forward_decode_window / _paged_window in their order.
(ii) The status codes in the documented order, with pointers that are never dereferenced: the siblings' codes without the row
limit, and FA2_ERR_INVALID_SHAPE for every product that would overflow.
(iii) fa2_extend_num_splits against the stated rule, and against the sibling's for M <= 32; fa2_extend_workspace_bytes against
its formula.
(iv) The wrappers' ValueErrors, and the decode wrappers' refusal of 36 rows, which stays."""
import ctypes
import os
import re

import pytest
import torch

import extend_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fa2_extend_num_splits", "fa2_extend_workspace_bytes", "fa2_forward_extend", "fa2_forward_extend_paged")
INT_MAX = 2 ** 31 - 1
BF16, F32, E4M3 = 0, 1, 2
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def _params(text, name):
    return [p.strip() for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text, main = _strip("fa2_extend_mi355x.h"), _strip("fa2_mi355x.h")
    so = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    bound = _capi.lib()
    assert sorted(_capi.EXTEND_SIGNATURES) == sorted(NEW)
    for name in NEW:
        assert hasattr(so, name), f"{name} not exported"
        assert name not in _capi.SIGNATURES and not re.search(r"\b" + name + r"\b", main), name      # a header and a table of their own
        res, args = _capi.EXTEND_SIGNATURES[name]
        params = _params(text, name)
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_float if "float" in p else ctypes.c_int
            assert a is want, (name, p)
        assert res is (ctypes.c_size_t if name == "fa2_extend_workspace_bytes" else ctypes.c_int)
        assert list(getattr(bound, name).argtypes) == list(args)
    for name, sibling in (("fa2_forward_extend", "fa2_forward_decode_window"), ("fa2_forward_extend_paged", "fa2_forward_decode_paged_window")):
        assert _params(text, name) == _params(main, sibling)
    assert _params(text, "fa2_extend_num_splits") == [f"int {n}" for n in ("B", "H_q", "H_kv", "q_len", "kv_capacity", "head_dim", "window_left")]
    assert _params(text, "fa2_extend_workspace_bytes") == [f"int {n}" for n in ("B", "H_q", "H_kv", "q_len", "kv_capacity", "head_dim", "n_splits",
                                                                                  "window_left")]


def test_header_describes_the_contract():
    text = open(os.path.join(ROOT, "include", "fa2_extend_mi355x.h")).read()
    for phrase in ("STATUS CODES", "NOT COVERED", "ROUTING", "tree masks", "a backward", "token-major", "fa2_merge_states", "no row limit"):
        assert phrase in text, phrase


def _contiguous(lib, ptrs=None, **kw):
    a = dict(B=1, Hq=64, Hkv=1, q=1, cap=4096, d=128, scale=0.125, dtype=BF16, kv=BF16, causal=1, ns=1, ws=None, wsb=0, wl=127,
             kd=None, vd=None)
    a.update(kw)
    p = list(ptrs or (ONE, ONE, ONE, None, None, a["kd"], a["vd"], ONE, ONE))
    return lib.fa2_forward_extend(*p, a["B"], a["Hq"], a["Hkv"], a["q"], a["cap"], a["d"], a["scale"], a["dtype"], a["kv"],
                                  a["causal"], a["ns"], a["ws"], a["wsb"], None, a["wl"])


def _paged(lib, ptrs=None, **kw):
    a = dict(B=1, Hq=64, Hkv=1, q=1, pages=100, P=64, mp=64, d=128, scale=0.125, dtype=BF16, kv=BF16, causal=1, ns=1, ws=None, wsb=0,
             wl=127, kd=None, vd=None)
    a.update(kw)
    if "cap" in a:
        a["mp"] = a.pop("cap") // a["P"]
    p = list(ptrs or (ONE, ONE, ONE, ONE, None, None, a["kd"], a["vd"], ONE, ONE))
    return lib.fa2_forward_extend_paged(*p, a["B"], a["Hq"], a["Hkv"], a["q"], a["pages"], a["P"], a["mp"], a["d"], a["scale"],
                                        a["dtype"], a["kv"], a["causal"], a["ns"], a["ws"], a["wsb"], None, a["wl"])


@pytest.mark.parametrize("call,required", ((_contiguous, (0, 1, 2, 7, 8)), (_paged, (0, 1, 2, 3, 8, 9))), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, required):
    """Every call here has M = 64 rows per K/V head (or more) unless it says otherwise: the extend path's own checks."""
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    n_ptrs = 9 if call is _contiguous else 10
    for missing in required:      # Q, K, V, (block_table,) O, L: NULL comes before everything else
        ptrs = [ONE] * n_ptrs
        ptrs[missing] = None
        assert call(lib, tuple(ptrs), B=0, d=96, dtype=7, wl=-5) == -1, missing
        assert call(lib, tuple(ptrs), d=96, dtype=7, wl=-5) == -1, missing
    # shapes, window_left < -1 and the rows of O among them, before head_dim, dtype, workspace and the refusal
    shapes = [dict(B=0), dict(Hq=0), dict(Hkv=3), dict(q=0), dict(scale=0.0), dict(ns=-1), dict(ns=257), dict(wl=-2), dict(wl=-INT_MAX - 1),
              dict(B=1 << 14, Hq=1 << 12, q=1 << 6), dict(B=1 << 18, q=1 << 8)]
    shapes += [dict(cap=0)] if call is _contiguous else [dict(pages=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15)]
    for bad in shapes:
        assert call(lib, **dict(dict(d=96, dtype=7, causal=0, kd=ONE), **bad)) == -2, bad
    if call is _contiguous:      # the slab limit follows the caches' element size, as in the siblings
        assert call(lib, cap=1 << 23, d=128) == -2 and call(lib, cap=(1 << 23) - 1, d=128, dtype=7) == -4
        assert call(lib, cap=1 << 24, d=128, kv=E4M3) == -2 and call(lib, cap=(1 << 24) - 1, d=128, kv=E4M3, dtype=7) == -4
    assert call(lib, d=96, dtype=7, causal=0) == -3                      # head_dim before dtype
    for kw in (dict(dtype=F32), dict(dtype=E4M3), dict(kv=F32), dict(kv=7), dict(kd=ONE), dict(vd=ONE)):      # a descale beside bf16 caches
        assert call(lib, **dict(kw, ns=4, causal=0)) == -4, kw           # dtype before the workspace and the refusal
    assert call(lib, kv=E4M3, kd=ONE, vd=ONE, ns=4) == -5                # descales belong to e4m3 caches
    # the grid B H_kv ceil(M / 64) n_splits, and a workspace size that does not fit, before the workspace
    assert call(lib, B=1 << 18, Hq=64, Hkv=64, q=64, ns=256, causal=0) == -2
    assert call(lib, B=1 << 18, Hq=64, Hkv=64, q=64, ns=64, causal=0) == -5
    need = lib.fa2_extend_workspace_bytes(1, 64, 1, 1, 4096, 128, 4, 127)
    assert need == (4 * 64 * 129 * 4 + 255) // 256 * 256
    assert call(lib, ns=4, causal=0) == -5                               # the workspace before the refusal
    assert call(lib, ns=4, ws=ONE, wsb=need - 1) == -5
    assert call(lib, ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    # n_splits = 0 resolves by the rule: 127 + 1 + 127 keys are one split; without a window one row block of a capacity of 4096 is 16
    assert call(lib, ns=0, causal=0) == -6
    for wl in (-1, 4095, 4096, INT_MAX):
        assert call(lib, ns=0, wl=wl) == -5, wl
    # the one refusal left: a window without causal.  There is no row limit: -6 is never about M
    assert call(lib, causal=0) == -6 and call(lib, causal=0, wl=0) == -6 and call(lib, causal=0, wl=INT_MAX) == -6
    assert call(lib, causal=0, wl=0, kv=E4M3, kd=ONE) == -6
    # M <= 32 is the sibling's call, its codes in its order
    assert call(lib, Hq=8, Hkv=2, causal=0) == -6 and call(lib, Hq=8, Hkv=2, ns=4) == -5 and call(lib, Hq=8, Hkv=2, d=96) == -3


SHAPES = ((1, 64, 8, 8, 8192, 128), (8, 64, 8, 8, 8192, 128), (8, 64, 8, 8, 32768, 128), (1, 64, 1, 1, 32768, 128), (4, 64, 1, 1, 8192, 64),
          (1, 32, 8, 512, 8192, 128), (1, 32, 8, 2048, 32768, 128), (1, 32, 8, 2048, 4096, 64), (2, 13, 1, 5, 2560, 64), (1, 4, 4, 70, 2560, 128),
          (10, 33, 1, 1, 2560, 64), (3, 8, 2, 40, 100000, 64), (1, 8, 2, 4, 4096, 128), (9, 32, 1, 1, 1024, 64), (1, 8, 8, 32, 131072, 128))


def test_num_splits_and_workspace_follow_the_rule():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    seen = set()
    for B, hq, hkv, q, cap, d in SHAPES:
        M = hq // hkv * q
        c = dict(lens=(0,) * B, hq=hq, hkv=hkv, nq=q, ncap=cap)
        for wl in (-1, 0, 1, 31, 127, 128, 200, 1000, 4095, cap - 2, cap - 1, cap, INT_MAX):
            got = lib.fa2_extend_num_splits(B, hq, hkv, q, cap, d, wl)
            assert got == er.resolved_splits(c, None if wl < 0 else wl, 0), (B, hq, hkv, q, cap, wl)
            if M <= 32:
                assert got == lib.fa2_decode_window_num_splits(B, hkv, q, cap, d, wl)
            else:
                keys = cap if wl < 0 or wl >= cap - 1 else min(cap, wl + q + 127)
                assert got == min(-(-256 // (B * hkv * -(-M // 64))), max(1, keys // 256), 256)
            seen.add((M <= 32, got > 1))
            for ns in (0, 1, 2, 7, 256):
                n = ns or got
                want = 0 if n == 1 else (n * B * hq * q * (d + 1) * 4 + 255) // 256 * 256
                assert lib.fa2_extend_workspace_bytes(B, hq, hkv, q, cap, d, ns, wl) == want, (B, hq, hkv, q, cap, wl, ns)
    assert len(seen) == 4
    assert lib.fa2_extend_num_splits(1, 32, 8, 2048, 32768, 128, -1) == 1          # a 2048-token chunk: one split, no workspace
    assert lib.fa2_extend_workspace_bytes(1, 32, 8, 2048, 32768, 128, 0, -1) == 0
    assert lib.fa2_extend_num_splits(8, 64, 8, 8, 32768, 128, -1) == 4             # verification: 64 workgroups, 4 splits
    assert lib.fa2_extend_num_splits(0, 64, 1, 1, 1024, 128, 127) == 1 and lib.fa2_extend_num_splits(1, 64, 1, 1, 0, 128, 127) == 1
    for bad in ((0, 64, 1, 1, 1024, 128, 2, -1), (1, 64, 0, 1, 1024, 128, 2, -1), (1, 64, 1, 1, 1024, 128, 257, -1), (1, 64, 1, 1, 1024, 128, -1, -1)):
        assert lib.fa2_extend_workspace_bytes(*bad) == 0, bad


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


@pytest.mark.parametrize("what,kw,match", [
    ("negative window", dict(window_left=-1), "window_left: -1, expected an int >= 0, or None"),
    ("float window", dict(window_left=127.0), "window_left: 127.0, expected an int >= 0"),
    ("not causal", dict(window_left=127, causal=False), "window_left: 127 with causal=False; the window is a causal one"),
    ("splits", dict(n_splits=257), "n_splits: 257, expected an int in 1..256"),
    ("bool splits", dict(n_splits=True), "n_splits: True, expected an int"),
    ("host lengths", dict(seqlens_k=[1, 2]), "seqlens_k must be an int32 device tensor"),
    ("cpu lengths", dict(seqlens_k=torch.zeros(2, dtype=torch.int32)), "seqlens_k is a CPU tensor"),
    ("descale beside bf16", dict(k_descale=torch.ones(2)), "k_descale: a descale belongs to torch.float8_e4m3fn caches"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_wrappers_refuse(what, kw, match):
    """The decode wrappers' checks, through the shared helpers, on 40 rows per K/V head (which those wrappers refuse)."""
    import cuda_flashattention_amd as fa
    with pytest.raises(ValueError, match=match):
        fa.flash_attention_2_extend(_t(2, 16, 5, 128), _t(2, 2, 256, 128), _t(2, 2, 256, 128), **kw)
    if "seqlens_k" not in kw:      # (the paged wrapper looks at the block table first, a CPU tensor here)
        with pytest.raises(ValueError, match=match):
            fa.flash_attention_2_extend_paged(_t(2, 16, 5, 128), _t(12, 2, 64, 128), _t(12, 2, 64, 128), torch.zeros(2, 5, dtype=torch.int32), **kw)


def test_wrappers_refuse_shapes_and_the_decode_wrappers_keep_their_row_limit():
    import cuda_flashattention_amd as fa
    for f in (fa.flash_attention_2_extend, fa.flash_attention_2_decode):
        with pytest.raises(ValueError, match="head_dim 96"):
            f(_t(2, 16, 5, 96), _t(2, 2, 256, 96), _t(2, 2, 256, 96))
        with pytest.raises(ValueError):
            f(_t(2, 16, 5, 128), _t(2, 3, 256, 128), _t(2, 3, 256, 128))          # 3 does not divide 16
        with pytest.raises(ValueError):
            f(_t(2, 16, 5, 128, dtype=torch.float32), _t(2, 2, 256, 128), _t(2, 2, 256, 128))
    with pytest.raises(ValueError, match="page_size 48 is not a multiple of 32"):
        fa.flash_attention_2_extend_paged(_t(2, 16, 5, 128), _t(12, 2, 48, 128), _t(12, 2, 48, 128), torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="block_table: dtype"):
        fa.flash_attention_2_extend_paged(_t(2, 16, 5, 128), _t(12, 2, 64, 128), _t(12, 2, 64, 128), torch.zeros(2, 5, dtype=torch.int64))
    # the decode wrappers still refuse 36 rows, in their words
    with pytest.raises(ValueError, match="36 rows, decode takes at most 32: that is a prefill chunk"):
        fa.flash_attention_2_decode(_t(1, 8, 9, 128), _t(1, 2, 256, 128), _t(1, 2, 256, 128))
    with pytest.raises(ValueError, match="36 rows, decode takes at most 32: that is a prefill chunk"):
        fa.flash_attention_2_decode_paged(_t(1, 8, 9, 128), _t(12, 2, 64, 128), _t(12, 2, 64, 128), torch.zeros(1, 5, dtype=torch.int32))
    # the extend wrappers take them as far as the device check (CPU tensors here)
    with pytest.raises(ValueError) as e:
        fa.flash_attention_2_extend(_t(1, 8, 9, 128), _t(1, 2, 256, 128), _t(1, 2, 256, 128))
    assert "rows" not in str(e.value)


def test_helpers():
    import cuda_flashattention_amd as fa
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    assert fa.extend_num_splits(8, 64, 8, 8, 32768, 128) == lib.fa2_extend_num_splits(8, 64, 8, 8, 32768, 128, -1) == 4
    assert fa.extend_num_splits(8, 64, 8, 8, 32768, 128, window_left=127) == 1
    assert fa.extend_num_splits(1, 8, 2, 4, 4096, 128) == fa.decode_num_splits(1, 2, 4096, 128)
    assert fa.extend_workspace(8, 64, 8, 8, 32768, 128, device="cpu").numel() == lib.fa2_extend_workspace_bytes(8, 64, 8, 8, 32768, 128, 4, -1) > 0
    assert fa.extend_workspace(8, 64, 8, 8, 32768, 128, device="cpu", window_left=127).numel() == 0
    assert fa.extend_workspace(1, 32, 8, 2048, 32768, 128, device="cpu").numel() == 0
    with pytest.raises(ValueError, match="window_left: -1"):
        fa.extend_num_splits(8, 64, 8, 8, 32768, 128, window_left=-1)
