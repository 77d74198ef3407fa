"""CPU: the argument checks of ragged extend attention (include/fa2_extend_ragged_mi355x.h), without a GPU.
(i) The seven symbols are declared in the header, exported by libfa2_mi355x.so and bound through _capi.EXTEND_RAGGED_SIGNATURES;
the two calls take the siblings' arguments with total_q for q_len, q_token_stride behind Q and plan, plan_bytes behind the caches
(the table).
(ii) The status codes in the documented order, with pointers that are never dereferenced.
(iii) The host formulas -- max_blocks, plan_bytes, num_splits, workspace_bytes -- against extend_ragged_ref's restatement.
(iv) The wrappers' ValueErrors: wrong dtype, wrong device, wrong shape, a bad stride."""
import ctypes
import os
import re

import pytest
import torch

import extend_ragged_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fa2_extend_ragged_max_blocks", "fa2_extend_ragged_plan_bytes", "fa2_extend_ragged_plan", "fa2_extend_ragged_num_splits",
       "fa2_extend_ragged_workspace_bytes", "fa2_forward_extend_ragged", "fa2_forward_extend_ragged_paged")
INT_MAX = 2 ** 31 - 1
BF16, F32, E4M3 = 0, 1, 2
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def _params(text, name):
    return [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", text).group(1).split(",")]


def test_symbols_exported_and_bound():
    from cuda_flashattention_amd import _capi
    text, sib, main = _strip("fa2_extend_ragged_mi355x.h"), _strip("fa2_extend_mi355x.h"), _strip("fa2_mi355x.h")
    so = ctypes.CDLL(os.path.join(ROOT, "cuda_flashattention_amd", "lib", "libfa2_mi355x.so"))
    bound = _capi.lib()
    assert sorted(_capi.EXTEND_RAGGED_SIGNATURES) == sorted(NEW)
    assert sorted(re.findall(r"\b(fa2_\w+)\s*\(", text)) == sorted(NEW)
    res_of = {"fa2_extend_ragged_max_blocks": ctypes.c_longlong, "fa2_extend_ragged_plan_bytes": ctypes.c_size_t,
              "fa2_extend_ragged_workspace_bytes": ctypes.c_size_t}
    for name in NEW:
        assert hasattr(so, name), f"{name} not exported"
        for table in (_capi.SIGNATURES, _capi.KVCACHE_SIGNATURES, _capi.ROPE_SIGNATURES, _capi.EXTEND_SIGNATURES):
            assert name not in table
        assert not re.search(r"\b" + name + r"\b", main) and not re.search(r"\b" + name + r"\b", sib), name
        res, args = _capi.EXTEND_RAGGED_SIGNATURES[name]
        params = _params(text, name)
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = (ctypes.c_void_p if "*" in p else ctypes.c_size_t if "size_t" in p else ctypes.c_float if "float" in p
                    else ctypes.c_longlong if "long long" in p else ctypes.c_int)
            assert a is want, (name, p)
        assert res is res_of.get(name, ctypes.c_int)
        assert list(getattr(bound, name).argtypes) == list(args)

    def ragged_form(params, after):      # the sibling's list as the ragged call takes it
        out = [p.replace("int q_len", "int total_q") for p in params]
        out.insert(1, "long long q_token_stride")
        at = out.index(after) + 1
        return out[:at] + ["const void* plan", "size_t plan_bytes"] + out[at:]

    assert _params(text, "fa2_forward_extend_ragged") == ragged_form(_params(sib, "fa2_forward_extend"), "const void* V_cache")
    assert _params(text, "fa2_forward_extend_ragged_paged") == ragged_form(_params(sib, "fa2_forward_extend_paged"), "const int* block_table")
    dims = [f"int {n}" for n in ("B", "H_q", "H_kv", "total_q")]
    assert _params(text, "fa2_extend_ragged_max_blocks") == dims and _params(text, "fa2_extend_ragged_plan_bytes") == dims
    assert _params(text, "fa2_extend_ragged_plan") == ["const int* cu_seqlens_q"] + dims + ["void* plan", "size_t plan_bytes", "void* stream"]
    assert _params(text, "fa2_extend_ragged_num_splits") == dims + ["int kv_capacity", "int head_dim", "int window_left"]
    assert _params(text, "fa2_extend_ragged_workspace_bytes") == dims + ["int kv_capacity", "int head_dim", "int n_splits", "int window_left"]
    assert sorted(_capi.SIGNATURES) == sorted(set(re.findall(r"\b(fa2_\w+|flash_attention\w*)\s*\(", main)))      # SIGNATURES stays the main header's


def test_header_describes_the_contract():
    text = open(os.path.join(ROOT, "include", "fa2_extend_ragged_mi355x.h")).read()
    for phrase in ("STATUS CODES", "NOT COVERED", "THE PLAN IS THE SAFETY CONTRACT", "CALLER'S ERROR", "running maximum", "ragged KV append",
                   "tree masks", "backward", "token-major pools", "longest-first", "q_token_stride", "fa2_merge_states", "FA2_ERR_WORKSPACE"):
        assert phrase in text, phrase
    sib = open(os.path.join(ROOT, "include", "fa2_extend_mi355x.h")).read()
    assert "fa2_extend_ragged_mi355x.h" in sib      # the "not covered" line now points here


T0, HQ0 = 575, 32
PB0 = rr.plan_bytes(64, 32, 8, 575)


def _contiguous(lib, ptrs=None, **kw):
    a = dict(B=64, Hq=HQ0, Hkv=8, T=T0, cap=4096, d=128, scale=0.125, dtype=BF16, kv=BF16, causal=1, ns=1, ws=None, wsb=0, wl=127,
             kd=None, vd=None, qs=HQ0 * 128, pb=PB0)
    a.update(kw)
    Q, K, V, plan, O, L = ptrs or (ONE,) * 6
    return lib.fa2_forward_extend_ragged(Q, a["qs"], K, V, plan, a["pb"], None, None, a["kd"], a["vd"], O, L, a["B"], a["Hq"], a["Hkv"], a["T"],
                                         a["cap"], a["d"], a["scale"], a["dtype"], a["kv"], a["causal"], a["ns"], a["ws"], a["wsb"], None, a["wl"])


def _paged(lib, ptrs=None, **kw):
    a = dict(B=64, Hq=HQ0, Hkv=8, T=T0, pages=100, P=64, mp=64, d=128, scale=0.125, dtype=BF16, kv=BF16, causal=1, ns=1, ws=None, wsb=0,
             wl=127, kd=None, vd=None, qs=HQ0 * 128, pb=PB0)
    a.update(kw)
    if "cap" in a:
        a["mp"] = a.pop("cap") // a["P"]
    Q, K, V, table, plan, O, L = ptrs or (ONE,) * 7
    return lib.fa2_forward_extend_ragged_paged(Q, a["qs"], K, V, table, plan, a["pb"], None, None, a["kd"], a["vd"], O, L, a["B"], a["Hq"],
                                               a["Hkv"], a["T"], a["pages"], a["P"], a["mp"], a["d"], a["scale"], a["dtype"], a["kv"],
                                               a["causal"], a["ns"], a["ws"], a["wsb"], None, a["wl"])


@pytest.mark.parametrize("call,n_ptrs", ((_contiguous, 6), (_paged, 7)), ids=("contiguous", "paged"))
def test_status_codes_in_order(call, n_ptrs):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    for missing in range(n_ptrs):      # Q, K, V, (block_table,) plan, O, L: NULL comes before everything else
        ptrs = [ONE] * n_ptrs
        ptrs[missing] = None
        assert call(lib, tuple(ptrs), B=0, d=96, dtype=7, wl=-5, pb=0) == -1, missing
    # shapes -- the stride, window_left < -1 and the rows of O among them -- before head_dim, dtype, the plan, the workspace, the refusal
    shapes = [dict(B=0), dict(Hq=0), dict(Hkv=3), dict(T=0), dict(T=-1), dict(scale=0.0), dict(ns=-1), dict(ns=257), dict(wl=-2),
              dict(qs=HQ0 * 96 - 8), dict(qs=HQ0 * 128 + 4), dict(qs=0), dict(qs=-HQ0 * 128), dict(T=(INT_MAX - 64) // HQ0 + 1),      # (d is 96 here)
              dict(B=1 << 22, Hq=8)]
    shapes += [dict(cap=0)] if call is _contiguous else [dict(pages=0), dict(P=48), dict(mp=0), dict(P=1 << 16, mp=1 << 15)]
    for bad in shapes:
        assert call(lib, **dict(dict(d=96, dtype=7, causal=0, kd=ONE, pb=0), **bad)) == -2, bad
    if call is _contiguous:      # the slab limit follows the caches' element size, as in the siblings
        assert call(lib, cap=1 << 23) == -2 and call(lib, cap=(1 << 23) - 1, dtype=7) == -4
        assert call(lib, cap=1 << 24, kv=E4M3) == -2 and call(lib, cap=(1 << 24) - 1, kv=E4M3, dtype=7) == -4
    assert call(lib, d=96, qs=HQ0 * 96, dtype=7, causal=0, pb=0) == -3                      # head_dim before dtype
    for kw in (dict(dtype=F32), dict(dtype=E4M3), dict(kv=F32), dict(kv=7), dict(kd=ONE), dict(vd=ONE)):      # a descale beside bf16 caches
        assert call(lib, **dict(kw, ns=4, causal=0, pb=0)) == -4, kw      # dtype before the plan, the workspace and the refusal
    # the grid max_blocks x H_kv x n_splits, before the plan and the workspace
    big = dict(T=(INT_MAX - 64) // 64, Hq=64, Hkv=64, qs=64 * 128, B=1 << 16)
    assert call(lib, **big, ns=256, causal=0, pb=0) == -2
    assert call(lib, **big, ns=1, causal=0, pb=0) == -5
    # the plan: too small, misaligned -- before the workspace and the refusal
    assert call(lib, pb=PB0 - 1, ns=4, causal=0) == -5 and call(lib, pb=0, causal=0) == -5
    ptrs = [ONE] * n_ptrs
    ptrs[n_ptrs - 3] = ctypes.c_void_p(24)
    assert call(lib, tuple(ptrs), causal=0) == -5
    need = lib.fa2_extend_ragged_workspace_bytes(64, HQ0, 8, T0, 4096, 128, 4, 127)
    assert need == (4 * T0 * HQ0 * 129 * 4 + 255) // 256 * 256
    assert call(lib, ns=4, causal=0) == -5                               # the workspace before the refusal
    assert call(lib, ns=4, ws=ONE, wsb=need - 1) == -5
    assert call(lib, ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    # the one refusal: a window without causal
    assert call(lib, causal=0) == -6 and call(lib, causal=0, wl=0) == -6 and call(lib, causal=0, wl=INT_MAX) == -6
    assert call(lib, causal=0, wl=0, kv=E4M3, kd=ONE) == -6
    assert call(lib, ns=0, causal=0) == -6                               # 127 + 575 + 127 keys over 64 x 8 workgroups: one split


def test_plan_status_codes():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    plan = lambda cu=ONE, B=64, Hq=32, Hkv=8, T=575, p=ONE, pb=PB0: lib.fa2_extend_ragged_plan(cu, B, Hq, Hkv, T, p, pb, None)
    assert plan(cu=None, B=0) == -1 and plan(p=None, pb=0) == -1
    for bad in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(Hkv=5), dict(T=0), dict(T=(INT_MAX - 64) // 32 + 1)):
        assert plan(**bad, pb=0) == -2, bad
    assert plan(pb=PB0 - 1) == -5 and plan(p=ctypes.c_void_p(24)) == -5


SHAPES = ((64, 32, 8, 575), (64, 32, 8, 288), (8, 32, 8, 64), (1, 32, 8, 2048), (256, 32, 8, 2303), (10, 8, 2, 95), (5, 33, 1, 5), (5, 4, 4, 233),
          (10, 16, 2, 10), (2, 8, 1, 29), (300, 8, 8, 7), (1, 64, 1, 1), (3, 128, 8, 100000))


def test_host_formulas_follow_the_rule():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    seen = set()
    for B, hq, hkv, T in SHAPES:
        assert lib.fa2_extend_ragged_max_blocks(B, hq, hkv, T) == rr.max_blocks(B, hq, hkv, T) == (hq // hkv) * T // 64 + min(B, T)
        assert lib.fa2_extend_ragged_plan_bytes(B, hq, hkv, T) == rr.plan_bytes(B, hq, hkv, T)
        for cap, d in ((8192, 128), (32768, 128), (2560, 64), (300, 64)):
            for wl in (-1, 0, 1, 31, 127, 200, 1000, cap - 2, cap - 1, cap, INT_MAX):
                got = lib.fa2_extend_ragged_num_splits(B, hq, hkv, T, cap, d, wl)
                groups = hkv * max(min(B, T), -(-(hq // hkv * T) // 64))
                span = cap if wl < 0 or wl >= cap - 1 else min(cap, wl + T + 127)
                assert got == rr.num_splits(B, hq, hkv, T, cap, wl) == min(-(-256 // groups), max(1, span // 256), 256), (B, hq, hkv, T, cap, wl)
                seen.add(got > 1)
                for ns in (0, 1, 2, 7, 256):
                    want = rr.workspace_bytes(hq, T, d, ns or got)
                    assert lib.fa2_extend_ragged_workspace_bytes(B, hq, hkv, T, cap, d, ns, wl) == want, (B, hq, hkv, T, cap, wl, ns)
    assert seen == {False, True}
    assert lib.fa2_extend_ragged_num_splits(8, 32, 8, 64, 32768, 128, -1) == 4      # 8 x 8 workgroups of verification: 4 splits
    assert lib.fa2_extend_ragged_num_splits(64, 32, 8, 575, 32768, 128, -1) == 1    # a mixed step fills the GPU: one split
    for bad in ((0, 32, 8, 5), (1, 0, 8, 5), (1, 32, 0, 5), (1, 32, 5, 5), (1, 32, 8, 0), (1, 32, 8, (INT_MAX - 64) // 32 + 1)):
        assert lib.fa2_extend_ragged_max_blocks(*bad) == 0 and lib.fa2_extend_ragged_plan_bytes(*bad) == 0, bad
        assert lib.fa2_extend_ragged_num_splits(*bad, 4096, 128, -1) == 1 and lib.fa2_extend_ragged_workspace_bytes(*bad, 4096, 128, 2, -1) == 0
    assert lib.fa2_extend_ragged_num_splits(1, 32, 8, 5, 0, 128, -1) == 1
    for ns in (-1, 257):
        assert lib.fa2_extend_ragged_workspace_bytes(1, 32, 8, 5, 4096, 128, ns, -1) == 0


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


CU = torch.tensor([0, 5, 29], dtype=torch.int32)


@pytest.mark.parametrize("what,args,kw,match", [
    ("Q rank", (_t(2, 8, 29, 128),), {}, r"Q: expected a 3-d tensor \[T, H_q, d\]"),
    ("Q dtype", (_t(29, 8, 128, dtype=torch.float32),), {}, "Q: dtype torch.float32, expected torch.bfloat16"),
    ("head_dim", (_t(29, 8, 96), _t(2, 1, 256, 96)), {}, "head_dim 96"),
    ("heads", (_t(29, 8, 128), _t(2, 3, 256, 128)), {}, "does not match Q"),
    ("cache rank", (_t(29, 8, 128), _t(2, 256, 128)), {}, "K_cache: expected a 4-d tensor"),
    ("cache dtype", (_t(29, 8, 128), _t(2, 1, 256, 128, dtype=torch.float16)), {}, "K_cache: dtype torch.float16"),
    ("head-major Q", (_t(8, 29, 128).transpose(0, 1),), {}, "the last two dimensions must be contiguous"),
    ("odd stride", (_t(29, 8 * 128 + 4)[:, :8 * 128].view(29, 8, 128),), {}, "token stride 1028"),
    ("offset", (_t(29 * 8 * 128 + 4)[4:].view(29, 8, 128),), {}, "storage offset 4"),
    ("splits", (), dict(n_splits=257), "n_splits: 257, expected an int in 1..256"),
    ("negative window", (), dict(window_left=-1), "window_left: -1, expected an int >= 0, or None"),
    ("not causal", (), dict(window_left=127, causal=False), "window_left: 127 with causal=False"),
    ("host cu", (), dict(cu=[0, 5, 29]), "cu_seqlens_q must be an int32 device tensor"),
    ("cu dtype", (), dict(cu=CU.long()), "cu_seqlens_q: dtype torch.int64"),
    ("cu shape", (), dict(cu=CU[:1]), r"cu_seqlens_q: shape \(1,\)"),
    ("cpu cu", (), dict(), "cu_seqlens_q is a CPU tensor"),
    ("descale beside bf16", (), dict(k_descale=torch.ones(1), cu="plan"), "k_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("cpu lengths", (), dict(seqlens_k=torch.zeros(2, dtype=torch.int32), cu="plan"), "seqlens_k is a CPU tensor"),
    ("plan for another T", (_t(30, 8, 128),), dict(cu="plan"), "plan: built for H_q / H_kv = 8 and total_q = 29"),
    ("plan's B", (_t(29, 8, 128), _t(3, 1, 256, 128)), dict(cu="plan"), "K_cache: 3 sequences"),
    ("cpu Q", (), dict(cu="plan"), "Q must be a device tensor"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 24 else "")
def test_wrappers_refuse(what, args, kw, match):
    """A plan object stands in for cu_seqlens_q where the check under test comes behind cu_seqlens_q's own (CPU tensors here)."""
    import cuda_flashattention_amd as fa
    kw = dict(kw)
    cu = kw.pop("cu", CU)
    if isinstance(cu, str):
        cu = fa.ExtendRaggedPlan(torch.zeros(64, dtype=torch.int32), 2, 8, 1, 29)
    Q = args[0] if args else _t(29, 8, 128)
    K = args[1] if len(args) > 1 else _t(2, 1, 256, Q.shape[-1])
    with pytest.raises(ValueError, match=match):
        fa.flash_attention_2_extend_ragged(Q, K, torch.zeros_like(K), cu, **kw)
    if what in ("Q rank", "Q dtype", "head-major Q", "odd stride", "offset", "splits", "negative window", "not causal", "host cu", "cpu cu"):
        table = torch.zeros(2, 4, dtype=torch.int32)
        with pytest.raises(ValueError, match=match):
            fa.flash_attention_2_extend_ragged_paged(Q, _t(9, 1, 64, 128), _t(9, 1, 64, 128), table, cu, **kw)


def test_paged_wrapper_and_plan_helper_refuse():
    import cuda_flashattention_amd as fa
    plan = fa.ExtendRaggedPlan(torch.zeros(64, dtype=torch.int32), 2, 8, 1, 29)
    Q = _t(29, 8, 128)
    with pytest.raises(ValueError, match="page_size 48 is not a multiple of 32"):
        fa.flash_attention_2_extend_ragged_paged(Q, _t(9, 1, 48, 128), _t(9, 1, 48, 128), torch.zeros(2, 4, dtype=torch.int32), plan)
    with pytest.raises(ValueError, match="block_table: dtype"):
        fa.flash_attention_2_extend_ragged_paged(Q, _t(9, 1, 64, 128), _t(9, 1, 64, 128), torch.zeros(2, 4, dtype=torch.int64), plan)
    with pytest.raises(ValueError, match=r"block_table: shape \(3, 4\)"):
        fa.flash_attention_2_extend_ragged_paged(Q, _t(9, 1, 64, 128), _t(9, 1, 64, 128), torch.zeros(3, 4, dtype=torch.int32), plan)
    with pytest.raises(ValueError, match="block_table must be"):
        fa.flash_attention_2_extend_ragged_paged(Q, _t(9, 1, 64, 128), _t(9, 1, 64, 128), None, plan)
    for bad, match in (((8, 3, 29), "H_kv: 3 does not divide"), ((8, 1, 0), "total_q: 0"), ((0, 1, 29), "H_q: 0"), ((8, 1, 2.0), "total_q: 2.0")):
        with pytest.raises(ValueError, match=match):
            fa.extend_ragged_plan(CU, *bad)
    with pytest.raises(ValueError, match="cu_seqlens_q is a CPU tensor"):
        fa.extend_ragged_plan(CU, 8, 1, 29)
    with pytest.raises(ValueError, match="cu_seqlens_q: dtype"):
        fa.extend_ragged_plan(CU.float(), 8, 1, 29)


def test_helpers():
    import cuda_flashattention_amd as fa
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    assert fa.extend_ragged_num_splits(8, 32, 8, 64, 32768, 128) == lib.fa2_extend_ragged_num_splits(8, 32, 8, 64, 32768, 128, -1) == 4
    assert fa.extend_ragged_num_splits(8, 32, 8, 64, 32768, 128, window_left=127) == 1
    assert fa.extend_ragged_workspace(8, 32, 8, 64, 32768, 128, device="cpu").numel() == lib.fa2_extend_ragged_workspace_bytes(8, 32, 8, 64, 32768, 128, 4, -1) > 0
    assert fa.extend_ragged_workspace(8, 32, 8, 64, 32768, 128, device="cpu", window_left=127).numel() == 0
    assert fa.extend_ragged_workspace(64, 32, 8, 575, 32768, 128, device="cpu").numel() == 0
    with pytest.raises(ValueError, match="window_left: -1"):
        fa.extend_ragged_num_splits(8, 32, 8, 64, 32768, 128, window_left=-1)
