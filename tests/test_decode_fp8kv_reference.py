"""CPU: what tests/test_gpu_decode_fp8kv.py rests on (tests/decode_fp8kv_ref.py) and everything of the fp8-cache decode calls that
needs no GPU.

(i) decode_ref's emulation of the kernels' data flow on the quantised-then-dequantised caches against the float64 reference on
the same values, inside decode_ref's gates: every fourth case plus every regime case, at 1 and 7 splits.
(ii) The quantiser: per-head descales, saturation, exact round trips.
(iii) The ValueErrors flash_attention_2_decode and flash_attention_2_decode_paged add for fp8 caches and descales, on CPU tensors.
(iv) The status codes of fa2_forward_decode_fp8kv and fa2_forward_decode_paged_fp8kv, in the bf16 siblings' order, with pointers
that are never dereferenced; the workspace and split functions answer alike for both element sizes."""
import ctypes

import pytest
import torch

import decode_fp8kv_ref as fr
import decode_ref as dr

EMULATED = sorted(set(range(0, len(dr.CASES), 4)) | {i for i, c in enumerate(dr.CASES) if c["regime"]})


def _lib():
    from cuda_flashattention_amd import _capi
    return _capi.lib()


# ------------------------------------------------------------------------------------------------ (i)
@pytest.mark.parametrize("i", EMULATED, ids=[dr.case_id(dr.CASES[i]) for i in EMULATED])
def test_emulation_on_dequantised_caches_is_within_the_gates(i):
    ref = fr.reference(i)
    for n_splits in (1, 7):
        e = dr.errors(*fr.emulate(i, n_splits), ref)
        print(dr.case_id(dr.CASES[i]), f"splits {n_splits}: O {e[0]:.3e} dL {e[1]:.3e} dL(|L| > 25) {e[2]:.3e}")
        assert dr.within_gates(e), (dr.case_id(dr.CASES[i]), n_splits, e)


def test_the_emulated_selection():
    assert len(EMULATED) == 17 and sum(bool(dr.CASES[i]["regime"]) for i in EMULATED) == 8


# ------------------------------------------------------------------------------------------------ (ii)
def test_quantise_descales_per_head_and_saturates():
    g = torch.Generator().manual_seed(5)
    X = (torch.rand(2, 3, 40, 64, generator=g) - 0.5).bfloat16()
    X[:, 1] *= 37.0
    X[:, 2] *= 1e-3
    X8, ds = fr.quantise(X)
    assert X8.dtype == torch.float8_e4m3fn and ds.dtype == torch.float32 and ds.shape == (3,)
    torch.testing.assert_close(ds, X.float().abs().amax(dim=(0, 2, 3)) / 448.0, rtol=0, atol=0)
    assert len(set(ds.tolist())) == 3
    codes = X8.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any()                               # no NaN code: the clamp holds the cast below 448
    assert all(float(X8[:, h].float().abs().max()) == 448.0 for h in range(3))      # each head's largest magnitude is stored as 448
    # the quantisation error of a value is at most half an e4m3 step of its magnitude (2^-4 relative; 2^-10 absolute below 2^-6)
    err = (fr.dequantise(X8, ds) - X.float()).abs() / ds[None, :, None, None]
    stored = (X.float() / ds[None, :, None, None]).abs()
    assert (err <= torch.maximum(stored * 2.0 ** -4, torch.tensor(2.0 ** -10))).all()
    # every e4m3 value is a bf16 value: the cast to bf16 and back is the identity on all 254 numbers
    every = torch.arange(256, dtype=torch.int16).to(torch.uint8).view(torch.float8_e4m3fn)
    number = ~torch.isnan(every.float())
    assert int(number.sum()) == 254
    assert torch.equal(every.to(torch.bfloat16).to(torch.float8_e4m3fn).view(torch.uint8)[number], every.view(torch.uint8)[number])
    assert torch.equal(every.to(torch.bfloat16).float()[number], every.float()[number])


def test_pools_mark_what_no_key_was_copied_to():
    i, P = 2, 96
    Kp, Vp, table, lens, cap, unused = fr.paged_inputs(i, P)
    assert Kp.dtype == Vp.dtype == torch.float8_e4m3fn and cap == table.shape[1] * P
    assert unused.any() and not unused.all()
    assert set((Kp.view(torch.uint8)[unused] & 0x7F).unique().tolist()) == {0x7F}      # NaN where nothing was copied
    assert not torch.isnan(Kp.float()[~unused]).any()
    _, K8, _, _, _, _, _, _ = fr.inputs(i)
    K = fr.gather(Kp, table, lens, P)
    for b, n in enumerate(lens):
        assert torch.equal(K[b, :, :n].view(torch.uint8), K8[b, :, :n].view(torch.uint8))


# ------------------------------------------------------------------------------------------------ (iii)
def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


F8, F32 = torch.float8_e4m3fn, torch.float32
REFUSALS = [
    ("K fp8, V bf16", dict(K=F8), {}, "V_{}: dtype torch.bfloat16 beside K_{} torch.float8_e4m3fn: K and V are both"),
    ("K bf16, V fp8", dict(V=F8), {}, "V_{}: dtype torch.float8_e4m3fn beside K_{} torch.bfloat16: K and V are both"),
    ("e5m2", dict(K=torch.float8_e5m2, V=torch.float8_e5m2), {}, r"K_{}: dtype torch.float8_e5m2; an fp8 cache is OCP e4m3 \(torch.float8_e4m3fn\)"),
    ("fnuz", dict(K=torch.float8_e4m3fnuz, V=torch.float8_e4m3fnuz), {}, r"K_{}: dtype torch.float8_e4m3fnuz; an fp8 cache is OCP e4m3"),
    ("V e5m2", dict(K=F8, V=torch.float8_e5m2), {}, "V_{}: dtype torch.float8_e5m2; an fp8 cache is OCP e4m3"),
    ("descale, bf16 caches", {}, dict(k_descale=_t(2, dtype=F32)), "k_descale: a descale belongs to torch.float8_e4m3fn caches; K_{} is torch.bfloat16"),
    ("v_descale, bf16 caches", {}, dict(v_descale=_t(2, dtype=F32)), "v_descale: a descale belongs to torch.float8_e4m3fn caches"),
    ("descale no tensor", dict(K=F8, V=F8), dict(k_descale=[1.0, 1.0]), "k_descale must be a torch tensor"),
    ("descale a float", dict(K=F8, V=F8), dict(v_descale=0.5), "v_descale must be a torch tensor.*on the device"),
    ("descale dtype", dict(K=F8, V=F8), dict(k_descale=_t(2)), "k_descale: dtype torch.bfloat16, expected torch.float32"),
    ("descale count", dict(K=F8, V=F8), dict(v_descale=_t(8, dtype=F32)), r"v_descale: shape \(8,\), expected \(2,\): one descale per K/V head"),
    ("descale rank", dict(K=F8, V=F8), dict(k_descale=_t(1, 2, dtype=F32)), r"k_descale: shape \(1, 2\), expected \(2,\)"),
    ("descale strided", dict(K=F8, V=F8), dict(k_descale=_t(4, dtype=F32)[::2]), "k_descale must be contiguous"),
    ("descale on the host", dict(K=F8, V=F8), dict(v_descale=_t(2, dtype=F32)), "v_descale must be a device tensor"),
    ("fp8 Q", dict(Q=F8, K=F8, V=F8), {}, "Q: dtype torch.float8_e4m3fn, expected torch.bfloat16"),
]


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("what,dtypes,kw,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_wrapper_refuses(what, dtypes, kw, match, paged):
    import cuda_flashattention_amd as fa
    kv = (12, 2, 64, 128) if paged else (2, 2, 300, 128)
    Q, K, V = (_t(*s, dtype=dtypes.get(n, torch.bfloat16)) for n, s in (("Q", (2, 8, 1, 128)), ("K", kv), ("V", kv)))
    with pytest.raises(ValueError, match=match.format(*(["pages"] * 2 if paged else ["cache"] * 2))):
        if paged:
            fa.flash_attention_2_decode_paged(Q, K, V, torch.zeros(2, 5, dtype=torch.int32), **kw)
        else:
            fa.flash_attention_2_decode(Q, K, V, **kw)


def test_fp8_caches_get_past_the_dtype_checks():
    """Valid fp8 caches and descales on the host fail where the bf16 call's do: on the first tensor that must live on the device."""
    import cuda_flashattention_amd as fa
    Q, K8 = _t(2, 8, 1, 128), _t(2, 2, 300, 128, dtype=F8)
    with pytest.raises(ValueError, match="Q must be a device tensor"):
        fa.flash_attention_2_decode(Q, K8, K8)
    with pytest.raises(ValueError, match="k_descale must be a device tensor"):
        fa.flash_attention_2_decode(Q, K8, K8, k_descale=_t(2, dtype=F32))
    with pytest.raises(ValueError, match="block_table is a CPU tensor"):
        fa.flash_attention_2_decode_paged(Q, _t(12, 2, 64, 128, dtype=F8), _t(12, 2, 64, 128, dtype=F8), torch.zeros(2, 5, dtype=torch.int32))


def test_wrappers_document_the_descales():
    import cuda_flashattention_amd as fa
    for f in (fa.flash_attention_2_decode, fa.flash_attention_2_decode_paged):
        doc = " ".join(f.__doc__.split())
        assert "float8_e4m3fn" in doc and "x / descale" in doc and "on the device" in doc and "no append kernel" in doc
    assert "does not saturate" in fa.flash_attention_2_decode.__doc__


# ------------------------------------------------------------------------------------------------ (iv)
ONE = ctypes.c_void_p(16)      # never dereferenced: validation fails first


def test_status_codes_in_order():
    lib = _lib()
    ok = dict(B=1, Hq=8, Hkv=2, q=1, cap=4096, d=128, scale=0.125, dtype=0, kv=2, causal=1, ns=1, ws=None, wsb=0)

    def call(ptrs=(ONE,) * 9, **kw):
        a = dict(ok, **kw)
        return lib.fa2_forward_decode_fp8kv(*ptrs, a["B"], a["Hq"], a["Hkv"], a["q"], a["cap"], a["d"], a["scale"], a["dtype"], a["kv"],
                                            a["causal"], a["ns"], a["ws"], a["wsb"], None)

    for missing in (0, 1, 2, 7, 8):          # Q, K_cache, V_cache, O, L
        ptrs = [ONE] * 9
        ptrs[missing] = None
        assert call(tuple(ptrs), d=96, dtype=7, kv=7, B=0) == -1      # a NULL tensor comes before everything else
    # seqlens_k, sink and the two descales may be NULL: the call gets past the pointers and fails on what follows
    assert call((ONE, ONE, ONE, None, None, None, None, ONE, ONE), B=0) == -2
    for bad in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(q=0), dict(cap=0), dict(scale=0.0), dict(scale=-1.0), dict(Hq=8, Hkv=3),
                dict(ns=-1), dict(ns=257), dict(cap=1 << 24, d=128), dict(cap=1 << 25, d=64)):
        assert call(**dict(bad, dtype=7, kv=7)) == -2, bad            # shapes before head_dim and dtype
    assert call(cap=(1 << 24) - 1, dtype=7) == -4                     # one byte per element: the largest slab below 2 GiB
    assert call(cap=1 << 23, dtype=7) == -4                           # (the bf16 call's limit is not this one's)
    assert call(d=96, dtype=7, kv=7) == -3                            # head_dim before either dtype
    assert call(d=256) == -3
    for dtype in (1, 2, 7):
        assert call(dtype=dtype, ns=4, q=64) == -4                    # Q's dtype before the workspace and the row limit
    for kv in (0, 1, 7):
        assert call(kv=kv, ns=4, q=64) == -4                          # ... and the caches', at the same position
    need = lib.fa2_decode_workspace_bytes(1, 8, 2, 1, 4096, 128, 4)
    assert call(ns=4, q=64) == -5                                     # the workspace before the row limit
    assert call(ns=4, ws=ONE, wsb=need - 1) == -5
    assert call(ns=0, ws=None) == -5                                  # 0 resolves to 16 splits here, as for bf16
    assert call(ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5         # 16-byte alignment
    assert call(ns=1, q=9) == -6                                      # G q_len = 4 x 9 = 36 rows
    assert call((ONE, ONE, ONE, None, None, None, None, ONE, ONE), ns=1, q=9) == -6      # NULL descales pass every check before it
    assert call(ns=4, q=9, ws=ONE, wsb=lib.fa2_decode_workspace_bytes(1, 8, 2, 9, 4096, 128, 4)) == -6
    assert call(Hq=64, Hkv=1) == -6


def test_paged_status_codes_in_order():
    lib = _lib()
    ok = dict(B=1, Hq=8, Hkv=2, q=1, pages=100, P=64, mp=64, d=128, scale=0.125, dtype=0, kv=2, causal=1, ns=1, ws=None, wsb=0)

    def call(ptrs=(ONE,) * 10, **kw):
        a = dict(ok, **kw)
        return lib.fa2_forward_decode_paged_fp8kv(*ptrs, a["B"], a["Hq"], a["Hkv"], a["q"], a["pages"], a["P"], a["mp"], a["d"], a["scale"],
                                                  a["dtype"], a["kv"], a["causal"], a["ns"], a["ws"], a["wsb"], None)

    for missing in (0, 1, 2, 3, 8, 9):       # Q, K_pages, V_pages, block_table, O, L
        ptrs = [ONE] * 10
        ptrs[missing] = None
        assert call(tuple(ptrs), d=96, dtype=7, kv=7, B=0) == -1
    assert call((ONE, ONE, ONE, ONE, None, None, None, None, ONE, ONE), B=0) == -2
    for bad in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(q=0), dict(pages=0), dict(pages=-1), dict(P=0), dict(mp=0), dict(scale=0.0),
                dict(scale=-1.0), dict(Hq=8, Hkv=3), dict(P=48), dict(P=16), dict(P=33), dict(P=-32),
                dict(P=1 << 16, mp=1 << 15), dict(P=1 << 20, mp=1 << 20), dict(ns=-1), dict(ns=257),
                dict(B=1 << 24, Hq=1, Hkv=1, ns=256)):
        assert call(**dict(bad, d=96, dtype=7, kv=7)) == -2, bad      # shapes before head_dim and dtype
    assert call(P=1 << 15, mp=1 << 15, dtype=7) == -4                 # 2^30 keys pass the shape checks
    assert call(d=96, dtype=7, kv=7) == -3                            # head_dim before either dtype
    assert call(d=256) == -3
    for dtype in (1, 2, 7):
        assert call(dtype=dtype, ns=4, q=64) == -4
    for kv in (0, 1, 7):
        assert call(kv=kv, ns=4, q=64) == -4
    need = lib.fa2_decode_workspace_bytes(1, 8, 2, 1, 64 * 64, 128, 4)
    assert call(ns=4, q=64) == -5                                     # the workspace before the row limit
    assert call(ns=4, ws=ONE, wsb=need - 1) == -5
    assert call(ns=0, ws=None) == -5
    assert call(ns=4, ws=ctypes.c_void_p(24), wsb=need) == -5
    assert call(ns=1, q=9) == -6
    assert call((ONE, ONE, ONE, ONE, None, None, None, None, ONE, ONE), ns=1, q=9) == -6      # NULL descales accepted
    assert call(Hq=64, Hkv=1) == -6


def test_the_bf16_entry_points_still_refuse_fp8():
    lib = _lib()
    args = (1, 8, 2, 1, 4096, 128, ctypes.c_float(0.125), 2, 1, 1, None, 0, None)
    assert lib.fa2_forward_decode(*(ONE,) * 7, *args) == -4


def test_workspace_and_splits_do_not_depend_on_the_element_size():
    """One pair of functions serves both calls: the rule reads the capacity in keys.  The fp8 entry points resolve n_splits = 0 and
    size the workspace with them -- a workspace one byte short of fa2_decode_workspace_bytes is refused, that size gets past."""
    lib = _lib()
    for B, Hq, Hkv, q, cap, d in ((1, 8, 2, 1, 4096, 128), (1, 64, 8, 1, 131072, 128), (8, 32, 8, 4, 8192, 64)):
        ns = lib.fa2_decode_num_splits(B, Hkv, cap, d)
        need = lib.fa2_decode_workspace_bytes(B, Hq, Hkv, q, cap, d, 0)
        assert ns > 1 and need == lib.fa2_decode_workspace_bytes(B, Hq, Hkv, q, cap, d, ns)
        qq = 5 if Hq // Hkv * 5 > 32 else 33      # more than 32 rows: refused (-6), but only after the workspace check (-5)
        need_q = lib.fa2_decode_workspace_bytes(B, Hq, Hkv, qq, cap, d, 0)
        tail = (B, Hq, Hkv, qq, cap, d, ctypes.c_float(0.125))
        for fp8 in (False, True):
            def call(wsb):
                if fp8:
                    return lib.fa2_forward_decode_fp8kv(*(ONE,) * 9, *tail, 0, 2, 1, 0, ONE, wsb, None)
                return lib.fa2_forward_decode(*(ONE,) * 7, *tail, 0, 1, 0, ONE, wsb, None)
            assert call(need_q - 1) == -5 and call(need_q) == -6, (fp8, B, Hq, Hkv)
