"""CPU: the float64 reference for attention with sinks (tests/sink_ref.py) is pinned to regimes.ref_attention, and the new entry
points validate their arguments without a device.

THE EXTRA-KEY CONSTRUCTION.  A sink is a key with score s_h and value 0, and plain attention can hold such a key at the price of
one head dimension: put 1 in the last component of every query and 0 in the last component of every key, and prepend the key
(0, ..., 0, s_h / scale) with V = 0.  Its score is scale . 1 . s_h / scale = s_h on every row, the real keys' scores are
unchanged, and ref_attention on the d-wide problem with N_k + 1 keys must give the O, L, dQ (but for the last component, which
there carries dS_sink s_h) and the real keys' dK and dV of ref_attention_sink; the last component of the extra key's dK is
scale sum_rows dS_sink = scale dsink.  Under the bottom-right causal mask the prepended key is visible to row i iff
0 <= i + N_k + 1 - N_q: the construction holds for N_q <= N_k + 1, the shapes used here."""
import ctypes

import numpy as np
import pytest
import torch

from regimes import ref_attention
from sink_ref import dsink_from_kernel_feed, ref_attention_sink

H, D = 3, 8
SINKS = np.array([-1.5, 2.0, 6.0])


def _data(seed, nq, nk, b=2):
    r = np.random.default_rng(seed)
    q, g = r.uniform(-1, 1, (b, H, nq, D)), r.uniform(-1, 1, (b, H, nq, D))
    k, v = r.uniform(-1, 1, (b, H, nk, D)), r.uniform(-1, 1, (b, H, nk, D)) + 0.3
    q[..., -1], k[..., -1] = 1.0, 0.0
    return q, k, v, g


@pytest.mark.parametrize("nq,nk,causal", [(7, 7, False), (7, 7, True), (5, 11, True), (11, 5, False), (6, 5, True), (1, 1, True)])
def test_reference_is_plain_attention_with_one_more_key(nq, nk, causal):
    scale = 0.37
    q, k, v, g = _data(100 + 13 * nq + nk, nq, nk)
    O, L, dQ, dK, dV, dsink, mag = ref_attention_sink(q, k, v, g, scale, causal, SINKS)
    extra = np.zeros((2, H, 1, D))
    extra[..., 0, -1] = SINKS[None, :] / scale
    k1, v1 = np.concatenate([extra, k], axis=-2), np.concatenate([np.zeros((2, H, 1, D)), v], axis=-2)
    O1, L1, dQ1, dK1, dV1 = ref_attention(q, k1, v1, g, scale, causal)
    tol = dict(rtol=0, atol=1e-12)
    np.testing.assert_allclose(O, O1, **tol)
    np.testing.assert_allclose(L, L1, **tol)
    np.testing.assert_allclose(dQ[..., :-1], dQ1[..., :-1], **tol)
    assert (dQ[..., -1] == 0).all()
    np.testing.assert_allclose(dK, dK1[..., 1:, :], **tol)
    np.testing.assert_allclose(dV, dV1[..., 1:, :], **tol)
    np.testing.assert_allclose(dsink, dK1[..., 0, -1].sum(axis=0) / scale, **tol)
    # what the kernels compute it from: L and O in full precision give the same number
    np.testing.assert_allclose(dsink_from_kernel_feed(SINKS, L, O, g), dsink, **tol)
    # the magnitudes bound what they are the magnitudes of
    assert (np.abs(dsink) <= mag["PD"] + 1e-15).all() and (mag["PD"] <= mag["M"] + 1e-15).all() and (mag["M"] <= mag["A"]).all()


@pytest.mark.parametrize("nq,nk,causal", [(7, 7, True), (11, 5, True), (5, 11, False), (4, 0, False)])
def test_minus_infinity_is_no_sink(nq, nk, causal):
    q, k, v, g = _data(300 + 13 * nq + nk, nq, nk)
    got = ref_attention_sink(q, k, v, g, 0.5, causal, np.full(H, -np.inf))
    for a, b in zip(got[:5], ref_attention(q, k, v, g, 0.5, causal)):
        assert np.array_equal(a, b)
    assert (got[5] == 0).all() and all((x == 0).all() for x in got[6].values())
    # one head without a sink beside two with one: that head is plain attention, the others are not
    mixed = ref_attention_sink(q, k, v, g, 0.5, causal, np.array([1.0, -np.inf, 3.0]))
    plain = ref_attention(q, k, v, g, 0.5, causal)
    for a, b in zip(mixed[:5], plain):
        assert np.array_equal(a[:, 1], b[:, 1])
    assert mixed[5][1] == 0
    if nk:
        assert not np.array_equal(mixed[0][:, 0], plain[0][:, 0])


def test_rows_without_a_key_follow_the_rule():
    nq, nk = 9, 4                                    # causal: rows 0 .. 4 see no key
    q, k, v, g = _data(500, nq, nk)
    sinks = np.array([0.7, -np.inf, -20.0])
    O, L, dQ, dK, dV, dsink, mag = ref_attention_sink(q, k, v, g, 0.5, True, sinks)
    none = slice(0, nq - nk)
    assert (O[:, :, none] == 0).all() and (dQ[:, :, none] == 0).all()
    assert (L[:, 0, none] == 0.7).all() and np.isneginf(L[:, 1, none]).all() and (L[:, 2, none] == -20.0).all()
    assert np.isfinite(L[:, :, nq - nk:]).all()
    for t in (O, dQ, dK, dV, dsink):
        assert np.isfinite(t).all()
    # those rows add nothing to dsink: the sum over the rows with a key alone is the whole of it
    seen = ref_attention_sink(q[:, :, nq - nk:], k, v, g[:, :, nq - nk:], 0.5, True, sinks)
    np.testing.assert_allclose(dsink, seen[5], rtol=0, atol=1e-14)
    # no key anywhere: every row is its sink
    O, L, dQ, dK, dV, dsink, mag = ref_attention_sink(q, k[:, :, :0], v[:, :, :0], g, 0.5, False, sinks)
    assert (O == 0).all() and (dQ == 0).all() and (dsink == 0).all() and dK.shape[-2] == 0
    assert (L[:, 0] == 0.7).all() and np.isneginf(L[:, 1]).all()


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
def _host(b=1, h=4, hkv=2, nq=5, nk=7, d=64, dtype=torch.bfloat16):
    return torch.zeros(b, h, nq, d, dtype=dtype), torch.zeros(b, hkv, nk, d, dtype=dtype), torch.zeros(b, hkv, nk, d, dtype=dtype)


BAD_SINKS = [("shape", lambda: torch.zeros(5), r"sink: shape"), ("shape", lambda: torch.zeros(4, 1), r"sink: shape"),
             ("dtype", lambda: torch.zeros(4, dtype=torch.bfloat16), r"sink: dtype"),
             ("dtype", lambda: torch.zeros(4, dtype=torch.float64), r"sink: dtype"),
             ("contiguity", lambda: torch.zeros(8)[::2], r"sink must be contiguous"),
             ("device", lambda: torch.zeros(4), r"sink must be a device tensor"),
             ("type", lambda: [0.0] * 4, r"sink must be a torch tensor")]


@pytest.mark.parametrize("what,make,message", BAD_SINKS, ids=[f"{w}-{i}" for i, (w, _, _) in enumerate(BAD_SINKS)])
def test_ops_validate_the_sink_before_anything_reaches_the_library(what, make, message):
    """The C ABI takes raw pointers: a sink of the wrong shape, dtype, layout or device is refused in Python.  (Host tensors
    throughout: the sink is looked at first, and a sink that is right in everything but its device is refused for that.)"""
    import cuda_flashattention_amd as fa
    from cuda_flashattention_amd import ops
    Q, K, V = _host()
    O, L = torch.zeros_like(Q), torch.zeros(Q.shape[:3])
    with pytest.raises(ValueError, match=message):
        fa.flash_attention_2_qk_forward(Q, K, V, sink=make())
    with pytest.raises(ValueError, match=message):
        fa.flash_attention_2_qk_backward(Q, K, V, O, L, O, sink=make())
    plan = fa.VarlenPlan([0, 5], [0, 7])
    with pytest.raises(ValueError, match=message):
        fa.flash_attention_2_varlen_forward(Q[0], K[0], V[0], plan, sink=make())
    with pytest.raises(ValueError, match=message):
        fa.flash_attention_2_varlen_backward(Q[0], K[0], V[0], O[0], L[0], O[0], plan, sink=make())
    if what != "type":
        with pytest.raises(ValueError, match=message.replace("sink", "dsink")):
            ops._sink_arg(make(), Q, 1, "dsink")


def test_ops_refuse_a_sink_beside_tensors_that_are_not_bf16_and_a_gradient_without_a_sink():
    import cuda_flashattention_amd as fa
    Q, K, V = _host(dtype=torch.float32)
    sink = torch.zeros(4)
    with pytest.raises(ValueError, match="attention sinks are bf16"):
        fa.flash_attention_2_qk_forward(Q, K, V, sink=sink)
    with pytest.raises(ValueError, match="attention sinks are bf16"):
        fa.attention(Q, K, V, sink=sink)
    with pytest.raises(ValueError, match="attention sinks are bf16"):
        fa.attention_varlen(Q[0], K[0], V[0], fa.VarlenPlan([0, 5], [0, 7]), sink=sink)
    with pytest.raises(ValueError, match="bf16 or fp32"):
        fa.attention_qk(*_host(), sink=torch.zeros(4, dtype=torch.float16))
    Q, K, V = _host()
    with pytest.raises(ValueError, match="dsink belongs to a call with sink="):
        fa.flash_attention_2_qk_backward(Q, K, V, Q, torch.zeros(Q.shape[:3]), Q, dsink=sink)
    with pytest.raises(ValueError, match="dsink belongs to a call with sink="):
        fa.flash_attention_2_varlen_backward(Q[0], K[0], V[0], Q[0], torch.zeros(Q.shape[1:3]), Q[0], fa.VarlenPlan([0, 5], [0, 7]), dsink=sink)


def test_c_entry_points_report_null_pointers_and_the_dtype():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    one = ctypes.c_void_p(16)                        # never dereferenced: validation fails first
    fwd = lambda t, dtype=0: lib.fa2_forward_sink(*t, 2, 4, 2, 300, 500, 128, 0.1, dtype, 1, None)
    assert fwd([one] * 6, 1) == -4 and fwd([one] * 6, 2) == -4 and fwd([one] * 6, 7) == -4
    bwd = lambda t, dtype=0: lib.fa2_backward_sink(*t, 2, 4, 2, 300, 500, 128, 0.1, dtype, 1, one, 1 << 30, None, 7)
    assert bwd([one] * 11, 1) == -4
    blob = np.zeros(4096, dtype=np.uint8)
    cq, ck = np.array([0, 300], dtype=np.int32), np.array([0, 500], dtype=np.int32)
    assert lib.fa2_varlen_plan_build_qk(cq.ctypes.data, ck.ctypes.data, 1, blob.ctypes.data, blob.size) == 0
    tail = (4, 2, 300, 500, 128, 0.1)
    vfwd = lambda t, dtype=0: lib.fa2_forward_varlen_sink(*t, *tail, dtype, 1, blob.ctypes.data, one, blob.size, None)
    vbwd = lambda t, dtype=0: lib.fa2_backward_varlen_sink(*t, *tail, dtype, 1, blob.ctypes.data, one, blob.size, one, 1 << 30, None)
    assert vfwd([one] * 6, 1) == -4 and vbwd([one] * 11, 1) == -4
    for call, n in ((fwd, 6), (bwd, 11), (vfwd, 6), (vbwd, 11)):
        for i in range(n):                           # every tensor in turn, the sink (index 3) and dsink (index 10) among them
            args = [one] * n
            args[i] = None
            assert call(args) == -1, (call, i)
    assert lib.fa2_backward_sink_workspace_bytes(2, 4, 2, 300, 500, 128, 0) == lib.fa2_backward_qk_workspace_bytes(2, 4, 2, 300, 500, 128, 0)
    assert lib.fa2_backward_sink_workspace_bytes(2, 4, 2, 1024, 1024, 128, 0) == lib.fa2_backward_gqa_workspace_bytes(2, 4, 2, 1024, 128, 0)
    assert lib.fa2_backward_varlen_sink_workspace_bytes(*tail[:5], 0) == lib.fa2_backward_varlen_qk_workspace_bytes(*tail[:5], 0) > 0
