"""CPU: grouped-query attention (K, V of shape [B, H_kv, N, d], H_kv dividing H_q) -- what the Python mirror and the C ABI
refuse before any pointer is read, and the workspace fa2_backward_gqa_workspace_bytes promises."""
import ctypes

import pytest

torch = pytest.importorskip("torch")


class _Fake(torch.Tensor):
    """A CPU tensor that claims to live on a device: lets the validation logic run without a GPU."""
    @property
    def is_cuda(self):
        return True


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_Fake)


def test_ops_refuse_bad_grouped_shapes():
    from cuda_flashattention_amd import ops
    Q, L = _t(1, 8, 64, 128), _t(1, 8, 64, dtype=torch.float32)
    K3, K2 = _t(1, 3, 64, 128), _t(1, 2, 64, 128)
    with pytest.raises(ValueError, match="shape"):          # 3 does not divide 8
        ops.flash_attention_2_forward(Q, K3, K3)
    with pytest.raises(ValueError, match="shape"):
        ops.flash_attention_2_backward(Q, K3, K3, Q, L, Q)
    for bad in (_t(2, 2, 64, 128), _t(1, 2, 32, 128), _t(1, 2, 64, 64)):      # batch, length, head_dim differ from Q's
        with pytest.raises(ValueError, match="K.*shape"):
            ops.flash_attention_2_forward(Q, bad, bad)
    with pytest.raises(ValueError, match="V"):              # V must match K, not Q
        ops.flash_attention_2_forward(Q, K2, _t(1, 4, 64, 128))
    with pytest.raises(ValueError, match="V"):
        ops.flash_attention_2_backward(Q, K2, Q, Q, L, Q)
    with pytest.raises(ValueError, match="dK"):             # dK has K's shape
        ops.flash_attention_2_backward(Q, K2, K2, Q, L, Q, dK=_t(1, 8, 64, 128))
    with pytest.raises(ValueError, match="dV"):
        ops.flash_attention_2_backward(Q, K2, K2, Q, L, Q, dV=_t(1, 8, 64, 128))
    Qf, Kf = _t(1, 8, 64, 128, dtype=torch.float32), _t(1, 2, 64, 128, dtype=torch.float32)
    with pytest.raises(ValueError, match="bf16"):           # grouped tensors are bf16 in this version
        ops.flash_attention_2_forward(Qf, Kf, Kf)
    with pytest.raises(ValueError, match="bf16"):
        ops.flash_attention_2_backward(Qf, Kf, Kf, Qf, L, Qf)


def test_ops_accept_grouped_shapes_up_to_the_workspace_check():
    """K [1,2,64,128] against Q [1,8,64,128] passes every shape check: the call gets as far as the workspace argument (a host
    tensor here, so no kernel is reached)."""
    from cuda_flashattention_amd import ops
    Q, L, K2 = _t(1, 8, 64, 128), _t(1, 8, 64, dtype=torch.float32), _t(1, 2, 64, 128)
    with pytest.raises(ValueError, match="workspace"):
        ops.flash_attention_2_backward(Q, K2, K2, Q, L, Q, workspace=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="workspace"):      # caller-owned dK / dV of K's shape
        ops.flash_attention_2_backward(Q, K2, K2, Q, L, Q, dK=_t(1, 2, 64, 128), dV=_t(1, 2, 64, 128),
                                       workspace=torch.zeros(16, dtype=torch.uint8))
    K1 = _t(1, 1, 64, 128)                                  # multi-query attention
    with pytest.raises(ValueError, match="workspace"):
        ops.flash_attention_2_backward(Q, K1, K1, Q, L, Q, workspace=torch.zeros(16, dtype=torch.uint8))


def test_gqa_status_codes():
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first
    fwd = lambda *a: lib.fa2_forward_gqa(one, one, one, one, one, *a, None)
    assert lib.fa2_forward_gqa(None, one, one, one, one, 1, 8, 2, 128, 128, 0.125, 0, 0, None) == -1
    assert fwd(1, 8, 3, 128, 128, 0.125, 0, 0) == -2        # B, H_q, H_kv, N, d, scale, dtype, causal
    assert fwd(1, 8, 0, 128, 128, 0.125, 0, 0) == -2
    assert fwd(1, 8, -2, 128, 128, 0.125, 0, 0) == -2
    assert fwd(1, 8, 16, 128, 128, 0.125, 0, 0) == -2       # more K/V heads than query heads
    assert fwd(1, 8, 2, 0, 128, 0.125, 0, 0) == -2
    assert fwd(1, 8, 2, 128, 96, 0.125, 0, 0) == -3
    assert fwd(1, 8, 2, 128, 128, 0.125, 1, 0) == -4        # fp32
    assert fwd(1, 8, 2, 128, 128, 0.125, 2, 0) == -4        # fp8
    bwd = lambda *a: lib.fa2_backward_gqa(*([one] * 9), *a)
    assert lib.fa2_backward_gqa(*([one] * 8), None, 1, 8, 2, 128, 128, 0.125, 0, 0, one, 1 << 30, None, 7) == -1
    big = 1 << 30
    assert bwd(1, 8, 3, 128, 128, 0.125, 0, 0, one, big, None, 7) == -2
    assert bwd(1, 8, 0, 128, 128, 0.125, 0, 0, one, big, None, 7) == -2
    assert bwd(1, 8, 2, 128, 96, 0.125, 0, 0, one, big, None, 7) == -3
    assert bwd(1, 8, 2, 128, 128, 0.125, 1, 0, one, big, None, 7) == -4
    assert bwd(1, 8, 2, 128, 128, 0.125, 2, 0, one, big, None, 7) == -4
    assert bwd(1, 8, 2, 128, 128, 0.125, 0, 0, None, 0, None, 7) == -5
    need = lib.fa2_backward_gqa_workspace_bytes(1, 8, 2, 1024, 128, 0)
    assert bwd(1, 8, 2, 1024, 128, 0.125, 0, 0, one, need - 1, None, 7) == -5
    # a workspace sized for the multi-head problem is too small where the single kernel's partials are needed
    assert bwd(1, 8, 2, 1024, 128, 0.125, 0, 0, one, lib.fa2_backward_workspace_bytes(1, 8, 1024, 128, 0), None, 7) == -5
    why = ctypes.c_char_p()
    assert lib.fa2_backward_gqa_plan(1, 8, 3, 1024, 128, 0, 0, ctypes.byref(why)) == -2
    assert lib.fa2_backward_gqa_plan(1, 8, 0, 1024, 128, 0, 0, ctypes.byref(why)) == -2
    assert lib.fa2_backward_gqa_plan(1, 8, 2, 1024, 96, 0, 0, ctypes.byref(why)) == -3
    assert lib.fa2_backward_gqa_plan(1, 8, 2, 1024, 128, 1, 0, ctypes.byref(why)) == -4
    assert lib.fa2_backward_gqa_plan(1, 8, 2, 300, 128, 0, 0, ctypes.byref(why)) == 2 and b"multiple of 256" in why.value
    assert lib.fa2_backward_gqa_workspace_bytes(1, 8, 3, 1024, 128, 0) == 0
    assert lib.fa2_backward_gqa_workspace_bytes(1, 8, 0, 1024, 128, 0) == 0


@pytest.mark.parametrize("B,H,N,d", [(4, 16, 8192, 128),      # aligned, single kernel
                                     (2, 14, 2000, 128),      # ragged, single kernel
                                     (1, 8, 1024, 64),        # head_dim 64, single kernel
                                     (2, 6, 300, 128),        # two kernels
                                     (1, 8, 800, 64)])        # two kernels
def test_gqa_workspace_bytes(B, H, N, d):
    from cuda_flashattention_amd import _capi
    lib = _capi.lib()
    mha = lib.fa2_backward_workspace_bytes(B, H, N, d, 0)
    assert lib.fa2_backward_gqa_workspace_bytes(B, H, H, N, d, 0) == mha
    npad = (N + 255) // 256 * 256
    for Hkv in (h for h in range(1, H) if H % h == 0):
        got = lib.fa2_backward_gqa_workspace_bytes(B, H, Hkv, N, d, 0)
        assert mha <= got <= mha + 2 * B * H * npad * d * 4 + 4096, (Hkv, got, mha)
        if lib.fa2_backward_fused_workspace_bytes(B, H, N, d) == 0:       # the two kernels need nothing more
            assert got == mha
        else:
            assert got > mha
