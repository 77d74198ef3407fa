"""Host-side mirror of the reference's operator interface for the FA2 hot path.

The reference's interface is three free functions taking raw device pointers
(flash_attention_2_forward / flash_attention_2_backward / ring_attention_forward, see
include/fa2_mi355x.h for file:line).  These wrappers keep the same names and argument
meaning, take torch tensors only as *device memory* (pointer + shape), and call the C ABI
through ctypes.  torch is plumbing here: allocation, streams, nothing numerical.
"""
import ctypes
import math

import numpy as np
import torch

from . import _capi
from ._capi import FA2_DTYPE_BF16, FA2_DTYPE_F32, FA2_DTYPE_FP8_E4M3, check


def _dtype_code(t):
    if t.dtype == torch.bfloat16:
        return FA2_DTYPE_BF16
    if t.dtype == torch.float32:
        return FA2_DTYPE_F32
    if t.dtype == torch.float8_e4m3fn:
        return FA2_DTYPE_FP8_E4M3
    raise TypeError(f"unsupported dtype {t.dtype}: bf16, fp32 or float8_e4m3fn (forward only) expected")


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _scale(softmax_scale, d):
    """The softmax scale a call runs with: the caller's, or 1 / sqrt(head_dim)."""
    return float(softmax_scale) if softmax_scale is not None else 1.0 / math.sqrt(d)


def _nbytes(t):
    return t.numel() * t.element_size()


def _workspace_arg(workspace, Q):
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or not workspace.is_contiguous() or workspace.device != Q.device:
        raise ValueError("workspace must be a contiguous device tensor on Q's device")
    return workspace


def _bhnd(x, name):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if not x.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous [B][H][N][d] (got strides {tuple(x.stride())}; call .contiguous())")
    if x.dim() == 2:
        return 1, 1, x.shape[0], x.shape[1]
    if x.dim() == 4:
        return tuple(x.shape)
    raise ValueError(f"{name}: expected [N,d] or [B,H,N,d], got {tuple(x.shape)}")


def _like(x, name, ref, shape, dtype):
    """The C ABI takes raw pointers: everything it will read or write as a dense [B][H][N][d] (or [B][H][N]) tensor is
    checked here -- device, contiguity, shape, dtype -- instead of becoming a silent out-of-bounds access."""
    if _bhnd(x, name) != shape and tuple(x.shape) != shape:
        raise ValueError(f"{name}: shape {tuple(x.shape)} does not match {shape}")
    if x.dtype != dtype:
        raise ValueError(f"{name}: dtype {x.dtype}, expected {dtype}")
    if x.device != ref.device:
        raise ValueError(f"{name} is on {x.device}, expected {ref.device}")
    return x


def _kv_shape(Q, K, V, shape):
    """K's shape for a Q of `shape`: Q's own, or (grouped-query attention, [B, H_kv, N, d] with H_kv dividing H) fewer heads.
    V must match K; both must have Q's dtype.  Grouped tensors are bf16."""
    B, H, N, d = shape
    kshape = _bhnd(K, "K")
    if Q.dim() != 4 or K.dim() != 4 or kshape == shape:
        _like(K, "K", Q, shape, Q.dtype)
        kshape = shape
    else:
        Hkv = kshape[1]
        if (kshape[0], kshape[2], kshape[3]) != (B, N, d) or Hkv < 1 or H % Hkv != 0:
            raise ValueError(f"K: shape {tuple(K.shape)} does not match {shape} (grouped-query attention: [B, H_kv, N, d] "
                             f"with H_kv dividing H = {H})")
        _like(K, "K", Q, kshape, Q.dtype)
        if Q.dtype != torch.bfloat16:
            raise ValueError(f"K: {Hkv} key/value heads against {H} query heads needs bf16 tensors, got {Q.dtype}")
    _like(V, "V", Q, kshape, Q.dtype)
    return kshape


def _rows(x, name, ref, B, H, N):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous device tensor")
    if x.dtype != torch.float32 or x.numel() != B * H * N or x.device != ref.device:
        raise ValueError(f"{name}: expected fp32 [B,H,N] = {B * H * N} elements on {ref.device}, got {x.dtype} {tuple(x.shape)}")
    return x


def _sink_arg(sink, Q, heads_dim, name="sink"):
    """An attention-sink tensor (or its gradient) beside Q ([B, H, N, d]: heads_dim 1; packed [H, T, d]: heads_dim 0), checked like
    every other tensor the C ABI takes on trust: a contiguous fp32 device tensor of H_q elements on Q's device, and Q in bf16.
    (A Q that is no tensor of that rank is the shape check's to refuse.)"""
    if not isinstance(sink, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if not isinstance(Q, torch.Tensor) or Q.dim() != (4 if heads_dim else 3):
        return sink
    if Q.dtype != torch.bfloat16:
        raise ValueError(f"{name}: attention sinks are bf16 in this version, Q is {Q.dtype}")
    H = Q.shape[heads_dim]
    if sink.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {sink.dtype}, expected torch.float32 (the autograd ops also take a bf16 parameter)")
    if sink.dim() != 1 or sink.numel() != H:
        raise ValueError(f"{name}: shape {tuple(sink.shape)}, expected ({H},): one logit per query head")
    if not sink.is_contiguous():
        raise ValueError(f"{name} must be contiguous (got stride {tuple(sink.stride())}; call .contiguous())")
    if not sink.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if sink.device != Q.device:
        raise ValueError(f"{name} is on {sink.device}, expected {Q.device}")
    return sink


def _sink_param(sink):
    """What the autograd ops call with: the fp32 copy of a bf16 or fp32 sink parameter (None stays None)."""
    if sink is None:
        return None
    if not isinstance(sink, torch.Tensor) or sink.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"sink: a bf16 or fp32 tensor of H_q logits expected, got {sink.dtype if isinstance(sink, torch.Tensor) else type(sink)}")
    return sink.detach().float().contiguous()


def forward_fp8_workspace(B, H, N, d, device="cuda"):
    """Scratch for the fp8 forward (V transposed + key-norm maxima): allocate once, pass as workspace=."""
    return torch.empty(_capi.lib().fa2_forward_fp8_workspace_bytes(B, H, N, d), dtype=torch.uint8, device=device)


def flash_attention_2_forward(Q, K, V, softmax_scale=None, causal=False, O=None, L=None, stream=None, workspace=None,
                              descale=None):
    """O, L = FA2 forward.  Mirrors flash_attention_2_forward(Q,K,V,O,L,seq_len,head_dim,scale)
    (reference 02_forward/flash_attention_kernel.cu:300-309) with B,H,dtype,causal,stream added.
    Tensors [N,d] or [B,H,N,d]; L is fp32 [.., N] natural-log LSE.  Grouped-query attention (bf16): K and V may be
    [B,H_kv,N,d] with H_kv dividing H -- query head h attends K/V head h // (H // H_kv).  fp8 (e4m3) inputs only: workspace= a caller-owned
    scratch tensor (forward_fp8_workspace; without it every call takes one from the stream-ordered allocator), descale=
    (q, k, v) per-tensor descales of tensors stored as x / descale (fa2_forward_fp8_scaled)."""
    B, H, N, d = shape = _bhnd(Q, "Q")
    Hkv = _kv_shape(Q, K, V, shape)[1]
    scale = _scale(softmax_scale, d)
    odt = torch.bfloat16 if Q.dtype == torch.float8_e4m3fn else Q.dtype      # fp8 inputs (OCP e4m3, d = 128) produce a bf16 O
    if O is None:
        O = torch.empty(Q.shape, dtype=odt, device=Q.device)
    if L is None:
        L = torch.empty(Q.shape[:-1], dtype=torch.float32, device=Q.device)
    _like(O, "O", Q, shape, odt)
    _rows(L, "L", Q, B, H, N)
    if Q.dtype == torch.float8_e4m3fn and (workspace is not None or descale is not None):
        if workspace is None:
            workspace = forward_fp8_workspace(B, H, N, d, Q.device)
        _workspace_arg(workspace, Q)
        dq, dk, dv = (1.0, 1.0, 1.0) if descale is None else (float(x) for x in descale)
        st = _capi.lib().fa2_forward_fp8_scaled(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), B, H, N, d, scale,
                                                dq, dk, dv, 1 if causal else 0, workspace.data_ptr(), _nbytes(workspace), _stream_ptr(stream))
        check(st, "fa2_forward_fp8_scaled")
        return O, L
    if workspace is not None or descale is not None:
        raise ValueError("workspace= / descale= belong to the fp8 (float8_e4m3fn) forward")
    lib, ptrs = _capi.lib(), (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr())
    tail = (N, d, scale, _dtype_code(Q), 1 if causal else 0, _stream_ptr(stream))
    if Hkv != H:
        check(lib.fa2_forward_gqa(*ptrs, B, H, Hkv, *tail), "fa2_forward_gqa")
    else:
        check(lib.fa2_forward(*ptrs, B, H, *tail), "fa2_forward")
    return O, L


def flash_attention_2_backward(Q, K, V, O, L, dO, softmax_scale=None, causal=False,
                               dQ=None, dK=None, dV=None, workspace=None, stream=None, phases=7):
    """dQ, dK, dV = FA2 backward.  Mirrors flash_attention_2_backward(Q,K,V,O,L,dO,dQ,dK,dV,...)
    (reference 02_backward/flash_attention_backward_kernel.cu:249-262).  dO must be contiguous (autograd often hands
    over an expanded or transposed view: call .contiguous() on it first -- the C ABI reads a dense tensor).
    Grouped-query attention (bf16): K, V and with them dK, dV may be [B,H_kv,N,d] with H_kv dividing H."""
    B, H, N, d = shape = _bhnd(Q, "Q")
    gdt = torch.bfloat16 if Q.dtype == torch.float8_e4m3fn else Q.dtype       # what the forward produced for fp8 inputs
    kshape = _kv_shape(Q, K, V, shape)
    Hkv = kshape[1]
    for n, t, dt in (("O", O, gdt), ("dO", dO, gdt)):
        _like(t, n, Q, shape, dt)
    _rows(L, "L", Q, B, H, N)
    scale = _scale(softmax_scale, d)
    dQ = torch.empty_like(Q) if dQ is None else _like(dQ, "dQ", Q, shape, Q.dtype)
    dK = torch.empty_like(K) if dK is None else _like(dK, "dK", Q, kshape, Q.dtype)
    dV = torch.empty_like(V) if dV is None else _like(dV, "dV", Q, kshape, Q.dtype)
    lib = _capi.lib()
    need = lib.fa2_backward_gqa_workspace_bytes(B, H, Hkv, N, d, _dtype_code(Q))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
    _workspace_arg(workspace, Q)
    ptrs = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), dO.data_ptr(), dQ.data_ptr(), dK.data_ptr(), dV.data_ptr())
    tail = (N, d, scale, _dtype_code(Q), 1 if causal else 0, workspace.data_ptr(), _nbytes(workspace), _stream_ptr(stream), int(phases))
    if Hkv != H:
        check(lib.fa2_backward_gqa(*ptrs, B, H, Hkv, *tail), "fa2_backward_gqa")
    else:
        check(lib.fa2_backward_phases(*ptrs, B, H, *tail), "fa2_backward")
    return dQ, dK, dV


def forward_step(Q, K, V, O, L, Oacc, M, softmax_scale, first, last, stream=None):
    """One resumable ring step (ring_attention_forward_kernel, ring_attention_kernel.cu:13-140)."""
    B, H, Nq, d = qshape = _bhnd(Q, "Q")
    _, _, Nk, _ = kshape = _bhnd(K, "K")
    if kshape != (B, H, Nk, d) or K.dtype != Q.dtype:
        raise ValueError("K must match Q in B, H, d and dtype")
    _like(V, "V", Q, kshape, Q.dtype)
    if O is not None:
        _like(O, "O", Q, qshape, Q.dtype)
    _rows(L, "L", Q, B, H, Nq)
    if Oacc is not None:
        _like(Oacc, "Oacc", Q, qshape, torch.float32)
    if M is not None:
        _rows(M, "M", Q, B, H, Nq)
    st = _capi.lib().fa2_forward_step(Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                                      O.data_ptr() if O is not None else None, L.data_ptr(),
                                      Oacc.data_ptr() if Oacc is not None else None,
                                      M.data_ptr() if M is not None else None,
                                      B, H, Nq, Nk, d, float(softmax_scale), _dtype_code(Q),
                                      1 if first else 0, 1 if last else 0, _stream_ptr(stream))
    check(st, "fa2_forward_step")


class _Attention(torch.autograd.Function):
    """flash_attention_2_forward / _backward as one differentiable op (device tensors in, device tensors out; the kernels
    are the only arithmetic).  Saves Q, K, V, O and the log-sum-exp L, as the reference's backward expects them
    (02_flash_attention_v2_backward/flash_attention_backward_kernel.cu:249-262)."""

    @staticmethod
    def forward(ctx, Q, K, V, softmax_scale, causal):
        Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
        scale = _scale(softmax_scale, Q.shape[-1])
        O, L = flash_attention_2_forward(Q, K, V, scale, causal=causal)
        ctx.save_for_backward(Q, K, V, O, L)
        ctx.scale, ctx.causal = scale, bool(causal)
        return O

    @staticmethod
    def backward(ctx, dO):
        Q, K, V, O, L = ctx.saved_tensors
        dQ, dK, dV = flash_attention_2_backward(Q, K, V, O, L, dO.contiguous(), ctx.scale, causal=ctx.causal)
        return dQ, dK, dV, None, None


def attention(Q, K, V, softmax_scale=None, causal=False, sink=None, return_lse=False):
    """softmax(scale Q K^T [causal]) V for [B, H, N, d] bf16 (d = 64 | 128) or fp32 (non-causal) device tensors, with gradients.
    bf16 K and V may have fewer heads ([B, H_kv, N, d], H_kv dividing H: grouped-query attention); their gradients have their shape.
    sink: attention sinks, a bf16 or fp32 tensor (a parameter) of H logits that join every row's softmax (attention_qk; bf16
    [B, H, N, d] tensors only), with its gradient.
    return_lse: return (O, L) with the differentiable log-sum-exp L (attention_qk; bf16 [B, H, N, d] tensors only).
    A convenience for callers that live in torch autograd; tests and bench.py call the two halves directly."""
    if sink is not None or return_lse:
        return attention_qk(Q, K, V, softmax_scale, causal, sink=sink, return_lse=return_lse)
    return _Attention.apply(Q, K, V, softmax_scale, causal)


def _qkv_shapes(Q, K, V, kname, vname, nk, family):
    """(B, H, H_kv, N_q, N_k, d) of Q [B, H, N_q, d] against K and V [B, H_kv, N_k, d], H_kv dividing H, Q in bf16: the relations
    between the shapes, with the names of the asking family (K or K_cache, N_k or N_cap) in the messages."""
    for n, t in (("Q", Q), (kname, K), (vname, V)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a [B, H, N, d] tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    B, H, Nq, d = Q.shape
    Bk, Hkv, Nk, dk = K.shape
    if (Bk, dk) != (B, d) or Hkv < 1 or H % Hkv != 0 or Nq < 1 or Nk < 1:
        raise ValueError(f"{kname}: shape {tuple(K.shape)} does not match Q {tuple(Q.shape)}: expected [B, H_kv, {nk}, d] with B = {B}, "
                         f"d = {d}, H_kv dividing H = {H} and N_q, {nk} >= 1")
    if tuple(V.shape) != tuple(K.shape):
        raise ValueError(f"{vname}: shape {tuple(V.shape)} does not match {kname} {tuple(K.shape)}")
    if Q.dtype != torch.bfloat16:
        raise ValueError(f"Q: dtype {Q.dtype}, expected torch.bfloat16 ({family} bf16 in this version)")
    return B, H, Hkv, Nq, Nk, d


def _qk_shapes(Q, K, V):
    """_qkv_shapes of a problem with its own query and key lengths, then what the C ABI takes on trust -- device, contiguity,
    dtype."""
    B, H, Hkv, Nq, Nk, d = shapes = _qkv_shapes(Q, K, V, "K", "V", "N_k", "different query and key lengths are")
    _bhnd(Q, "Q")
    _like(K, "K", Q, (B, Hkv, Nk, d), Q.dtype)
    _like(V, "V", Q, (B, Hkv, Nk, d), Q.dtype)
    return shapes


def flash_attention_2_qk_forward(Q, K, V, softmax_scale=None, causal=False, O=None, L=None, stream=None, sink=None):
    """O, L = FA2 forward of N_q queries against N_k keys (fa2_forward_qk): Q [B, H, N_q, d], K and V [B, H_kv, N_k, d] (H_kv
    dividing H), bf16, d = 64 | 128.  Cross-attention, or (causal) a prompt chunk against a longer contiguous KV cache: the mask
    is aligned bottom-right, key j visible to query i iff j <= i + N_k - N_q.  A query row that sees no key (causal, N_q > N_k)
    has O = 0 and L = -inf.  With N_q == N_k this is flash_attention_2_forward, bit for bit.
    sink (fa2_forward_sink): fp32 [H] device tensor of attention sinks, one logit per query head in natural units that joins every
    row's softmax and carries no value: L = log(exp(sink) + sum exp S), O = sum exp(S - L) v; -inf = no sink for that head; a
    row without a key then has L = sink."""
    if sink is not None:
        _sink_arg(sink, Q, 1)
    B, H, Hkv, Nq, Nk, d = _qk_shapes(Q, K, V)
    scale = _scale(softmax_scale, d)
    O = torch.empty_like(Q) if O is None else _like(O, "O", Q, (B, H, Nq, d), Q.dtype)
    L = torch.empty(B, H, Nq, dtype=torch.float32, device=Q.device) if L is None else _rows(L, "L", Q, B, H, Nq)
    lib, ptrs = _capi.lib(), (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr())
    tail = (B, H, Hkv, Nq, Nk, d, scale, FA2_DTYPE_BF16, 1 if causal else 0, _stream_ptr(stream))
    if sink is not None:
        check(lib.fa2_forward_sink(*ptrs[:3], sink.data_ptr(), *ptrs[3:], *tail), "fa2_forward_sink")
    else:
        check(lib.fa2_forward_qk(*ptrs, *tail), "fa2_forward_qk")
    return O, L


DECODE_MAX_ROWS = 32      # (H_q / H_kv) N_q: the query rows of one K/V head fill one 32-row MFMA tile (fa2_forward_decode)
DECODE_MAX_SPLITS = 256


_FP8_NOT_TAKEN = tuple(getattr(torch, n) for n in ("float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz") if hasattr(torch, n))


def _kv_dtypes(Q, K, V, kname, vname):
    """The dtypes of a decode call's caches beside a bf16 Q: both Q's, or both torch.float8_e4m3fn (OCP e4m3; returns True)."""
    for n, t in ((kname, K), (vname, V)):
        if t.dtype in _FP8_NOT_TAKEN:
            raise ValueError(f"{n}: dtype {t.dtype}; an fp8 cache is OCP e4m3 (torch.float8_e4m3fn), the encoding gfx950 converts natively")
    fp8 = [t.dtype == torch.float8_e4m3fn for t in (K, V)]
    if fp8[0] != fp8[1]:
        raise ValueError(f"{vname}: dtype {V.dtype} beside {kname} {K.dtype}: K and V are both torch.float8_e4m3fn or both {Q.dtype}")
    if all(fp8):
        return True
    for n, t in ((kname, K), (vname, V)):
        if t.dtype != Q.dtype:
            raise ValueError(f"{n}: dtype {t.dtype}, expected {Q.dtype}")
    return False


def _descale_arg(descale, Q, Hkv, name, fp8, kname):
    """k_descale / v_descale beside Q and e4m3 caches, checked like a sink (_sink_arg): a contiguous fp32 tensor of H_kv elements
    on Q's device.  The kernels read it ON THE DEVICE when they run, like seqlens_k; the host never does."""
    if not fp8:
        raise ValueError(f"{name}: a descale belongs to torch.float8_e4m3fn caches; {kname} is {Q.dtype} and holds its own values")
    if not isinstance(descale, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor (fp32 [{Hkv}] on Q's device: the kernels read it on the device when they run)")
    if descale.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {descale.dtype}, expected torch.float32")
    if descale.dim() != 1 or descale.numel() != Hkv:
        raise ValueError(f"{name}: shape {tuple(descale.shape)}, expected ({Hkv},): one descale per K/V head")
    if not descale.is_contiguous():
        raise ValueError(f"{name} must be contiguous (got stride {tuple(descale.stride())}; call .contiguous())")
    if not descale.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if descale.device != Q.device:
        raise ValueError(f"{name} is on {descale.device}, expected {Q.device}")
    return descale


def _ptr(t):
    return None if t is None else t.data_ptr()


def _decode_shapes(Q, K_cache, V_cache, max_rows=DECODE_MAX_ROWS):
    """(B, H, H_kv, N_q, N_cap, d, fp8) of a decode problem: Q [B, H, N_q, d] bf16 against caches [B, H_kv, N_cap, d], bf16 or (fp8)
    e4m3, H_kv dividing H.  Shapes and dtypes first (_qkv_shapes); device and contiguity are the caller's to check next.
    max_rows: the most rows (H / H_kv) N_q of a K/V head the call takes (None: any, the extend calls)."""
    B, H, Hkv, Nq, Ncap, d = _qkv_shapes(Q, K_cache, V_cache, "K_cache", "V_cache", "N_cap", "decode is")
    fp8 = _kv_dtypes(Q, K_cache, V_cache, "K_cache", "V_cache")
    if d not in (64, 128):
        raise ValueError(f"Q: head_dim {d}, expected 64 or 128")
    if max_rows is not None and (H // Hkv) * Nq > max_rows:
        raise ValueError(f"Q: {H // Hkv} query heads per K/V head x {Nq} query tokens = {(H // Hkv) * Nq} rows, decode takes at most "
                         f"{max_rows}: that is a prefill chunk, use flash_attention_2_qk_forward")
    return B, H, Hkv, Nq, Ncap, d, fp8


def _seqlens_arg(seqlens_k, Q, B):
    """seqlens_k beside Q: the kernels read it ON THE DEVICE at the time they run (that is what lets one captured graph serve
    every step), so a host list or a CPU tensor cannot stand in for it."""
    if not isinstance(seqlens_k, torch.Tensor):
        raise ValueError(f"seqlens_k must be an int32 device tensor of {B} lengths, got {type(seqlens_k).__name__}: the kernels read "
                         "the lengths on the device when they run, the host never does; use torch.tensor(..., dtype=torch.int32, device=Q.device)")
    if seqlens_k.dtype != torch.int32:
        raise ValueError(f"seqlens_k: dtype {seqlens_k.dtype}, expected torch.int32")
    if seqlens_k.dim() != 1 or seqlens_k.numel() != B:
        raise ValueError(f"seqlens_k: shape {tuple(seqlens_k.shape)}, expected ({B},): one length per sequence")
    if not seqlens_k.is_contiguous():
        raise ValueError(f"seqlens_k must be contiguous (got stride {tuple(seqlens_k.stride())}; call .contiguous())")
    if not seqlens_k.is_cuda:
        raise ValueError("seqlens_k is a CPU tensor: the kernels read the lengths on the device when they run (the host never "
                         "reads them), so it must live on Q's device")
    if seqlens_k.device != Q.device:
        raise ValueError(f"seqlens_k is on {seqlens_k.device}, expected {Q.device}")
    return seqlens_k


def _window_arg(window_left, causal):
    """window_left of a decode call: None (no window) or an int >= 0, the number of keys before its own position a query sees;
    the window is a causal one."""
    if window_left is None:
        return None
    if isinstance(window_left, bool) or not isinstance(window_left, int):
        raise ValueError(f"window_left: {window_left!r}, expected an int >= 0 (the keys before its own position a query sees; a "
                         "model's sliding_window = 128 is window_left = 127), or None for no window")
    if window_left < 0:
        raise ValueError(f"window_left: {window_left}, expected an int >= 0, or None for no window")
    if not causal:
        raise ValueError(f"window_left: {window_left} with causal=False; the window is a causal one (keys pos - window_left .. pos)")
    return min(window_left, 0x7fffffff)


def decode_num_splits(B, H_kv, kv_capacity, head_dim, *, q_len=1, window_left=None):
    """The split count n_splits=0 stands for (fa2_decode_num_splits): host arithmetic on the capacity, never on a length.
    window_left (with the call's q_len): the count of a windowed call (fa2_decode_window_num_splits), the same rule on
    min(kv_capacity, window_left + q_len + 127) keys."""
    w = _window_arg(window_left, True)
    if w is None:
        return _capi.lib().fa2_decode_num_splits(B, H_kv, kv_capacity, head_dim)
    return _capi.lib().fa2_decode_window_num_splits(B, H_kv, q_len, kv_capacity, head_dim, w)


def _decode_need(lib, B, H, Hkv, Nq, Ncap, d, n_splits, window_left, extend=False):
    """Workspace bytes of a decode call: n_splits = 0 resolved by the window's rule where there is one (extend: by the extend
    calls' rule, fa2_extend_workspace_bytes)."""
    if extend:
        return lib.fa2_extend_workspace_bytes(B, H, Hkv, Nq, Ncap, d, n_splits, -1 if window_left is None else window_left)
    if window_left is not None and n_splits == 0:
        n_splits = lib.fa2_decode_window_num_splits(B, Hkv, Nq, Ncap, d, window_left)
    return lib.fa2_decode_workspace_bytes(B, H, Hkv, Nq, Ncap, d, n_splits)


def decode_workspace(B, H, H_kv, N_q, kv_capacity, d, n_splits=0, device="cuda", *, q_len=1, window_left=None):
    """Scratch for flash_attention_2_decode (the splits' fp32 partials): allocate once, pass as workspace= (graph capture).
    window_left: the windowed call's (n_splits=0 is then decode_num_splits(..., q_len=N_q, window_left=window_left); the
    partials have N_q rows, q_len is accepted for symmetry with decode_num_splits and must equal N_q where both are given)."""
    w = _window_arg(window_left, True)
    if w is not None and q_len not in (1, N_q):
        raise ValueError(f"q_len: {q_len} beside N_q = {N_q}")
    return torch.empty(_decode_need(_capi.lib(), B, H, H_kv, N_q, kv_capacity, d, n_splits, w), dtype=torch.uint8, device=device)


def flash_attention_2_decode(Q, K_cache, V_cache, seqlens_k=None, softmax_scale=None, causal=True, sink=None, n_splits=0,
                             O=None, L=None, workspace=None, stream=None, k_descale=None, v_descale=None, window_left=None):
    """O, L = attention of a few new tokens per sequence against a preallocated KV cache (fa2_forward_decode): Q [B, H, N_q, d],
    K_cache and V_cache [B, H_kv, N_cap, d] (H_kv dividing H, (H / H_kv) N_q <= 32), bf16, d = 64 | 128.  INFERENCE ONLY: there is
    no autograd and no backward.
    seqlens_k: int32 [B] DEVICE tensor; sequence b attends keys [0, min(max(seqlens_k[b], 0), N_cap)) of its cache rows (None: all
    N_cap).  The host never reads it.  The N_q queries are the sequence's last N_q tokens, already in the cache; causal=True masks
    bottom-right (key j visible to query i iff j <= i + len_b - N_q).  A row without a visible key has O = 0 and L = -inf (L = sink
    with a sink).  sink: as flash_attention_2_qk_forward.
    n_splits: how many workgroups share a K/V head's keys, 1..256, or 0 = decode_num_splits(B, H_kv, N_cap, d).  More than one
    split needs a workspace (decode_workspace); it is allocated per call when omitted -- PASS ONE FOR GRAPH CAPTURE, with O, L and a
    seqlens_k tensor that is updated in place between replays.
    The returned (O, L) is what merge_states_forward takes: a cache held in two allocations is two calls (the first with
    causal=False and no sink, the last with the mask and the sink) and a merge.
    FP8 CACHES (fa2_forward_decode_fp8kv): K_cache and V_cache may both be torch.float8_e4m3fn (OCP e4m3), half the bytes to hold and
    to stream; Q, O and L are unchanged.  k_descale, v_descale: fp32 [H_kv] DEVICE tensors or None (= 1).  A cache stores x as
    x / descale[h_kv]: the scores are softmax_scale * k_descale[h] * (Q . K8) and O = v_descale[h] * P V8.  The kernels read them on
    the device when they run (positive and finite by contract; the host never reads them), so they may be updated in place under a
    captured graph.  Everything above holds unchanged; bytes past a length may be anything, e4m3's NaN codes included.
    WRITING THE CACHE: there is no append kernel inside this call; kv_cache_append is that call, bf16 or e4m3, and takes this
    call's seqlens_k tensor: bump the lengths in place, append, decode.  It stores (x / descale).clamp(-448, 448)
    .to(torch.float8_e4m3fn) byte for byte and saturates; a framework cast in its place needs that clamp --
    torch's cast does not saturate, an overflow becomes a NaN code.
    SLIDING WINDOW (fa2_forward_decode_window): window_left = None (no window, this call as it always was) or an int >= 0, the
    number of keys BEFORE its own position a query sees: with pos_i = i + len_b - N_q key j is visible iff pos_i - window_left <= j
    <= pos_i.  A model's sliding_window = 128 is window_left = 127; flash-attn's window_size = (left, 0) is window_left = left.
    It needs causal=True.  Only keys from rounddown(max(0, len_b - N_q - window_left), 128) on are split over the workgroups and
    read; cache rows BEFORE THE WINDOW (below len_b - N_q - window_left) may hold anything, NaN included.  n_splits=0 is then
    decode_num_splits(B, H_kv, N_cap, d, q_len=N_q, window_left=window_left) and the workspace decode_workspace(..., q_len=N_q,
    window_left=window_left).  bf16 and e4m3 caches, sinks, GQA and graph capture as above; a window >= N_cap - 1 is this call
    without one, bit for bit."""
    return _decode_call(Q, K_cache, V_cache, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace, stream, k_descale,
                        v_descale, window_left, False)


def _decode_call(Q, K_cache, V_cache, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace, stream, k_descale, v_descale,
                 window_left, extend):
    """flash_attention_2_decode (extend: flash_attention_2_extend, no row limit): one set of checks for both."""
    B, H, Hkv, Nq, Ncap, d, fp8 = _decode_shapes(Q, K_cache, V_cache, None if extend else DECODE_MAX_ROWS)
    if isinstance(n_splits, bool) or not isinstance(n_splits, int) or not 0 <= n_splits <= DECODE_MAX_SPLITS:
        raise ValueError(f"n_splits: {n_splits!r}, expected an int in 1..{DECODE_MAX_SPLITS}, or 0 for the default")
    window_left = _window_arg(window_left, causal)
    if seqlens_k is not None:
        _seqlens_arg(seqlens_k, Q, B)
    if sink is not None:
        _sink_arg(sink, Q, 1)
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if t is not None:
            _descale_arg(t, Q, Hkv, name, fp8, "K_cache")
    _bhnd(Q, "Q")
    _like(K_cache, "K_cache", Q, (B, Hkv, Ncap, d), K_cache.dtype)
    _like(V_cache, "V_cache", Q, (B, Hkv, Ncap, d), K_cache.dtype)
    scale = _scale(softmax_scale, d)
    if not scale > 0.0:
        raise ValueError(f"softmax_scale: {scale}, expected a positive number")
    O = torch.empty_like(Q) if O is None else _like(O, "O", Q, (B, H, Nq, d), Q.dtype)
    L = torch.empty(B, H, Nq, dtype=torch.float32, device=Q.device) if L is None else _rows(L, "L", Q, B, H, Nq)
    lib = _capi.lib()
    need = _decode_need(lib, B, H, Hkv, Nq, Ncap, d, n_splits, window_left, extend)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
    if workspace is not None and _nbytes(_workspace_arg(workspace, Q)) < need:
        raise ValueError(f"workspace: {_nbytes(workspace)} bytes, {need} needed ({'extend' if extend else 'decode'}_workspace)")
    head = (Q.data_ptr(), K_cache.data_ptr(), V_cache.data_ptr(), _ptr(seqlens_k), _ptr(sink))
    tail = (1 if causal else 0, n_splits, _ptr(workspace), 0 if workspace is None else _nbytes(workspace), _stream_ptr(stream))
    if extend:
        st = lib.fa2_forward_extend(*head, _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr(), B, H, Hkv, Nq, Ncap, d, scale,
                                    FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, *tail,
                                    -1 if window_left is None else window_left)
        check(st, "fa2_forward_extend")
    elif window_left is not None:
        st = lib.fa2_forward_decode_window(*head, _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr(), B, H, Hkv, Nq, Ncap, d,
                                           scale, FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, *tail, window_left)
        check(st, "fa2_forward_decode_window")
    elif fp8:
        st = lib.fa2_forward_decode_fp8kv(*head, _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr(), B, H, Hkv, Nq, Ncap, d,
                                          scale, FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3, *tail)
        check(st, "fa2_forward_decode_fp8kv")
    else:
        st = lib.fa2_forward_decode(*head, O.data_ptr(), L.data_ptr(), B, H, Hkv, Nq, Ncap, d, scale, FA2_DTYPE_BF16, *tail)
        check(st, "fa2_forward_decode")
    return O, L


DECODE_PAGE_GRAIN = 32      # kDecodeTile: a page is a whole number of the kernel's 32-key tiles, so a tile never crosses a page


def _block_table_arg(block_table, Q, B):
    """block_table beside Q: like seqlens_k it is read ON THE DEVICE when the kernels run (one captured graph serves every step as
    pages are assigned), so a host list or a CPU tensor cannot stand in for it.  Returns max_pages."""
    if not isinstance(block_table, torch.Tensor):
        raise ValueError(f"block_table must be an int32 device tensor [{B}, max_pages], got {type(block_table).__name__}: the kernels read "
                         "the table on the device when they run, the host never does; use torch.tensor(..., dtype=torch.int32, device=Q.device)")
    if block_table.dtype != torch.int32:
        raise ValueError(f"block_table: dtype {block_table.dtype}, expected torch.int32")
    if block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] < 1:
        raise ValueError(f"block_table: shape {tuple(block_table.shape)}, expected ({B}, max_pages): one row of page numbers per sequence")
    if not block_table.is_contiguous():
        raise ValueError(f"block_table must be contiguous (got stride {tuple(block_table.stride())}; call .contiguous())")
    if not block_table.is_cuda:
        raise ValueError("block_table is a CPU tensor: the kernels read the table on the device when they run (the host never "
                         "reads it), so it must live on Q's device")
    if block_table.device != Q.device:
        raise ValueError(f"block_table is on {block_table.device}, expected {Q.device}")
    return block_table.shape[1]


def _decode_paged_shapes(Q, K_pages, V_pages, max_rows=DECODE_MAX_ROWS):
    """(B, H, H_kv, N_q, n_pages, page_size, d, fp8) of a paged decode problem: Q [B, H, N_q, d] bf16 against pools [n_pages, H_kv,
    page_size, d], bf16 or (fp8) e4m3, H_kv dividing H, page_size a multiple of 32.  Device and contiguity are the caller's to check
    next.  max_rows: as _decode_shapes."""
    for n, t in (("Q", Q), ("K_pages", K_pages), ("V_pages", V_pages)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor ({'[B, H, N_q, d]' if n == 'Q' else '[n_pages, H_kv, page_size, d]'}), got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    B, H, Nq, d = Q.shape
    n_pages, Hkv, page_size, dk = K_pages.shape
    if dk != d or Hkv < 1 or H % Hkv != 0 or B < 1 or Nq < 1 or n_pages < 1 or page_size < 1:
        raise ValueError(f"K_pages: shape {tuple(K_pages.shape)} does not match Q {tuple(Q.shape)}: expected [n_pages, H_kv, page_size, d] "
                         f"with d = {d}, H_kv dividing H = {H} and n_pages, page_size >= 1")
    if page_size % DECODE_PAGE_GRAIN:
        raise ValueError(f"K_pages: page_size {page_size} is not a multiple of {DECODE_PAGE_GRAIN} (the kernel's key tile; a page of 16 "
                         "keys is not taken)")
    if tuple(V_pages.shape) != tuple(K_pages.shape):
        raise ValueError(f"V_pages: shape {tuple(V_pages.shape)} does not match K_pages {tuple(K_pages.shape)}")
    if Q.dtype != torch.bfloat16:
        raise ValueError(f"Q: dtype {Q.dtype}, expected torch.bfloat16 (decode is bf16 in this version)")
    fp8 = _kv_dtypes(Q, K_pages, V_pages, "K_pages", "V_pages")
    if d not in (64, 128):
        raise ValueError(f"Q: head_dim {d}, expected 64 or 128")
    if max_rows is not None and (H // Hkv) * Nq > max_rows:
        raise ValueError(f"Q: {H // Hkv} query heads per K/V head x {Nq} query tokens = {(H // Hkv) * Nq} rows, decode takes at most "
                         f"{max_rows}: that is a prefill chunk, use flash_attention_2_qk_forward")
    return B, H, Hkv, Nq, n_pages, page_size, d, fp8


def flash_attention_2_decode_paged(Q, K_pages, V_pages, block_table, seqlens_k=None, softmax_scale=None, causal=True, sink=None,
                                   n_splits=0, O=None, L=None, workspace=None, stream=None, k_descale=None, v_descale=None,
                                   window_left=None):
    """O, L = flash_attention_2_decode over a KV cache held as a pool of pages (fa2_forward_decode_paged): Q [B, H, N_q, d], K_pages
    and V_pages [n_pages, H_kv, page_size, d] (head-major; H_kv dividing H, (H / H_kv) N_q <= 32, page_size a multiple of 32, not
    necessarily a power of two), bf16, d = 64 | 128.  A token-major pool [n_pages, page_size, H_kv, d] needs one permute when it is
    allocated.  INFERENCE ONLY.
    block_table: int32 [B, max_pages] DEVICE tensor; key j of sequence b is row j % page_size of page block_table[b, j // page_size].
    Entries may repeat (shared prefix pages); entries past a sequence's last used page may hold anything; an entry in use is
    clamped to [0, n_pages) in the kernel.  The pool is only read, and its rows past a length may hold anything (NaN included).
    The host never reads the table.
    The logical capacity is kv_capacity = max_pages * page_size, and everything flash_attention_2_decode says about seqlens_k, the
    mask, rows without a key, sink and n_splits holds with it: n_splits=0 is decode_num_splits(B, H_kv, kv_capacity, d), the
    workspace is decode_workspace(B, H, H_kv, N_q, kv_capacity, d, n_splits) -- PASS ONE FOR GRAPH CAPTURE, with O, L, and seqlens_k
    and block_table tensors that are updated in place between replays (a sequence grows into a new page, pages are reassigned).
    With the same n_splits the result is bit for bit flash_attention_2_decode's on the gathered cache of that capacity.
    FP8 POOLS (fa2_forward_decode_paged_fp8kv): K_pages and V_pages may both be torch.float8_e4m3fn with k_descale, v_descale (fp32
    [H_kv] DEVICE tensors or None = 1; a pool stores x as x / descale[h_kv]), exactly as flash_attention_2_decode describes them:
    read on the device, never by the host; unused pages may hold any byte.
    WRITING THE POOL: there is no append kernel inside this call; kv_cache_append_paged is that call, through the same table and
    seqlens_k tensors: bump the lengths (and assign a new page's entry) in place, append, decode.
    SLIDING WINDOW (fa2_forward_decode_paged_window): window_left as flash_attention_2_decode describes it (None: no window).
    BEFORE THE WINDOW: with lo_b = max(0, len_b - N_q - window_left), every table entry of a page that lies wholly below lo_b may
    hold anything (stale, -1, out of range) and so may those pages: they are never read, prefetches included, so a server may
    free the pages behind the window and hand them to other sequences."""
    return _decode_paged_call(Q, K_pages, V_pages, block_table, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace, stream,
                              k_descale, v_descale, window_left, False)


def _decode_paged_call(Q, K_pages, V_pages, block_table, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace, stream,
                       k_descale, v_descale, window_left, extend):
    """flash_attention_2_decode_paged (extend: flash_attention_2_extend_paged, no row limit): one set of checks for both."""
    B, H, Hkv, Nq, n_pages, page_size, d, fp8 = _decode_paged_shapes(Q, K_pages, V_pages, None if extend else DECODE_MAX_ROWS)
    if isinstance(n_splits, bool) or not isinstance(n_splits, int) or not 0 <= n_splits <= DECODE_MAX_SPLITS:
        raise ValueError(f"n_splits: {n_splits!r}, expected an int in 1..{DECODE_MAX_SPLITS}, or 0 for the default")
    window_left = _window_arg(window_left, causal)
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):      # (they belong to the pools' dtype: checked with it)
        if t is not None:
            _descale_arg(t, Q, Hkv, name, fp8, "K_pages")
    max_pages = _block_table_arg(block_table, Q, B)
    kv_capacity = max_pages * page_size
    if kv_capacity > 0x7fffffff - (DECODE_MAX_SPLITS + 2) * 128:
        raise ValueError(f"block_table: {max_pages} pages of {page_size} keys is a capacity of {kv_capacity} keys, above what an int indexes")
    if seqlens_k is not None:
        _seqlens_arg(seqlens_k, Q, B)
    if sink is not None:
        _sink_arg(sink, Q, 1)
    _bhnd(Q, "Q")
    _like(K_pages, "K_pages", Q, (n_pages, Hkv, page_size, d), K_pages.dtype)
    _like(V_pages, "V_pages", Q, (n_pages, Hkv, page_size, d), K_pages.dtype)
    scale = _scale(softmax_scale, d)
    if not scale > 0.0:
        raise ValueError(f"softmax_scale: {scale}, expected a positive number")
    O = torch.empty_like(Q) if O is None else _like(O, "O", Q, (B, H, Nq, d), Q.dtype)
    L = torch.empty(B, H, Nq, dtype=torch.float32, device=Q.device) if L is None else _rows(L, "L", Q, B, H, Nq)
    lib = _capi.lib()
    need = _decode_need(lib, B, H, Hkv, Nq, kv_capacity, d, n_splits, window_left, extend)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
    if workspace is not None and _nbytes(_workspace_arg(workspace, Q)) < need:
        raise ValueError(f"workspace: {_nbytes(workspace)} bytes, {need} needed ({'extend' if extend else 'decode'}_workspace)")
    head = (Q.data_ptr(), K_pages.data_ptr(), V_pages.data_ptr(), block_table.data_ptr(), _ptr(seqlens_k), _ptr(sink))
    dims = (B, H, Hkv, Nq, n_pages, page_size, max_pages, d, scale)
    tail = (1 if causal else 0, n_splits, _ptr(workspace), 0 if workspace is None else _nbytes(workspace), _stream_ptr(stream))
    if extend:
        st = lib.fa2_forward_extend_paged(*head, _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr(), *dims, FA2_DTYPE_BF16,
                                          FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, *tail, -1 if window_left is None else window_left)
        check(st, "fa2_forward_extend_paged")
    elif window_left is not None:
        st = lib.fa2_forward_decode_paged_window(*head, _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr(), *dims,
                                                 FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, *tail, window_left)
        check(st, "fa2_forward_decode_paged_window")
    elif fp8:
        st = lib.fa2_forward_decode_paged_fp8kv(*head, _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr(), *dims,
                                                FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3, *tail)
        check(st, "fa2_forward_decode_paged_fp8kv")
    else:
        st = lib.fa2_forward_decode_paged(*head, O.data_ptr(), L.data_ptr(), *dims, FA2_DTYPE_BF16, *tail)
        check(st, "fa2_forward_decode_paged")
    return O, L


def extend_num_splits(B, H, H_kv, q_len, kv_capacity, head_dim, *, window_left=None):
    """The split count n_splits=0 stands for in the extend calls (fa2_extend_num_splits): host arithmetic, never on a length.  With
    M = (H / H_kv) q_len <= 32 it is decode_num_splits(B, H_kv, kv_capacity, head_dim, q_len=q_len, window_left=window_left); above, the
    same rule with B H_kv ceil(M / 64) workgroups to fill the GPU -- a prefill chunk resolves to one split."""
    w = _window_arg(window_left, True)
    return _capi.lib().fa2_extend_num_splits(B, H, H_kv, q_len, kv_capacity, head_dim, -1 if w is None else w)


def extend_workspace(B, H, H_kv, N_q, kv_capacity, d, n_splits=0, device="cuda", *, window_left=None):
    """Scratch for flash_attention_2_extend / _paged (the splits' fp32 partials; empty for one split): allocate once, pass as
    workspace= (graph capture).  n_splits=0 is extend_num_splits(B, H, H_kv, N_q, kv_capacity, d, window_left=window_left)."""
    w = _window_arg(window_left, True)
    return torch.empty(_decode_need(_capi.lib(), B, H, H_kv, N_q, kv_capacity, d, n_splits, w, True), dtype=torch.uint8, device=device)


def flash_attention_2_extend(Q, K_cache, V_cache, seqlens_k=None, softmax_scale=None, causal=True, sink=None, n_splits=0,
                             O=None, L=None, workspace=None, stream=None, k_descale=None, v_descale=None, window_left=None):
    """O, L = flash_attention_2_decode for ANY number of query rows per K/V head (fa2_forward_extend, include/fa2_extend_mi355x.h):
    extend attention -- speculative-decoding verification, MQA and wide groups at N_q = 1, a prefill chunk or a prefix-cache hit
    against a cache that is bf16 or e4m3.  Every argument, check and promise is flash_attention_2_decode's (seqlens_k, block of
    the sequence's LAST N_q tokens already in the cache, bottom-right causal mask, sink, descales, window_left, rows without a key,
    garbage past a length and before the window, graph capture, (O, L) for merge_states_forward); only (H / H_kv) N_q <= 32 is
    gone.  With at most 32 rows per K/V head the call IS flash_attention_2_decode, bit for bit; above, a workgroup takes 64 rows
    of a K/V head's [H / H_kv][N_q] slab and a row's result is bit for bit what flash_attention_2_decode gives for it on a slice
    of at most 32 rows with the same n_splits.  n_splits=0 is extend_num_splits(...), the workspace extend_workspace(...).
    On a contiguous bf16 cache with equal lengths flash_attention_2_qk_forward computes the same; measured (profiles/extend_times.json,
    d = 128) it takes 1.35 - 1.41 times this call's time at N_q = 512 and 8 - 40 times at N_q 8 and 1: no measured N_q favours it.
    INFERENCE ONLY.  A q_len per sequence and token-major Q / O: flash_attention_2_extend_ragged.  Not covered: tree masks."""
    return _decode_call(Q, K_cache, V_cache, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace, stream, k_descale,
                        v_descale, window_left, True)


def flash_attention_2_extend_paged(Q, K_pages, V_pages, block_table, seqlens_k=None, softmax_scale=None, causal=True, sink=None,
                                   n_splits=0, O=None, L=None, workspace=None, stream=None, k_descale=None, v_descale=None,
                                   window_left=None):
    """flash_attention_2_extend over a pool of pages (fa2_forward_extend_paged): flash_attention_2_decode_paged's arguments, checks
    and promises (block table read on the device, entries past a length and behind the window never read, the clamp of an entry
    in use, shared pages) without the row limit; with the same n_splits bit for bit flash_attention_2_extend on the gathered cache."""
    return _decode_paged_call(Q, K_pages, V_pages, block_table, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace,
                              stream, k_descale, v_descale, window_left, True)


class ExtendRaggedPlan:
    """What extend_ragged_plan returns and the ragged extend calls take: the device buffer the plan kernel filled (`tensor`,
    int32) and the (B, H_q, H_kv, total_q) it was built for.  It depends on cu_seqlens_q and H_q / H_kv only: build it once per
    step, pass it to every layer's call."""
    __slots__ = ("tensor", "B", "H_q", "H_kv", "total_q")

    def __init__(self, tensor, B, H_q, H_kv, total_q):
        self.tensor, self.B, self.H_q, self.H_kv, self.total_q = tensor, B, H_q, H_kv, total_q


def _ragged_dims(H_q, H_kv, total_q):
    for n, v in (("H_q", H_q), ("H_kv", H_kv), ("total_q", total_q)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{n}: {v!r}, expected an int >= 1")
    if H_q % H_kv:
        raise ValueError(f"H_kv: {H_kv} does not divide H_q = {H_q}")
    if total_q * H_q > 0x7fffffff - 64:
        raise ValueError(f"total_q: {total_q} tokens x {H_q} heads is more rows than an int indexes")


def _cu_seqlens_q_arg(cu):
    """cu_seqlens_q of a ragged extend step: like seqlens_k it is read ON THE DEVICE (by the plan kernel), never by the host.
    Returns B."""
    if not isinstance(cu, torch.Tensor):
        raise ValueError(f"cu_seqlens_q must be an int32 device tensor of B + 1 offsets (or an ExtendRaggedPlan), got {type(cu).__name__}: "
                         "the plan kernel reads it on the device, the host never does")
    if cu.dtype != torch.int32:
        raise ValueError(f"cu_seqlens_q: dtype {cu.dtype}, expected torch.int32")
    if cu.dim() != 1 or cu.numel() < 2:
        raise ValueError(f"cu_seqlens_q: shape {tuple(cu.shape)}, expected (B + 1,) with B >= 1")
    if not cu.is_contiguous():
        raise ValueError(f"cu_seqlens_q must be contiguous (got stride {tuple(cu.stride())}; call .contiguous())")
    if not cu.is_cuda:
        raise ValueError("cu_seqlens_q is a CPU tensor: the plan kernel reads it on the device (the host never reads it)")
    return cu.numel() - 1


def extend_ragged_plan(cu_seqlens_q, H_q, H_kv, total_q, plan=None, stream=None):
    """The plan of a ragged extend step (fa2_extend_ragged_plan, include/fa2_extend_ragged_mi355x.h): ONE small launch that turns
    cu_seqlens_q (int32 [B + 1] DEVICE tensor: sequence b owns tokens cu[b] .. cu[b + 1] - 1 of the total_q packed ones, q_b = 0
    allowed) into the sanitised (start_b, q_b) and the list of 64-row work items the attention kernels read.  It depends on
    cu_seqlens_q and H_q / H_kv only: every layer of the step reuses it.  The host never reads cu_seqlens_q; a tensor that is not
    non-decreasing within [0, total_q] is the caller's error with a defined outcome (the running maximum, clamped).
    plan: None (a buffer is allocated), a device tensor of at least fa2_extend_ragged_plan_bytes bytes, 16-byte aligned, or an
    ExtendRaggedPlan to refill in place -- PASS ONE FOR GRAPH CAPTURE and rewrite cu_seqlens_q in place between replays.
    Returns an ExtendRaggedPlan."""
    _ragged_dims(H_q, H_kv, total_q)
    B = _cu_seqlens_q_arg(cu_seqlens_q)
    lib = _capi.lib()
    need = lib.fa2_extend_ragged_plan_bytes(B, H_q, H_kv, total_q)
    if not need:
        raise ValueError(f"extend_ragged_plan: no plan for B = {B}, H_q = {H_q}, H_kv = {H_kv}, total_q = {total_q}")
    if isinstance(plan, ExtendRaggedPlan):
        if (plan.B, plan.H_q // plan.H_kv, plan.total_q) != (B, H_q // H_kv, total_q):
            raise ValueError(f"plan: built for B = {plan.B}, H_q / H_kv = {plan.H_q // plan.H_kv}, total_q = {plan.total_q}; "
                             f"this step has B = {B}, H_q / H_kv = {H_q // H_kv}, total_q = {total_q}")
        buf = plan.tensor
    elif plan is None:
        buf = torch.empty(need // 4, dtype=torch.int32, device=cu_seqlens_q.device)
    else:
        buf = plan
    if not isinstance(buf, torch.Tensor) or not buf.is_cuda or not buf.is_contiguous() or buf.device != cu_seqlens_q.device:
        raise ValueError("plan must be a contiguous device tensor on cu_seqlens_q's device")
    if _nbytes(buf) < need or buf.data_ptr() % 16:
        raise ValueError(f"plan: {_nbytes(buf)} bytes at an address % 16 = {buf.data_ptr() % 16}, {need} needed, 16-byte aligned")
    st = lib.fa2_extend_ragged_plan(cu_seqlens_q.data_ptr(), B, H_q, H_kv, total_q, buf.data_ptr(), _nbytes(buf), _stream_ptr(stream))
    check(st, "fa2_extend_ragged_plan")
    return ExtendRaggedPlan(buf, B, H_q, H_kv, total_q)


def extend_ragged_num_splits(B, H, H_kv, total_q, kv_capacity, head_dim, *, window_left=None):
    """The split count n_splits=0 stands for in the ragged extend calls (fa2_extend_ragged_num_splits): host arithmetic on B,
    total_q and the capacity, never on a q_b or a length: min(ceil(256 / workgroups), max(1, span / 256), 256) with
    workgroups = H_kv max(min(B, total_q), ceil((H / H_kv) total_q / 64))."""
    w = _window_arg(window_left, True)
    return _capi.lib().fa2_extend_ragged_num_splits(B, H, H_kv, total_q, kv_capacity, head_dim, -1 if w is None else w)


def extend_ragged_workspace(B, H, H_kv, total_q, kv_capacity, d, n_splits=0, device="cuda", *, window_left=None):
    """Scratch for flash_attention_2_extend_ragged / _paged (the splits' fp32 partials; empty for one split): allocate once, pass
    as workspace= (graph capture).  n_splits=0 is extend_ragged_num_splits(...)."""
    w = _window_arg(window_left, True)
    need = _capi.lib().fa2_extend_ragged_workspace_bytes(B, H, H_kv, total_q, kv_capacity, d, n_splits, -1 if w is None else w)
    return torch.empty(need, dtype=torch.uint8, device=device)


def _extend_ragged_call(Q, K, V, block_table, cu_or_plan, seqlens_k, softmax_scale, causal, sink, n_splits, O, L, workspace, stream,
                        k_descale, v_descale, window_left):
    """flash_attention_2_extend_ragged (block_table None) and _paged: one set of checks for both, the siblings' in their order."""
    paged = block_table is not None
    kname, vname = ("K_pages", "V_pages") if paged else ("K_cache", "V_cache")
    want = "[n_pages, H_kv, page_size, d]" if paged else "[B, H_kv, N_cap, d]"
    if not isinstance(Q, torch.Tensor) or Q.dim() != 3:
        raise ValueError(f"Q: expected a 3-d tensor [T, H_q, d] (token-major), got {tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__}")
    for n, t in ((kname, K), (vname, V)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor {want}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    T, H, d = Q.shape
    n0, Hkv, n2, dk = K.shape
    if dk != d or Hkv < 1 or H % Hkv != 0 or T < 1 or n0 < 1 or n2 < 1:
        raise ValueError(f"{kname}: shape {tuple(K.shape)} does not match Q {tuple(Q.shape)}: expected {want} with d = {d} and H_kv dividing H_q = {H}")
    if tuple(V.shape) != tuple(K.shape):
        raise ValueError(f"{vname}: shape {tuple(V.shape)} does not match {kname} {tuple(K.shape)}")
    if paged and n2 % DECODE_PAGE_GRAIN:
        raise ValueError(f"K_pages: page_size {n2} is not a multiple of {DECODE_PAGE_GRAIN} (the kernel's key tile)")
    if Q.dtype != torch.bfloat16:
        raise ValueError(f"Q: dtype {Q.dtype}, expected torch.bfloat16")
    fp8 = _kv_dtypes(Q, K, V, kname, vname)
    if d not in (64, 128):
        raise ValueError(f"Q: head_dim {d}, expected 64 or 128")
    if Q.stride(2) != 1 or Q.stride(1) != d:
        raise ValueError(f"Q: strides {tuple(Q.stride())}, the last two dimensions must be contiguous ([T, H_q, d] with strides (s, d, 1))")
    if T > 1 and (Q.stride(0) < H * d or Q.stride(0) % 8):
        raise ValueError(f"Q: token stride {Q.stride(0)}, expected at least H_q x d = {H * d} and a multiple of 8 elements (a lane loads 16 bytes)")
    if Q.storage_offset() % 8:
        raise ValueError(f"Q: storage offset {Q.storage_offset()} elements is not 16-byte aligned (a multiple of 8): a lane loads 16 bytes")
    q_stride = Q.stride(0) if T > 1 else H * d
    if isinstance(n_splits, bool) or not isinstance(n_splits, int) or not 0 <= n_splits <= DECODE_MAX_SPLITS:
        raise ValueError(f"n_splits: {n_splits!r}, expected an int in 1..{DECODE_MAX_SPLITS}, or 0 for the default")
    window_left = _window_arg(window_left, causal)
    if isinstance(cu_or_plan, ExtendRaggedPlan):
        plan = cu_or_plan
        if (plan.H_q // plan.H_kv, plan.total_q) != (H // Hkv, T):
            raise ValueError(f"plan: built for H_q / H_kv = {plan.H_q // plan.H_kv} and total_q = {plan.total_q}; Q {tuple(Q.shape)} against "
                             f"{Hkv} K/V heads has H_q / H_kv = {H // Hkv} and total_q = {T}")
        B = plan.B
    else:
        plan = None
        B = _cu_seqlens_q_arg(cu_or_plan)
    if paged:
        Q4 = Q.new_empty((B, H, 0, d))      # (the shared helpers describe their tensors beside a [B, H, N, d] Q)
        for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
            if t is not None:
                _descale_arg(t, Q4, Hkv, name, fp8, kname)
        max_pages = _block_table_arg(block_table, Q4, B)
        kv_capacity = max_pages * n2
        if kv_capacity > 0x7fffffff - (DECODE_MAX_SPLITS + 2) * 128:
            raise ValueError(f"block_table: {max_pages} pages of {n2} keys is a capacity of {kv_capacity} keys, above what an int indexes")
    else:
        Q4 = Q.new_empty((B, H, 0, d))
        if n0 != B:
            raise ValueError(f"K_cache: {n0} sequences, cu_seqlens_q (the plan) has {B}")
        kv_capacity = n2
    if seqlens_k is not None:
        _seqlens_arg(seqlens_k, Q4, B)
    if sink is not None:
        _sink_arg(sink, Q4, 1)
    if not paged:
        for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
            if t is not None:
                _descale_arg(t, Q4, Hkv, name, fp8, kname)
    if not Q.is_cuda:
        raise ValueError("Q must be a device tensor")
    _like(K, kname, Q, tuple(K.shape), K.dtype)
    _like(V, vname, Q, tuple(K.shape), K.dtype)
    scale = _scale(softmax_scale, d)
    if not scale > 0.0:
        raise ValueError(f"softmax_scale: {scale}, expected a positive number")
    if plan is None:
        if cu_or_plan.device != Q.device:
            raise ValueError(f"cu_seqlens_q is on {cu_or_plan.device}, expected {Q.device}")
        plan = extend_ragged_plan(cu_or_plan, H, Hkv, T, stream=stream)
    elif plan.tensor.device != Q.device:
        raise ValueError(f"plan is on {plan.tensor.device}, expected {Q.device}")
    if O is None:
        O = torch.empty(T, H, d, dtype=Q.dtype, device=Q.device)
    elif not isinstance(O, torch.Tensor) or tuple(O.shape) != (T, H, d) or O.dtype != Q.dtype or not O.is_contiguous() or O.device != Q.device:
        raise ValueError(f"O: expected a contiguous {Q.dtype} tensor {(T, H, d)} on {Q.device}")
    L = torch.empty(T, H, dtype=torch.float32, device=Q.device) if L is None else _rows(L, "L", Q, T, H, 1)
    lib = _capi.lib()
    need = lib.fa2_extend_ragged_workspace_bytes(B, H, Hkv, T, kv_capacity, d, n_splits, -1 if window_left is None else window_left)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=Q.device)
    if workspace is not None and _nbytes(_workspace_arg(workspace, Q)) < need:
        raise ValueError(f"workspace: {_nbytes(workspace)} bytes, {need} needed (extend_ragged_workspace)")
    mid = (plan.tensor.data_ptr(), _nbytes(plan.tensor), _ptr(seqlens_k), _ptr(sink), _ptr(k_descale), _ptr(v_descale), O.data_ptr(), L.data_ptr())
    tail = (d, scale, FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, 1 if causal else 0, n_splits, _ptr(workspace),
            0 if workspace is None else _nbytes(workspace), _stream_ptr(stream), -1 if window_left is None else window_left)
    if paged:
        st = lib.fa2_forward_extend_ragged_paged(Q.data_ptr(), q_stride, K.data_ptr(), V.data_ptr(), block_table.data_ptr(), *mid,
                                                 B, H, Hkv, T, n0, n2, max_pages, *tail)
        check(st, "fa2_forward_extend_ragged_paged")
    else:
        st = lib.fa2_forward_extend_ragged(Q.data_ptr(), q_stride, K.data_ptr(), V.data_ptr(), *mid, B, H, Hkv, T, kv_capacity, *tail)
        check(st, "fa2_forward_extend_ragged")
    return O, L


def flash_attention_2_extend_ragged(Q, K_cache, V_cache, cu_seqlens_q_or_plan, seqlens_k=None, softmax_scale=None, causal=True,
                                    sink=None, n_splits=0, O=None, L=None, workspace=None, stream=None, k_descale=None,
                                    v_descale=None, window_left=None):
    """O, L = flash_attention_2_extend with a q_len PER SEQUENCE and TOKEN-MAJOR rows (fa2_forward_extend_ragged,
    include/fa2_extend_ragged_mi355x.h): one call for a continuous-batching step that mixes prompt chunks, speculative
    verification and plain decodes.  Q: bf16 [T, H_q, d], any view with contiguous last two dimensions and a token stride that is
    a multiple of 8 (the Q slice of a fused QKV output goes in as it is); K_cache, V_cache [B, H_kv, N_cap, d], bf16 or e4m3;
    returns O [T, H_q, d] and L [T, H_q] -- flattened, the rows merge_states_forward takes.
    cu_seqlens_q_or_plan: an int32 [B + 1] DEVICE tensor (sequence b owns tokens cu[b] .. cu[b + 1] - 1, q_b = cu[b + 1] - cu[b],
    0 allowed; the plan is then built inside this call, one more small launch), or the ExtendRaggedPlan extend_ragged_plan
    built from it -- once per step, shared by every layer.  The host never reads cu_seqlens_q.  Everything
    flash_attention_2_extend defines with N_q holds with q_b: the q_b queries are the sequence's last q_b cached tokens, key j is
    visible to token i iff j <= i + len_b - q_b, window_left counts from pos_i = i + len_b - q_b, rows with pos_i < 0 have O = 0
    and L = -inf (or the sink).  Tokens of no sequence keep what O and L held.  seqlens_k, sink, descales, window_left,
    n_splits (0 = extend_ragged_num_splits), workspace (extend_ragged_workspace), graph capture: flash_attention_2_extend's.  With
    the same n_splits a sequence's rows are bit for bit flash_attention_2_extend's on that sequence alone.  INFERENCE ONLY.
    The step's ragged append is rope_kv_cache_append_ragged (the same plan).  Not covered: tree masks, token-major pools."""
    return _extend_ragged_call(Q, K_cache, V_cache, None, cu_seqlens_q_or_plan, seqlens_k, softmax_scale, causal, sink, n_splits, O, L,
                               workspace, stream, k_descale, v_descale, window_left)


def flash_attention_2_extend_ragged_paged(Q, K_pages, V_pages, block_table, cu_seqlens_q_or_plan, seqlens_k=None, softmax_scale=None,
                                          causal=True, sink=None, n_splits=0, O=None, L=None, workspace=None, stream=None,
                                          k_descale=None, v_descale=None, window_left=None):
    """flash_attention_2_extend_ragged over a pool of pages (fa2_forward_extend_ragged_paged): K_pages, V_pages [n_pages, H_kv,
    page_size, d] and block_table int32 [B, max_pages] as flash_attention_2_extend_paged takes them (read on the device, entries
    past a length and behind the window never read, an entry in use clamped, shared pages); with the same n_splits bit for bit
    flash_attention_2_extend_ragged on the gathered cache."""
    if block_table is None:
        raise ValueError("block_table must be an int32 device tensor [B, max_pages]")
    return _extend_ragged_call(Q, K_pages, V_pages, block_table, cu_seqlens_q_or_plan, seqlens_k, softmax_scale, causal, sink, n_splits,
                               O, L, workspace, stream, k_descale, v_descale, window_left)


def _kv_new_arg(K_new, V_new):
    """(B, H_kv, n_new, d, (stride_b, stride_h, stride_t)) of an append's source: bf16 [B, H_kv, n_new, d] VIEWS with the last
    dimension contiguous and one stride triple for both, each a non-negative multiple of 8 elements, 16-byte aligned -- a lane
    loads 16 bytes.  No copy is made: a token-major tensor or a slice of a fused QKV output is passed permuted."""
    how = ("pass [B, H_kv, n_new, d] views, e.g. x.permute(0, 2, 1, 3) of a token-major [B, n_new, H_kv, d] tensor or the K and V "
           "slices of one fused QKV output")
    for n, t in (("K_new", K_new), ("V_new", V_new)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor [B, H_kv, n_new, d], got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}; {how}")
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{n}: dtype {t.dtype}, expected torch.bfloat16 (the source of an append is bf16; the cache may be e4m3)")
    B, Hkv, n_new, d = K_new.shape
    if min(B, Hkv, n_new) < 1:
        raise ValueError(f"K_new: shape {tuple(K_new.shape)}, expected [B, H_kv, n_new, d] with B, H_kv, n_new >= 1")
    if tuple(V_new.shape) != tuple(K_new.shape):
        raise ValueError(f"V_new: shape {tuple(V_new.shape)} does not match K_new {tuple(K_new.shape)}")
    if d not in (64, 128):
        raise ValueError(f"K_new: head_dim {d}, expected 64 or 128")
    for n, t in (("K_new", K_new), ("V_new", V_new)):
        if t.stride(-1) != 1:
            raise ValueError(f"{n}: stride {tuple(t.stride())}, the last dimension must be contiguous (stride(-1) == 1); {how}")
    if tuple(V_new.stride()) != tuple(K_new.stride()):
        raise ValueError(f"V_new: strides {tuple(V_new.stride())} differ from K_new's {tuple(K_new.stride())}: one (batch, head, token) "
                         f"stride triple serves both; {how}")
    strides = tuple(K_new.stride()[:3])
    if any(s < 0 or s % 8 for s in strides):
        raise ValueError(f"K_new: strides {strides} (batch, head, token) must be non-negative multiples of 8 elements: a lane loads 16 bytes")
    for n, t in (("K_new", K_new), ("V_new", V_new)):
        if t.storage_offset() % 8:
            raise ValueError(f"{n}: storage offset {t.storage_offset()} elements is not 16-byte aligned (a multiple of 8): a lane loads 16 bytes")
    return B, Hkv, n_new, d, strides


def _kv_append_dtypes(K_new, K, V, kname, vname, Hkv, k_descale, v_descale):
    """The caches' dtypes beside an append's source (returns fp8) and the descales that belong to them."""
    fp8 = _kv_dtypes(K_new, K, V, kname, vname)
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if t is not None:
            _descale_arg(t, K_new, Hkv, name, fp8, kname)
    return fp8


def _kv_append_devices(K_new, V_new, K, V, kname, vname, shape):
    """Last, like every wrapper here: the source on a device, the caches contiguous on that device (_like)."""
    for n, t in (("K_new", K_new), ("V_new", V_new)):
        if not t.is_cuda:
            raise ValueError(f"{n} must be a device tensor")
    if V_new.device != K_new.device:
        raise ValueError(f"V_new is on {V_new.device}, expected {K_new.device}")
    _like(K, kname, K_new, shape, K.dtype)
    _like(V, vname, K_new, shape, K.dtype)


def kv_cache_append(K_new, V_new, K_cache, V_cache, seqlens_k, k_descale=None, v_descale=None, stream=None):
    """Append the n_new newest tokens' K and V of every sequence to the caches flash_attention_2_decode reads (fa2_kv_append), IN
    PLACE, in one launch; returns None.  K_new, V_new: bf16 [B, H_kv, n_new, d] VIEWS (d = 64 | 128) with stride(-1) == 1 and equal
    strides, non-negative multiples of 8 elements: a token-major [B, n_new, H_kv, d] tensor permuted, or the K and V slices of a
    fused QKV projection output -- no .contiguous() copy.  K_cache, V_cache: [B, H_kv, N_cap, d] contiguous, both bf16 (the source
    bits are copied) or both torch.float8_e4m3fn: head h then stores (x.float() / descale[h]).clamp(-448, 448).to(float8_e4m3fn),
    byte for byte (saturating: inf -> +-448, NaN -> a NaN code), k_descale / v_descale fp32 [H_kv] DEVICE tensors or None (= 1), the
    decode call's.
    seqlens_k: int32 [B] DEVICE tensor, required, the lengths AFTER the append -- the tensor the decode call of the same step
    reads.  A step is: seqlens_k += n_new (in place), kv_cache_append, flash_attention_2_decode; one captured graph serves every
    step.  Token t of sequence b goes to row seqlens_k[b] - n_new + t and is written iff that row is in [0, N_cap); every other
    token is dropped, nothing is clamped into range.  The host never reads seqlens_k or a descale, nothing is allocated.
    A source that overlaps the cache is undefined."""
    B, Hkv, n_new, d, strides = _kv_new_arg(K_new, V_new)
    for n, t in (("K_cache", K_cache), ("V_cache", V_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor [B, H_kv, N_cap, d], got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    Ncap = K_cache.shape[2]
    shape = (B, Hkv, Ncap, d)
    if tuple(K_cache.shape) != shape or Ncap < 1:
        raise ValueError(f"K_cache: shape {tuple(K_cache.shape)} does not match K_new {tuple(K_new.shape)}: expected [{B}, {Hkv}, N_cap, {d}]")
    if tuple(V_cache.shape) != shape:
        raise ValueError(f"V_cache: shape {tuple(V_cache.shape)} does not match K_cache {tuple(K_cache.shape)}")
    fp8 = _kv_append_dtypes(K_new, K_cache, V_cache, "K_cache", "V_cache", Hkv, k_descale, v_descale)
    if seqlens_k is None:
        raise ValueError("seqlens_k is required: an append writes token t of sequence b at row seqlens_k[b] - n_new + t (the lengths "
                         "AFTER the append, the decode call's tensor); 'all of the capacity' has no meaning for a write")
    _seqlens_arg(seqlens_k, K_new, B)
    _kv_append_devices(K_new, V_new, K_cache, V_cache, "K_cache", "V_cache", shape)
    st = _capi.lib().fa2_kv_append(K_new.data_ptr(), V_new.data_ptr(), K_cache.data_ptr(), V_cache.data_ptr(), seqlens_k.data_ptr(),
                                   _ptr(k_descale), _ptr(v_descale), B, Hkv, n_new, Ncap, d, *strides, FA2_DTYPE_BF16,
                                   FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, _stream_ptr(stream))
    check(st, "fa2_kv_append")


def kv_cache_append_paged(K_new, V_new, K_pages, V_pages, block_table, seqlens_k, k_descale=None, v_descale=None, stream=None):
    """kv_cache_append into a pool of pages (fa2_kv_append_paged), the pool flash_attention_2_decode_paged reads: K_pages, V_pages
    [n_pages, H_kv, page_size, d] contiguous, page_size a multiple of 32, bf16 or torch.float8_e4m3fn; block_table int32
    [B, max_pages] DEVICE tensor.  Row pos = seqlens_k[b] - n_new + t is row pos % page_size of page block_table[b, pos // page_size];
    it is written iff 0 <= pos < max_pages * page_size AND that table entry lies in [0, n_pages) -- a token whose entry does not is
    DROPPED (the decode clamps such an entry; a write through a clamped entry would corrupt another sequence's page) while its
    neighbours on other pages are written.  Only the table entries of written rows are read; the host reads none.
    PAGES WRITTEN BY ONE CALL MUST BELONG TO ONE SEQUENCE EACH: shared prefix pages are read-only to an append, and allocating
    pages (assign the entry before the step that grows into it) and copy-on-write stay the allocator's.  Everything else is
    kv_cache_append's: the source views, the values, the descales, seqlens_k (required, the lengths after the append), in place,
    one launch, returns None."""
    B, Hkv, n_new, d, strides = _kv_new_arg(K_new, V_new)
    for n, t in (("K_pages", K_pages), ("V_pages", V_pages)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor [n_pages, H_kv, page_size, d], got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    n_pages, hk, page_size, dk = K_pages.shape
    if hk != Hkv or dk != d or n_pages < 1 or page_size < 1:
        raise ValueError(f"K_pages: shape {tuple(K_pages.shape)} does not match K_new {tuple(K_new.shape)}: expected "
                         f"[n_pages, {Hkv}, page_size, {d}] with n_pages, page_size >= 1")
    if page_size % DECODE_PAGE_GRAIN:
        raise ValueError(f"K_pages: page_size {page_size} is not a multiple of {DECODE_PAGE_GRAIN} (the decode kernel's key tile; a page "
                         "of 16 keys is not taken)")
    shape = (n_pages, Hkv, page_size, d)
    if tuple(V_pages.shape) != shape:
        raise ValueError(f"V_pages: shape {tuple(V_pages.shape)} does not match K_pages {tuple(K_pages.shape)}")
    fp8 = _kv_append_dtypes(K_new, K_pages, V_pages, "K_pages", "V_pages", Hkv, k_descale, v_descale)
    if seqlens_k is None:
        raise ValueError("seqlens_k is required: an append writes token t of sequence b at row seqlens_k[b] - n_new + t (the lengths "
                         "AFTER the append, the decode call's tensor); 'all of the capacity' has no meaning for a write")
    max_pages = _block_table_arg(block_table, K_new, B)
    if max_pages * page_size > 0x7fffffff - (DECODE_MAX_SPLITS + 2) * 128:
        raise ValueError(f"block_table: {max_pages} pages of {page_size} keys is a capacity of {max_pages * page_size} keys, above what an int indexes")
    _seqlens_arg(seqlens_k, K_new, B)
    _kv_append_devices(K_new, V_new, K_pages, V_pages, "K_pages", "V_pages", shape)
    st = _capi.lib().fa2_kv_append_paged(K_new.data_ptr(), V_new.data_ptr(), K_pages.data_ptr(), V_pages.data_ptr(),
                                         block_table.data_ptr(), seqlens_k.data_ptr(), _ptr(k_descale), _ptr(v_descale),
                                         B, Hkv, n_new, n_pages, page_size, max_pages, d, *strides, FA2_DTYPE_BF16,
                                         FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, _stream_ptr(stream))
    check(st, "fa2_kv_append_paged")


def _rope_q_arg(Q, K_new):
    """(H_q, (stride_b, stride_h, stride_t)) of the step's queries beside K_new: a bf16 [B, H_q, n_new, d] VIEW with strides of its
    own, under the rules of K_new (_kv_new_arg); None is a K/V-only call (H_q = 0)."""
    if Q is None:
        return 0, (0, 0, 0)
    B, _, n_new, d = K_new.shape
    how = ("pass a [B, H_q, n_new, d] view, e.g. x.permute(0, 2, 1, 3) of a token-major [B, n_new, H_q, d] tensor or the Q slice of the "
           "fused QKV output")
    if not isinstance(Q, torch.Tensor) or Q.dim() != 4:
        raise ValueError(f"Q: expected a 4-d tensor [B, H_q, n_new, d], got {tuple(Q.shape) if isinstance(Q, torch.Tensor) else type(Q).__name__}; {how}")
    if Q.dtype != torch.bfloat16:
        raise ValueError(f"Q: dtype {Q.dtype}, expected torch.bfloat16")
    if Q.shape[0] != B or Q.shape[1] < 1 or Q.shape[2] != n_new or Q.shape[3] != d:
        raise ValueError(f"Q: shape {tuple(Q.shape)} does not match K_new {tuple(K_new.shape)}: expected [{B}, H_q, {n_new}, {d}] with H_q >= 1")
    if Q.stride(-1) != 1:
        raise ValueError(f"Q: stride {tuple(Q.stride())}, the last dimension must be contiguous (stride(-1) == 1); {how}")
    strides = tuple(Q.stride()[:3])
    if any(s < 0 or s % 8 for s in strides):
        raise ValueError(f"Q: strides {strides} (batch, head, token) must be non-negative multiples of 8 elements: a lane loads 16 bytes")
    if Q.storage_offset() % 8:
        raise ValueError(f"Q: storage offset {Q.storage_offset()} elements is not 16-byte aligned (a multiple of 8): a lane loads 16 bytes")
    return Q.shape[1], strides


def _rope_tables_arg(cos, sin, d, capacity):
    """(rot_dim, n_positions) of the cos/sin tables: fp32 [n_positions, rot_dim / 2], one shape for both, rot_dim a multiple of 16 in
    [16, d], a row for every row of the cache.  Device and contiguity are checked last (_rope_devices)."""
    for n, t in (("cos", cos), ("sin", sin)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{n}: expected a 2-d tensor [n_positions, rot_dim / 2], got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"{n}: dtype {t.dtype}, expected torch.float32 (the rotation is fp32 arithmetic on fp32 tables)")
    n_positions, half = cos.shape
    if tuple(sin.shape) != tuple(cos.shape):
        raise ValueError(f"sin: shape {tuple(sin.shape)} does not match cos {tuple(cos.shape)}")
    if half < 8 or half % 8 or 2 * half > d:
        raise ValueError(f"cos: shape {tuple(cos.shape)} is a rot_dim of {2 * half}, expected a multiple of 16 in [16, {d}] (head_dim)")
    if n_positions < capacity:
        raise ValueError(f"cos: {n_positions} positions for a cache of {capacity} rows: a token's position is its cache row, so the "
                         "tables need a row for every row of the cache")
    return 2 * half, n_positions


def _rope_devices(Q, Q_out, cos, sin, K_new, B, Hq, n_new, d):
    """Last: the tables contiguous on the source's device, Q there too, Q_out (allocated here when not given: the only
    allocation) dense [B, H_q, n_new, d] there."""
    if Q is not None and not Q.is_cuda:
        raise ValueError("Q must be a device tensor")
    if Q is not None and Q.device != K_new.device:
        raise ValueError(f"Q is on {Q.device}, expected {K_new.device}")
    for n, t in (("cos", cos), ("sin", sin)):
        if not t.is_cuda:
            raise ValueError(f"{n} must be a device tensor: the kernel reads the tables on the device when it runs")
        if t.device != K_new.device:
            raise ValueError(f"{n} is on {t.device}, expected {K_new.device}")
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous (got stride {tuple(t.stride())}; call .contiguous())")
        if t.data_ptr() % 16:
            raise ValueError(f"{n}: not 16-byte aligned (storage offset {t.storage_offset()} elements): a lane loads 16 bytes")
    if Q is None:
        if Q_out is not None:
            raise ValueError("Q_out: given without Q (a K/V-only call has neither)")
        return None
    if Q_out is None:
        return torch.empty(B, Hq, n_new, d, dtype=torch.bfloat16, device=K_new.device)
    return _like(Q_out, "Q_out", K_new, (B, Hq, n_new, d), torch.bfloat16)


def _rope_interleaved(interleaved):
    if not isinstance(interleaved, bool):
        raise ValueError(f"interleaved: {interleaved!r}, expected a bool (False: rotate-half pairs (i, i + rot_dim/2); True: pairs (2i, 2i+1))")
    return 1 if interleaved else 0


def rope_kv_cache_append(Q, K_new, V_new, K_cache, V_cache, cos, sin, seqlens_k, *, interleaved=False, k_descale=None,
                         v_descale=None, Q_out=None, stream=None):
    """kv_cache_append with rotary position embedding (RoPE) in front, and the step's queries beside it (fa2_rope_kv_append): ONE
    launch rotates the n_new newest tokens' K and writes it into K_cache, copies their V into V_cache -- both exactly as
    kv_cache_append stores them, bf16 or torch.float8_e4m3fn with descales -- and writes the rotated queries; returns Q_out,
    bf16 [B, H_q, n_new, d] contiguous, what flash_attention_2_decode takes.  A step is: seqlens_k += n_new (in place),
    rope_kv_cache_append, flash_attention_2_decode(Q_out, ...); one captured graph serves every step.
    Q, K_new, V_new: bf16 [B, H, n_new, d] VIEWS (d = 64 | 128) as kv_cache_append describes them; Q has strides of its own, so the
    three slices of a fused QKV projection output are passed as they are -- no .contiguous() copy.  Q=None is a K/V-only call
    (returns None).
    POSITION: token t of sequence b has position seqlens_k[b] - n_new + t -- its cache row, the position the decode's mask gives
    query t, and the row of the tables.  cos, sin: fp32 [n_positions, rot_dim / 2] contiguous DEVICE tensors the caller builds (any
    frequency scaling is the caller's), n_positions >= the cache's capacity, rot_dim a multiple of 16 in [16, d]; elements past
    rot_dim pass through (partial rotary).  interleaved=False: rotate-half (NeoX, HF) pairs (i, i + rot_dim/2); True: GPT-J pairs
    (2i, 2i + 1); both use table column i.
    ARITHMETIC: byte for byte (x1.float()*c - x2.float()*s).bfloat16() and (x2.float()*c + x1.float()*s).bfloat16(), every product
    and sum one fp32 rounding (no fused multiply-add).  HF's all-bf16 arithmetic is a different, less exact expression and is not
    reproduced.  An e4m3 cache stores the quantised ROUNDED bf16 value, so the call is byte for byte {rotate in torch to bf16,
    kv_cache_append}.
    Q_out: EVERY row is written: rotated where 0 <= position < capacity, +0.0 throughout elsewhere (such a token's K and V are
    dropped, as kv_cache_append drops them).  Allocated when not given -- the ONLY allocation; pass one for graph capture.  The host
    never reads seqlens_k, a descale or a table.  Q_out overlapping an input is undefined."""
    B, Hkv, n_new, d, strides = _kv_new_arg(K_new, V_new)
    Hq, q_strides = _rope_q_arg(Q, K_new)
    for n, t in (("K_cache", K_cache), ("V_cache", V_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor [B, H_kv, N_cap, d], got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    Ncap = K_cache.shape[2]
    shape = (B, Hkv, Ncap, d)
    if tuple(K_cache.shape) != shape or Ncap < 1:
        raise ValueError(f"K_cache: shape {tuple(K_cache.shape)} does not match K_new {tuple(K_new.shape)}: expected [{B}, {Hkv}, N_cap, {d}]")
    if tuple(V_cache.shape) != shape:
        raise ValueError(f"V_cache: shape {tuple(V_cache.shape)} does not match K_cache {tuple(K_cache.shape)}")
    fp8 = _kv_append_dtypes(K_new, K_cache, V_cache, "K_cache", "V_cache", Hkv, k_descale, v_descale)
    rot_dim, n_positions = _rope_tables_arg(cos, sin, d, Ncap)
    flag = _rope_interleaved(interleaved)
    if seqlens_k is None:
        raise ValueError("seqlens_k is required: token t of sequence b has position seqlens_k[b] - n_new + t (the lengths AFTER the "
                         "append, the decode call's tensor)")
    _seqlens_arg(seqlens_k, K_new, B)
    _kv_append_devices(K_new, V_new, K_cache, V_cache, "K_cache", "V_cache", shape)
    Q_out = _rope_devices(Q, Q_out, cos, sin, K_new, B, Hq, n_new, d)
    st = _capi.lib().fa2_rope_kv_append(_ptr(Q), _ptr(Q_out), K_new.data_ptr(), V_new.data_ptr(), K_cache.data_ptr(), V_cache.data_ptr(),
                                        cos.data_ptr(), sin.data_ptr(), seqlens_k.data_ptr(), _ptr(k_descale), _ptr(v_descale),
                                        B, Hq, Hkv, n_new, Ncap, d, rot_dim, n_positions, flag, *q_strides, *strides, FA2_DTYPE_BF16,
                                        FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, _stream_ptr(stream))
    check(st, "fa2_rope_kv_append")
    return Q_out


def rope_kv_cache_append_paged(Q, K_new, V_new, K_pages, V_pages, block_table, cos, sin, seqlens_k, *, interleaved=False,
                               k_descale=None, v_descale=None, Q_out=None, stream=None):
    """rope_kv_cache_append into a pool of pages (fa2_rope_kv_append_paged), the pool flash_attention_2_decode_paged reads: K_pages,
    V_pages [n_pages, H_kv, page_size, d] and block_table int32 [B, max_pages] exactly as kv_cache_append_paged takes them, the
    capacity max_pages * page_size (the tables need that many rows).  A token whose table entry lies outside [0, n_pages) has its
    K and V DROPPED, as there; its Q_out row is still the rotated query: Q depends on the position alone.  PAGES WRITTEN BY ONE
    CALL MUST BELONG TO ONE SEQUENCE EACH.  Everything else is rope_kv_cache_append's: the views, the tables, the pair forms, the
    arithmetic, seqlens_k (required, the lengths after the append), one launch, returns Q_out."""
    B, Hkv, n_new, d, strides = _kv_new_arg(K_new, V_new)
    Hq, q_strides = _rope_q_arg(Q, K_new)
    for n, t in (("K_pages", K_pages), ("V_pages", V_pages)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor [n_pages, H_kv, page_size, d], got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    n_pages, hk, page_size, dk = K_pages.shape
    if hk != Hkv or dk != d or n_pages < 1 or page_size < 1:
        raise ValueError(f"K_pages: shape {tuple(K_pages.shape)} does not match K_new {tuple(K_new.shape)}: expected "
                         f"[n_pages, {Hkv}, page_size, {d}] with n_pages, page_size >= 1")
    if page_size % DECODE_PAGE_GRAIN:
        raise ValueError(f"K_pages: page_size {page_size} is not a multiple of {DECODE_PAGE_GRAIN} (the decode kernel's key tile; a page "
                         "of 16 keys is not taken)")
    shape = (n_pages, Hkv, page_size, d)
    if tuple(V_pages.shape) != shape:
        raise ValueError(f"V_pages: shape {tuple(V_pages.shape)} does not match K_pages {tuple(K_pages.shape)}")
    fp8 = _kv_append_dtypes(K_new, K_pages, V_pages, "K_pages", "V_pages", Hkv, k_descale, v_descale)
    _rope_tables_arg(cos, sin, d, 0)
    flag = _rope_interleaved(interleaved)
    if seqlens_k is None:
        raise ValueError("seqlens_k is required: token t of sequence b has position seqlens_k[b] - n_new + t (the lengths AFTER the "
                         "append, the decode call's tensor)")
    max_pages = _block_table_arg(block_table, K_new, B)
    if max_pages * page_size > 0x7fffffff - (DECODE_MAX_SPLITS + 2) * 128:
        raise ValueError(f"block_table: {max_pages} pages of {page_size} keys is a capacity of {max_pages * page_size} keys, above what an int indexes")
    rot_dim, n_positions = _rope_tables_arg(cos, sin, d, max_pages * page_size)
    _seqlens_arg(seqlens_k, K_new, B)
    _kv_append_devices(K_new, V_new, K_pages, V_pages, "K_pages", "V_pages", shape)
    Q_out = _rope_devices(Q, Q_out, cos, sin, K_new, B, Hq, n_new, d)
    st = _capi.lib().fa2_rope_kv_append_paged(_ptr(Q), _ptr(Q_out), K_new.data_ptr(), V_new.data_ptr(), K_pages.data_ptr(),
                                              V_pages.data_ptr(), block_table.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                              seqlens_k.data_ptr(), _ptr(k_descale), _ptr(v_descale), B, Hq, Hkv, n_new, n_pages, page_size,
                                              max_pages, d, rot_dim, n_positions, flag, *q_strides, *strides, FA2_DTYPE_BF16,
                                              FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16, _stream_ptr(stream))
    check(st, "fa2_rope_kv_append_paged")
    return Q_out


def _ragged_rows_arg(x, name, H_name, how):
    """(H, (stride_t, stride_h)) of a token-major source of a ragged append: a bf16 [T, H, d] VIEW with the last dimension
    contiguous, strides non-negative multiples of 8 elements, 16-byte aligned -- a lane loads 16 bytes (_kv_new_arg's rules)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"{name}: expected a 3-d tensor [T, {H_name}, d] (token-major), got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}; {how}")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"{name}: dtype {x.dtype}, expected torch.bfloat16 (the source of an append is bf16; the cache may be e4m3)")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name}: shape {tuple(x.shape)}, expected [T, {H_name}, d] with T, {H_name} >= 1")
    if x.stride(-1) != 1:
        raise ValueError(f"{name}: stride {tuple(x.stride())}, the last dimension must be contiguous (stride(-1) == 1); {how}")
    strides = tuple(x.stride()[:2])
    if any(s < 0 or s % 8 for s in strides):
        raise ValueError(f"{name}: strides {strides} (token, head) must be non-negative multiples of 8 elements: a lane loads 16 bytes")
    if x.storage_offset() % 8:
        raise ValueError(f"{name}: storage offset {x.storage_offset()} elements is not 16-byte aligned (a multiple of 8): a lane loads 16 bytes")
    return x.shape[1], strides


def _f32(x):
    """x rounded to float32, as a Python float (inf where it overflows)."""
    try:
        with np.errstate(over="ignore"):
            return float(np.float32(float(x)))
    except OverflowError:      # an int too large for a double
        return math.inf


def _norm_weight_arg(w, name, d):
    """A weight of the per-head RMSNorm: an fp32 [d] contiguous tensor, 16-byte aligned -- a lane loads its eight in two 16-byte
    loads.  (Its device is checked with the other tensors'.)"""
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] != d:
        raise ValueError(f"{name}: expected a 1-d tensor [{d}] (one weight per element of head_dim), got "
                         f"{tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
    if w.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {w.dtype}, expected torch.float32 (convert a checkpoint's bf16 weight, and fold Gemma's "
                         "1 + w, once: the caller builds the weights as it builds cos and sin)")
    if not w.is_contiguous():
        raise ValueError(f"{name} must be contiguous (got stride {tuple(w.stride())}; call .contiguous())")
    if w.storage_offset() % 4:
        raise ValueError(f"{name}: storage offset {w.storage_offset()} elements is not 16-byte aligned (a multiple of 4): a lane loads 16 bytes")


def _rope_ragged_call(Q, K_new, V_new, K, V, block_table, cos, sin, cu_or_plan, seqlens_k, interleaved, k_descale, v_descale, Q_out,
                      stream, norm=None):
    """rope_kv_cache_append_ragged (block_table None) and _paged, kv_cache_append_ragged (cos, sin, Q None) and _paged, and
    norm_rope_kv_cache_append_ragged (norm = (q_weight, k_weight, eps)) and _paged: one set of checks for the six, the uniform
    calls' in their order.  Nothing here reads a device value."""
    paged = block_table is not None
    kname, vname = ("K_pages", "V_pages") if paged else ("K_cache", "V_cache")
    want = "[n_pages, H_kv, page_size, d]" if paged else "[B, H_kv, N_cap, d]"
    how = "pass token-major [T, H, d] views, e.g. the Q, K and V slices of one fused [T, H_q + 2 H_kv, d] projection output"
    Hkv, strides = _ragged_rows_arg(K_new, "K_new", "H_kv", how)
    _ragged_rows_arg(V_new, "V_new", "H_kv", how)
    T, _, d = K_new.shape
    if tuple(V_new.shape) != tuple(K_new.shape):
        raise ValueError(f"V_new: shape {tuple(V_new.shape)} does not match K_new {tuple(K_new.shape)}")
    if d not in (64, 128):
        raise ValueError(f"K_new: head_dim {d}, expected 64 or 128")
    if tuple(V_new.stride()) != tuple(K_new.stride()):
        raise ValueError(f"V_new: strides {tuple(V_new.stride())} differ from K_new's {tuple(K_new.stride())}: one (token, head) "
                         f"stride pair serves both; {how}")
    Hq, q_strides = 0, (0, 0)
    if Q is not None:
        Hq, q_strides = _ragged_rows_arg(Q, "Q", "H_q", how)
        if Q.shape[0] != T or Q.shape[2] != d or Hq % Hkv:
            raise ValueError(f"Q: shape {tuple(Q.shape)} does not match K_new {tuple(K_new.shape)}: expected [{T}, H_q, {d}] with "
                             f"H_kv = {Hkv} dividing H_q")
    elif Q_out is not None:
        raise ValueError("Q_out: given without Q (a K/V-only call has neither)")
    if (Hq + Hkv) * T > 0x7fffffff:
        raise ValueError(f"K_new: {T} tokens x {Hq + Hkv} heads is more rows than an int indexes")
    for n, t in ((kname, K), (vname, V)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{n}: expected a 4-d tensor {want}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    n0, hk, n2, dk = K.shape
    if hk != Hkv or dk != d or n0 < 1 or n2 < 1:
        raise ValueError(f"{kname}: shape {tuple(K.shape)} does not match K_new {tuple(K_new.shape)}: expected {want} with H_kv = {Hkv}, d = {d}")
    if paged and n2 % DECODE_PAGE_GRAIN:
        raise ValueError(f"K_pages: page_size {n2} is not a multiple of {DECODE_PAGE_GRAIN} (the decode kernel's key tile; a page "
                         "of 16 keys is not taken)")
    if tuple(V.shape) != tuple(K.shape):
        raise ValueError(f"{vname}: shape {tuple(V.shape)} does not match {kname} {tuple(K.shape)}")
    fp8 = _kv_dtypes(K_new, K, V, kname, vname)
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if t is not None:
            _descale_arg(t, K_new, Hkv, name, fp8, kname)
    if (cos is None) != (sin is None):
        raise ValueError("cos and sin come as a pair: both tensors, or both None for an append without rotation")
    if cos is not None:
        _rope_tables_arg(cos, sin, d, 0)
    flag = _rope_interleaved(interleaved)
    if norm is not None:
        q_weight, k_weight, eps = norm
        if Q is not None:
            _norm_weight_arg(q_weight, "q_weight", d)
        elif q_weight is not None:
            raise ValueError("q_weight: given without Q (a K/V-only call normalises K alone)")
        _norm_weight_arg(k_weight, "k_weight", d)
        # as the kernel gets it: a C float (1e-46 is 0.0f there and 1e39 is inf)
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.floating)) or not math.isfinite(_f32(eps)) or _f32(eps) <= 0:
            raise ValueError(f"eps: {eps!r}, expected a finite float > 0 (as a float32)")
    G = Hq // Hkv if Hq else 1      # a K/V-only call takes a plan of any G; one built here is built for G = 1
    if isinstance(cu_or_plan, ExtendRaggedPlan):
        plan = cu_or_plan
        if plan.total_q != T or (Hq and plan.H_q // plan.H_kv != G):
            raise ValueError(f"plan: built for H_q / H_kv = {plan.H_q // plan.H_kv} and total_q = {plan.total_q}; this step has "
                             + (f"H_q / H_kv = {G} and " if Hq else "") + f"total_q = {T} (K_new {tuple(K_new.shape)})")
        B = plan.B
    else:
        plan = None
        B = _cu_seqlens_q_arg(cu_or_plan)
    if seqlens_k is None:
        raise ValueError("seqlens_k is required: token t of sequence b has position seqlens_k[b] - q_b + (t - start_b) (the lengths "
                         "AFTER the append, the ragged extend call's tensor)")
    if paged:
        max_pages = _block_table_arg(block_table, K_new, B)
        capacity = max_pages * n2
        if capacity > 0x7fffffff - (DECODE_MAX_SPLITS + 2) * 128:
            raise ValueError(f"block_table: {max_pages} pages of {n2} keys is a capacity of {capacity} keys, above what an int indexes")
    else:
        if n0 != B:
            raise ValueError(f"K_cache: {n0} sequences, cu_seqlens_q (the plan) has {B}")
        capacity = n2
    rot_dim, n_positions = (0, 0) if cos is None else _rope_tables_arg(cos, sin, d, capacity)
    _seqlens_arg(seqlens_k, K_new, B)
    _kv_append_devices(K_new, V_new, K, V, kname, vname, tuple(K.shape))
    for n, t in ((kname, K), (vname, V)):
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous (got stride {tuple(t.stride())})")
    if Q is not None and (not Q.is_cuda or Q.device != K_new.device):
        raise ValueError(f"Q is on {Q.device}, expected {K_new.device}")
    for n, t in (("cos", cos), ("sin", sin)):
        if t is None:
            continue
        if not t.is_cuda or t.device != K_new.device:
            raise ValueError(f"{n} is on {t.device}, expected {K_new.device}: the kernel reads the tables on the device when it runs")
        if not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous (got stride {tuple(t.stride())}; call .contiguous())")
        if t.data_ptr() % 16:
            raise ValueError(f"{n}: not 16-byte aligned (storage offset {t.storage_offset()} elements): a lane loads 16 bytes")
    if norm is not None:
        for n, t in (("q_weight", q_weight), ("k_weight", k_weight)):
            if t is not None and (not t.is_cuda or t.device != K_new.device):
                raise ValueError(f"{n} is on {t.device}, expected {K_new.device}: the kernel reads the weights on the device when it runs")
    if Q is None:
        pass
    elif Q_out is None:
        Q_out = torch.empty(T, Hq, d, dtype=torch.bfloat16, device=K_new.device)
    elif (not isinstance(Q_out, torch.Tensor) or tuple(Q_out.shape) != (T, Hq, d) or Q_out.dtype != torch.bfloat16
          or not Q_out.is_contiguous() or Q_out.device != K_new.device):
        raise ValueError(f"Q_out: expected a contiguous torch.bfloat16 tensor {(T, Hq, d)} on {K_new.device}")
    if plan is None:
        if cu_or_plan.device != K_new.device:
            raise ValueError(f"cu_seqlens_q is on {cu_or_plan.device}, expected {K_new.device}")
        plan = extend_ragged_plan(cu_or_plan, Hq if Hq else Hkv, Hkv, T, stream=stream)
    elif plan.tensor.device != K_new.device:
        raise ValueError(f"plan is on {plan.tensor.device}, expected {K_new.device}")
    lib = _capi.lib()
    head = (_ptr(Q), _ptr(Q_out), K_new.data_ptr(), V_new.data_ptr(), K.data_ptr(), V.data_ptr())
    mid = (_ptr(cos), _ptr(sin), plan.tensor.data_ptr(), _nbytes(plan.tensor), seqlens_k.data_ptr(), _ptr(k_descale), _ptr(v_descale))
    tail = (d, rot_dim, n_positions, flag, *q_strides, *strides, FA2_DTYPE_BF16, FA2_DTYPE_FP8_E4M3 if fp8 else FA2_DTYPE_BF16,
            _stream_ptr(stream))
    if norm is not None:
        mid = mid[:2] + (_ptr(q_weight), k_weight.data_ptr(), float(eps)) + mid[2:]
    name = ("fa2_norm_rope_kv_append_ragged" if norm is not None else "fa2_rope_kv_append_ragged") + ("_paged" if paged else "")
    if paged:
        st = getattr(lib, name)(*head, block_table.data_ptr(), *mid, B, Hq, Hkv, T, n0, n2, max_pages, *tail)
    else:
        st = getattr(lib, name)(*head, *mid, B, Hq, Hkv, T, capacity, *tail)
    check(st, name)
    return Q_out


def rope_kv_cache_append_ragged(Q, K_new, V_new, K_cache, V_cache, cos, sin, cu_seqlens_q_or_plan, seqlens_k, *, interleaved=False,
                                k_descale=None, v_descale=None, Q_out=None, stream=None):
    """rope_kv_cache_append with an n_new PER SEQUENCE and TOKEN-MAJOR tensors (fa2_rope_kv_append_ragged,
    include/fa2_rope_ragged_mi355x.h): the cache-writing half of a continuous-batching step, beside
    flash_attention_2_extend_ragged.  ONE launch rotates and appends the K of the step's T packed tokens, appends their V, and
    writes the rotated queries; returns Q_out, bf16 [T, H_q, d] contiguous, what flash_attention_2_extend_ragged takes.  A step is:
    seqlens_k[b] += q_b (in place), extend_ragged_plan (once), then per layer rope_kv_cache_append_ragged(..., plan, seqlens_k) and
    flash_attention_2_extend_ragged(Q_out, ..., plan, seqlens_k); one captured graph serves every step while the mix changes.
    Q [T, H_q, d], K_new, V_new [T, H_kv, d]: bf16 VIEWS (d = 64 | 128) with stride(-1) == 1 and strides that are non-negative
    multiples of 8; K_new and V_new share theirs, Q has its own: the three slices of a fused [T, H_q + 2 H_kv, d] projection
    output are passed as they are.  Q=None is a K/V-only call (returns None).  K_cache, V_cache [B, H_kv, N_cap, d], bf16 or e4m3.
    cu_seqlens_q_or_plan: an int32 [B + 1] DEVICE tensor (sequence b owns tokens cu[b] .. cu[b + 1] - 1, q_b = 0 allowed; the plan
    is then built inside this call, one more small launch), or the ExtendRaggedPlan extend_ragged_plan built from it -- the one
    the attention call of the step takes.  The host never reads cu_seqlens_q, seqlens_k, a descale or a table.
    POSITION: token t of sequence b has position seqlens_k[b] - q_b + (t - cu[b]) -- its cache row, its table row, and the position
    the ragged extend's mask gives that query.  cos, sin, interleaved, the arithmetic, the e4m3 store and the write-or-drop rule are
    rope_kv_cache_append's; cos = sin = None appends without rotating.  A sequence's rows are bit for bit what
    rope_kv_cache_append writes when called on that sequence alone.
    Q_out: EVERY row t < T is written: rotated where the token is owned and 0 <= position < capacity, +0.0 throughout elsewhere
    (a dropped position, a token no sequence owns); such a token's K and V are dropped.  Allocated when not given -- pass one for
    graph capture.  A plan built for another B, H_q / H_kv or T makes the kernel leave without a store."""
    return _rope_ragged_call(Q, K_new, V_new, K_cache, V_cache, None, cos, sin, cu_seqlens_q_or_plan, seqlens_k, interleaved, k_descale,
                             v_descale, Q_out, stream)


def rope_kv_cache_append_ragged_paged(Q, K_new, V_new, K_pages, V_pages, block_table, cos, sin, cu_seqlens_q_or_plan, seqlens_k, *,
                                      interleaved=False, k_descale=None, v_descale=None, Q_out=None, stream=None):
    """rope_kv_cache_append_ragged into a pool of pages (fa2_rope_kv_append_ragged_paged), the pool
    flash_attention_2_extend_ragged_paged reads: K_pages, V_pages [n_pages, H_kv, page_size, d] and block_table int32 [B, max_pages]
    exactly as rope_kv_cache_append_paged takes them.  A token whose table entry lies outside [0, n_pages) has its K and V
    DROPPED; its Q_out row is still the rotated query.  PAGES WRITTEN BY ONE CALL MUST BELONG TO ONE SEQUENCE EACH."""
    if block_table is None:
        raise ValueError("block_table must be an int32 device tensor [B, max_pages]")
    return _rope_ragged_call(Q, K_new, V_new, K_pages, V_pages, block_table, cos, sin, cu_seqlens_q_or_plan, seqlens_k, interleaved,
                             k_descale, v_descale, Q_out, stream)


def norm_rope_kv_cache_append_ragged(Q, K_new, V_new, K_cache, V_cache, cos, sin, q_weight, k_weight, eps, cu_seqlens_q_or_plan,
                                     seqlens_k, *, interleaved=False, k_descale=None, v_descale=None, Q_out=None, stream=None):
    """rope_kv_cache_append_ragged with a PER-HEAD RMSNorm of every new Q row and K row in front of the rotation
    (fa2_norm_rope_kv_append_ragged, include/fa2_rope_norm_mi355x.h): the cache-writing half of a step for models that normalise
    queries and keys over head_dim before they rotate them (Qwen3, Gemma 3).  ONE launch; the Q, K and V slices of the fused
    projection output go in as they are, no framework norm and no normalised copy in between.  Every argument but three is
    rope_kv_cache_append_ragged's, with its rules, its Q_out (every row written, +0.0 throughout for dropped and un-owned
    tokens), its plan contract and its write-or-drop rule; V is copied untouched.
    q_weight, k_weight: fp32 [d] contiguous DEVICE tensors, read on the device; q_weight is None exactly when Q is None.  The caller
    builds them as it builds cos and sin: Gemma's 1 + w and a checkpoint's bf16 weight are folded or converted once.  eps: a
    finite float > 0.
    ARITHMETIC, all fp32 with one rounding per operation and no fused multiply-add: the squares are summed in a fixed order
    (eight per 16-byte chunk left to right, then a butterfly over the row's chunks), r = 1 / sqrt(sum / d + eps) with a correctly
    rounded sqrt and division, n = ((x * r) * w).bfloat16() -- ONE rounding to bf16, Gemma 3's form; HF Qwen3's extra bf16 rounding
    before the weight is a different, less exact expression and is not reproduced.  The call is bit for bit
    rope_kv_cache_append_ragged applied to the normalised bf16 tensors; cos = sin = None stores n itself."""
    return _rope_ragged_call(Q, K_new, V_new, K_cache, V_cache, None, cos, sin, cu_seqlens_q_or_plan, seqlens_k, interleaved, k_descale,
                             v_descale, Q_out, stream, norm=(q_weight, k_weight, eps))


def norm_rope_kv_cache_append_ragged_paged(Q, K_new, V_new, K_pages, V_pages, block_table, cos, sin, q_weight, k_weight, eps,
                                           cu_seqlens_q_or_plan, seqlens_k, *, interleaved=False, k_descale=None, v_descale=None,
                                           Q_out=None, stream=None):
    """norm_rope_kv_cache_append_ragged into a pool of pages (fa2_norm_rope_kv_append_ragged_paged): K_pages, V_pages, block_table
    and the drop rule exactly as rope_kv_cache_append_ragged_paged takes them.  A token whose table entry lies outside
    [0, n_pages) has its K and V DROPPED; its Q_out row is still the normalised, rotated query.  PAGES WRITTEN BY ONE CALL MUST
    BELONG TO ONE SEQUENCE EACH."""
    if block_table is None:
        raise ValueError("block_table must be an int32 device tensor [B, max_pages]")
    return _rope_ragged_call(Q, K_new, V_new, K_pages, V_pages, block_table, cos, sin, cu_seqlens_q_or_plan, seqlens_k, interleaved,
                             k_descale, v_descale, Q_out, stream, norm=(q_weight, k_weight, eps))


def kv_cache_append_ragged(K_new, V_new, K_cache, V_cache, cu_seqlens_q_or_plan, seqlens_k, k_descale=None, v_descale=None, stream=None):
    """kv_cache_append with an n_new PER SEQUENCE and token-major sources: rope_kv_cache_append_ragged without rotation and without
    queries (fa2_rope_kv_append_ragged with rot_dim = 0, H_q = 0), byte for byte kv_cache_append on every sequence.  K_new, V_new:
    bf16 [T, H_kv, d] views; a plan built for any H_q / H_kv serves (one built here is built for 1).  Returns None."""
    _rope_ragged_call(None, K_new, V_new, K_cache, V_cache, None, None, None, cu_seqlens_q_or_plan, seqlens_k, False, k_descale, v_descale,
                      None, stream)


def kv_cache_append_ragged_paged(K_new, V_new, K_pages, V_pages, block_table, cu_seqlens_q_or_plan, seqlens_k, k_descale=None,
                                 v_descale=None, stream=None):
    """kv_cache_append_ragged into a pool of pages: kv_cache_append_paged's pool, table and drop rule.  Returns None."""
    if block_table is None:
        raise ValueError("block_table must be an int32 device tensor [B, max_pages]")
    _rope_ragged_call(None, K_new, V_new, K_pages, V_pages, block_table, None, None, cu_seqlens_q_or_plan, seqlens_k, False, k_descale,
                      v_descale, None, stream)


def _sink_pair(sink, dsink, Q, heads_dim):
    """sink= and dsink= of a backward, each checked beside Q (_sink_arg); dsink without sink is refused."""
    if sink is not None:
        _sink_arg(sink, Q, heads_dim)
        if dsink is not None:
            _sink_arg(dsink, Q, heads_dim, "dsink")
    elif dsink is not None:
        raise ValueError("dsink belongs to a call with sink=")


def _backward_symbol(plain, ptrs, Q, H, sink, dsink, dL):
    """(symbol, pointers, dsink) of a backward of the _qk or the packed family -- the one place the symbol is picked: `plain`
    for a call without sinks and dL, else its _sink or _lse sibling with the optional pointers inserted among the nine (dsink
    is allocated when the call has sinks and brought none)."""
    stem = plain[:-len("_qk")] if plain.endswith("_qk") else plain
    if sink is not None and dsink is None:
        dsink = torch.empty(H, dtype=torch.float32, device=Q.device)
    if dL is not None:
        sp, dp = (None, None) if sink is None else (sink.data_ptr(), dsink.data_ptr())
        return stem + "_lse", (*ptrs[:3], sp, *ptrs[3:6], dL.data_ptr(), *ptrs[6:], dp), dsink
    if sink is not None:
        return stem + "_sink", (*ptrs[:3], sink.data_ptr(), *ptrs[3:], dsink.data_ptr()), dsink
    return plain, ptrs, dsink


def flash_attention_2_qk_backward(Q, K, V, O, L, dO, softmax_scale=None, causal=False,
                                  dQ=None, dK=None, dV=None, workspace=None, stream=None, phases=7, sink=None, dsink=None, dL=None):
    """dQ, dK, dV = FA2 backward of flash_attention_2_qk_forward (fa2_backward_qk): dO like O, dK / dV like K / V.  N_q != N_k
    runs the two deterministic kernels (phases: 1 = D and the row constants, 2 = dQ, 4 = dK/dV; 8, the single kernel, is
    refused); N_q == N_k is flash_attention_2_backward.  A row that saw no key gets dQ = 0.
    sink (fa2_backward_sink): the forward's sinks, with its O and L; returns (dQ, dK, dV, dsink), dsink fp32 [H] (written with
    phase bit 0).
    dL (fa2_backward_lse): the gradient of L, fp32 shaped like L -- dS = P o (dP - D + dL), through the row constant D' = D - dL
    that phase bit 0 writes; a row with L = -inf ignores it.  With or without sink=."""
    _sink_pair(sink, dsink, Q, 1)
    B, H, Hkv, Nq, Nk, d = _qk_shapes(Q, K, V)
    for n, t in (("O", O), ("dO", dO)):
        _like(t, n, Q, (B, H, Nq, d), Q.dtype)
    _rows(L, "L", Q, B, H, Nq)
    if dL is not None:
        _rows(dL, "dL", Q, B, H, Nq)
    scale = _scale(softmax_scale, d)
    dQ = torch.empty_like(Q) if dQ is None else _like(dQ, "dQ", Q, (B, H, Nq, d), Q.dtype)
    dK = torch.empty_like(K) if dK is None else _like(dK, "dK", Q, (B, Hkv, Nk, d), Q.dtype)
    dV = torch.empty_like(V) if dV is None else _like(dV, "dV", Q, (B, Hkv, Nk, d), Q.dtype)
    lib = _capi.lib()
    if workspace is None:
        workspace = torch.empty(lib.fa2_backward_qk_workspace_bytes(B, H, Hkv, Nq, Nk, d, FA2_DTYPE_BF16), dtype=torch.uint8, device=Q.device)
    _workspace_arg(workspace, Q)
    ptrs = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), dO.data_ptr(), dQ.data_ptr(), dK.data_ptr(), dV.data_ptr())
    name, ptrs, dsink = _backward_symbol("fa2_backward_qk", ptrs, Q, H, sink, dsink, dL)
    check(getattr(lib, name)(*ptrs, B, H, Hkv, Nq, Nk, d, scale, FA2_DTYPE_BF16, 1 if causal else 0, workspace.data_ptr(), _nbytes(workspace),
                             _stream_ptr(stream), int(phases)), name)
    return (dQ, dK, dV) if sink is None else (dQ, dK, dV, dsink)


def _grad_pair(O, dO, dL):
    """What a backward is handed for the outputs (O, L) of an op that does not materialise absent gradients, as the raw halves
    take it: dO contiguous (zeros when only L was used), dL contiguous fp32 or None."""
    dO = torch.zeros_like(O) if dO is None else dO.contiguous()
    return dO, None if dL is None else dL.float().contiguous()


class _AttentionQK(torch.autograd.Function):
    """flash_attention_2_qk_forward / _backward or, with a plan, flash_attention_2_varlen_forward / _backward as one differentiable
    op (as _Attention)."""

    @staticmethod
    def forward(ctx, Q, K, V, plan, softmax_scale, causal, sink=None, return_lse=False):
        Q, K, V = Q.contiguous(), K.contiguous(), V.contiguous()
        scale = _scale(softmax_scale, Q.shape[-1])
        s32 = _sink_param(sink)                      # the kernels read fp32 sinks; the parameter may be bf16
        if plan is None:
            O, L = flash_attention_2_qk_forward(Q, K, V, scale, causal=causal, sink=s32)
        else:
            O, L = flash_attention_2_varlen_forward(Q, K, V, plan, scale, causal=causal, sink=s32)
        ctx.save_for_backward(Q, K, V, O, L, s32)
        ctx.plan, ctx.scale, ctx.causal, ctx.sink_dtype = plan, scale, bool(causal), None if sink is None else sink.dtype
        ctx.set_materialize_grads(False)             # an output nobody used arrives as None: no dL, the call of before
        return (O, L) if return_lse else O

    @staticmethod
    def backward(ctx, dO, dL=None):
        Q, K, V, O, L, s32 = ctx.saved_tensors
        dO, dL = _grad_pair(O, dO, dL)
        plan = () if ctx.plan is None else (ctx.plan,)
        backward = flash_attention_2_qk_backward if ctx.plan is None else flash_attention_2_varlen_backward
        dQ, dK, dV, *dsink = backward(Q, K, V, O, L, dO, *plan, ctx.scale, causal=ctx.causal, sink=s32, dL=dL)
        return dQ, dK, dV, None, None, None, dsink[0].to(ctx.sink_dtype) if dsink else None, None


def attention_qk(Q, K, V, softmax_scale=None, causal=False, sink=None, return_lse=False):
    """attention() for N_q queries against N_k keys: Q [B, H, N_q, d], K and V [B, H_kv, N_k, d] bf16 device tensors (d = 64 | 128,
    H_kv dividing H); causal: bottom-right aligned (the last query sees every key).  With gradients, shaped like K and V.
    sink: attention sinks, a bf16 or fp32 tensor (a parameter) of H logits (flash_attention_2_qk_forward); its gradient comes
    back in its dtype.
    return_lse: return (O, L), L the fp32 [B, H, N_q] log-sum-exp of every row (-inf on a row without a key or sink), both
    differentiable (merge_attention_states, a z-loss)."""
    return _AttentionQK.apply(Q, K, V, None, softmax_scale, causal, sink, bool(return_lse))


class VarlenPlan:
    """The work plan of a packed variable-length batch (fa2_varlen_plan_build): built on the host from cu_seqlens -- a list, a
    numpy array or a CPU integer tensor of n_seqs + 1 non-decreasing offsets starting at 0 -- when the object is made (no GPU
    needed), uploaded to a device the first time a call needs it there and kept for every later call: make one per batch
    layout and reuse it for every layer and step (and make the first call before capturing a graph: the upload is a copy).
    Sequence i owns rows [cu_seqlens[i], cu_seqlens[i+1]) of every head of the packed [H, T, d] tensors.
    cu_seqlens_k: a second list of n_seqs + 1 offsets for the key side (fa2_varlen_plan_build_qk): sequence i then owns rows
    cu_seqlens[i] : cu_seqlens[i+1] of Q's T_q = total rows and rows cu_seqlens_k[i] : cu_seqlens_k[i+1] of K's and V's
    T_k = total_k rows, and the packed calls take K, V [H_kv, T_k, d].  None, or a list equal to cu_seqlens: the one-sided plan."""

    _HEADER_INTS, _ITEM_INTS = 8, 5

    @staticmethod
    def _offsets(cu_seqlens, name):
        if isinstance(cu_seqlens, torch.Tensor):
            if cu_seqlens.is_cuda:
                raise ValueError(f"{name} must be host data (a list, a numpy array or a CPU tensor): the plan is built on the host")
            if cu_seqlens.is_floating_point() or cu_seqlens.is_complex() or cu_seqlens.dtype == torch.bool:
                raise ValueError(f"{name} must hold integers, got {cu_seqlens.dtype}")
            cu_seqlens = cu_seqlens.numpy()
        cu = np.asarray(cu_seqlens)
        if cu.ndim != 1 or cu.size < 2 or not np.issubdtype(cu.dtype, np.integer):
            raise ValueError(f"{name}: expected n_seqs + 1 >= 2 integer offsets in one dimension")
        if int(cu.max()) > 2 ** 31 - 1 or int(cu.min()) < 0:
            raise ValueError(f"{name}: offsets must be non-negative and fit 32 bits")
        cu = np.ascontiguousarray(cu, dtype=np.int32)
        cu.setflags(write=False)
        return cu

    def __init__(self, cu_seqlens, cu_seqlens_k=None):
        self.cu_seqlens = self._offsets(cu_seqlens, "cu_seqlens")
        lib = _capi.lib()
        n_seqs, total = self.cu_seqlens.size - 1, int(self.cu_seqlens[-1])
        if cu_seqlens_k is None:
            self.cu_seqlens_k = self.cu_seqlens
            blob = np.zeros(max(lib.fa2_varlen_plan_bytes(n_seqs, total), 4 * self._HEADER_INTS), dtype=np.uint8)
            st = lib.fa2_varlen_plan_build(self.cu_seqlens.ctypes.data, n_seqs, blob.ctypes.data, blob.size)
            if st:
                raise ValueError(f"cu_seqlens {self.cu_seqlens.tolist()[:8]}{'...' if n_seqs > 7 else ''}: fa2_varlen_plan_build status {st} "
                                 f"({lib.fa2_status_string(st).decode()}): offsets start at 0, never decrease and end at T >= 1")
        else:
            self.cu_seqlens_k = self._offsets(cu_seqlens_k, "cu_seqlens_k")
            if self.cu_seqlens_k.size != self.cu_seqlens.size:
                raise ValueError(f"cu_seqlens_k: {self.cu_seqlens_k.size} offsets beside the {self.cu_seqlens.size} of cu_seqlens "
                                 "(both lists have n_seqs + 1 entries)")
            blob = np.zeros(max(lib.fa2_varlen_plan_bytes_qk(n_seqs, total, int(self.cu_seqlens_k[-1])), 4 * self._HEADER_INTS), dtype=np.uint8)
            st = lib.fa2_varlen_plan_build_qk(self.cu_seqlens.ctypes.data, self.cu_seqlens_k.ctypes.data, n_seqs, blob.ctypes.data, blob.size)
            if st:
                raise ValueError(f"cu_seqlens {self.cu_seqlens.tolist()[:8]}{'...' if n_seqs > 7 else ''} / cu_seqlens_k "
                                 f"{self.cu_seqlens_k.tolist()[:8]}{'...' if n_seqs > 7 else ''}: fa2_varlen_plan_build_qk status {st} "
                                 f"({lib.fa2_status_string(st).decode()}): each list starts at 0, never decreases and ends at a total >= 1")
        head = blob[:4 * self._HEADER_INTS].view(np.int32)
        self.n_seqs, self.total, n_row, n_key, self.max_len = int(head[2]), int(head[3]), int(head[4]), int(head[5]), int(head[6])
        self.two_sided = int(head[7]) != 0                 # what the blob says: equal lists give the one-sided plan
        self.total_k = int(head[7]) if self.two_sided else self.total
        self.max_len_k = int(np.diff(self.cu_seqlens_k).max())
        lo, mid = 4 * self._HEADER_INTS, 4 * (self._HEADER_INTS + self._ITEM_INTS * n_row)
        self._blob = np.ascontiguousarray(blob[:mid + 4 * self._ITEM_INTS * n_key])      # what the launches validate and the devices hold
        self._blob.setflags(write=False)
        # rows of (q_row0, k_row0, len_q, len_k, block), in launch order
        self.row_items = self._blob[lo:mid].view(np.int32).reshape(n_row, self._ITEM_INTS)
        self.key_items = self._blob[mid:].view(np.int32).reshape(n_key, self._ITEM_INTS)
        self._dev = {}

    @property
    def nbytes(self):
        return self._blob.size

    def host_ptr(self):
        return self._blob.ctypes.data

    def device(self, device):
        """The plan's copy on `device` (uploaded once per device)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"the plan is uploaded to GPUs, not to {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self._blob.copy()).to(device)
        return self._dev[device]


def _htd(x, name, dtype=torch.bfloat16):
    """A packed tensor [H, T, d]: shape first (a 3-D tensor), then what the C ABI takes on trust -- device, contiguity, dtype."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if x.dim() != 3:
        raise ValueError(f"{name}: expected a packed [H, T, d] tensor, got {tuple(x.shape)} (transpose a [T, H, d] tensor first)")
    if not x.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous [H][T][d] (got strides {tuple(x.stride())}; call .contiguous())")
    if x.dtype != dtype:
        raise ValueError(f"{name}: dtype {x.dtype}, expected {dtype} (packed variable-length attention is bf16 in this version)")
    return tuple(x.shape)


def _varlen_shapes(Q, K, V, plan):
    """(H, H_kv, T, T_k, d) of a packed problem, every relation between Q, K, V and the plan checked (T_k = T under a one-sided
    plan)."""
    if not isinstance(plan, VarlenPlan):
        raise ValueError("plan must be a VarlenPlan")
    for n, t in (("Q", Q), ("K", K), ("V", V)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{n}: expected a packed [H, T, d] tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} "
                             "(transpose a [T, H, d] tensor first)")
    H, T, d = Q.shape
    if T != plan.total:
        raise ValueError(f"Q: {T} rows per head, the plan's cu_seqlens end at T = {plan.total}")
    Hkv = K.shape[0]
    if Hkv < 1 or H % Hkv != 0:
        raise ValueError(f"K: {Hkv} key/value heads do not divide {H} query heads")
    Tk = plan.total_k
    if tuple(K.shape) != (Hkv, Tk, d) or tuple(V.shape) != (Hkv, Tk, d):
        raise ValueError(f"K {tuple(K.shape)} / V {tuple(V.shape)}: expected {(Hkv, Tk, d)} beside Q {tuple(Q.shape)}"
                         + (f" (the plan's cu_seqlens_k end at T_k = {Tk})" if plan.two_sided else ""))
    for n, t in (("Q", Q), ("K", K), ("V", V)):
        _htd(t, n)
        if t.device != Q.device:
            raise ValueError(f"{n} is on {t.device}, expected {Q.device}")
    return H, Hkv, T, Tk, d


def _packed(x, name, ref, shape):
    if _htd(x, name) != shape:
        raise ValueError(f"{name}: shape {tuple(x.shape)} does not match {shape}")
    if x.device != ref.device:
        raise ValueError(f"{name} is on {x.device}, expected {ref.device}")
    return x


def flash_attention_2_varlen_forward(Q, K, V, plan, softmax_scale=None, causal=False, O=None, L=None, stream=None, sink=None):
    """O, L = FA2 forward over a packed variable-length batch (fa2_forward_varlen): Q [H, T, d], K and V [H_kv, T, d] (H_kv
    dividing H), bf16, d = 64 | 128; sequence i owns rows plan.cu_seqlens[i] : plan.cu_seqlens[i+1] of every head and attends only
    itself (causal: within itself).  L is fp32 [H, T].  A [T, H, d] tensor must be transposed (and made contiguous) first.
    Under a two-sided plan (VarlenPlan(cu_seqlens, cu_seqlens_k); fa2_forward_varlen_qk) K and V are [H_kv, T_k, d] and sequence i
    attends its own key rows, causal: bottom-right aligned; a query row that sees no key has O = 0 and L = -inf.
    sink (fa2_forward_varlen_sink, either kind of plan): fp32 [H] attention sinks, as in flash_attention_2_qk_forward."""
    if sink is not None:
        _sink_arg(sink, Q, 0)
    H, Hkv, T, Tk, d = _varlen_shapes(Q, K, V, plan)
    scale = _scale(softmax_scale, d)
    O = torch.empty_like(Q) if O is None else _packed(O, "O", Q, (H, T, d))
    L = torch.empty(H, T, dtype=torch.float32, device=Q.device) if L is None else _rows(L, "L", Q, 1, H, T)
    lib, ptrs = _capi.lib(), (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr())
    tail = (d, scale, FA2_DTYPE_BF16, 1 if causal else 0, plan.host_ptr(), plan.device(Q.device).data_ptr(), plan.nbytes, _stream_ptr(stream))
    if sink is not None:
        check(lib.fa2_forward_varlen_sink(*ptrs[:3], sink.data_ptr(), *ptrs[3:], H, Hkv, T, Tk, *tail), "fa2_forward_varlen_sink")
    elif plan.two_sided:
        check(lib.fa2_forward_varlen_qk(*ptrs, H, Hkv, T, Tk, *tail), "fa2_forward_varlen_qk")
    else:
        check(lib.fa2_forward_varlen(*ptrs, H, Hkv, T, *tail), "fa2_forward_varlen")
    return O, L


def flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, softmax_scale=None, causal=False,
                                      dQ=None, dK=None, dV=None, workspace=None, stream=None, sink=None, dsink=None, dL=None):
    """dQ, dK, dV = FA2 backward over a packed variable-length batch (fa2_backward_varlen; the two deterministic kernels): the
    tensors of flash_attention_2_varlen_forward, dO like O, dK / dV like K / V.  workspace: a uint8 device tensor of
    fa2_backward_varlen_workspace_bytes (allocated per call when omitted -- pass one for graph capture).  Under a two-sided plan
    (fa2_backward_varlen_qk) dK / dV are [H_kv, T_k, d]; a sequence with keys and no queries gets dK = dV = 0.
    sink (fa2_backward_varlen_sink): the forward's sinks, with its O and L; returns (dQ, dK, dV, dsink), dsink fp32 [H].
    dL (fa2_backward_varlen_lse): the gradient of L, fp32 [H, T], as in flash_attention_2_qk_backward."""
    _sink_pair(sink, dsink, Q, 0)
    H, Hkv, T, Tk, d = _varlen_shapes(Q, K, V, plan)
    for n, t in (("O", O), ("dO", dO)):
        _packed(t, n, Q, (H, T, d))
    _rows(L, "L", Q, 1, H, T)
    if dL is not None:
        _rows(dL, "dL", Q, 1, H, T)
    scale = _scale(softmax_scale, d)
    dQ = torch.empty_like(Q) if dQ is None else _packed(dQ, "dQ", Q, (H, T, d))
    dK = torch.empty_like(K) if dK is None else _packed(dK, "dK", Q, (Hkv, Tk, d))
    dV = torch.empty_like(V) if dV is None else _packed(dV, "dV", Q, (Hkv, Tk, d))
    lib = _capi.lib()
    if workspace is None:
        workspace = torch.empty(lib.fa2_backward_varlen_workspace_bytes(H, Hkv, T, d, FA2_DTYPE_BF16), dtype=torch.uint8, device=Q.device)
    _workspace_arg(workspace, Q)
    ptrs = (Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), L.data_ptr(), dO.data_ptr(), dQ.data_ptr(), dK.data_ptr(), dV.data_ptr())
    name, ptrs, dsink = _backward_symbol("fa2_backward_varlen_qk" if plan.two_sided else "fa2_backward_varlen", ptrs, Q, H, sink, dsink, dL)
    rows = (T,) if name == "fa2_backward_varlen" else (T, Tk)      # the one-list call has one T for both sides
    check(getattr(lib, name)(*ptrs, H, Hkv, *rows, d, scale, FA2_DTYPE_BF16, 1 if causal else 0, plan.host_ptr(), plan.device(Q.device).data_ptr(),
                             plan.nbytes, workspace.data_ptr(), _nbytes(workspace), _stream_ptr(stream)), name)
    return (dQ, dK, dV) if sink is None else (dQ, dK, dV, dsink)


def attention_varlen(Q, K, V, plan, softmax_scale=None, causal=False, sink=None, return_lse=False):
    """attention() over a packed variable-length batch: Q [H, T, d], K and V [H_kv, T, d] bf16 device tensors (d = 64 | 128, H_kv
    dividing H), plan a VarlenPlan of the batch's cu_seqlens; every sequence attends itself only.  With gradients.  Under a
    two-sided plan K and V are [H_kv, T_k, d] and so are their gradients.  sink: attention sinks, as in attention_qk.
    return_lse: return (O, L), L fp32 [H, T], both differentiable."""
    if not isinstance(plan, VarlenPlan):
        raise ValueError("plan must be a VarlenPlan")
    return _AttentionQK.apply(Q, K, V, plan, softmax_scale, causal, sink, bool(return_lse))


MERGE_MAX_PARTS = 8


def _merge_parts(Os, Ls):
    """The parts of a merge, checked like every tensor the C ABI takes on trust: 1..8 bf16 contiguous device tensors [..., d] of one
    shape on one device, and as many fp32 tensors of that shape without its last dimension.  Returns (n, rows, d)."""
    if not isinstance(Os, (list, tuple)) or not isinstance(Ls, (list, tuple)):
        raise ValueError("Os and Ls must be lists (or tuples) of tensors")
    n = len(Os)
    if not 1 <= n <= MERGE_MAX_PARTS or len(Ls) != n:
        raise ValueError(f"expected 1..{MERGE_MAX_PARTS} parts and as many Ls as Os, got {n} Os and {len(Ls)} Ls")
    ref = Os[0]
    if not isinstance(ref, torch.Tensor) or ref.dim() < 2 or ref.shape[-1] < 1:
        raise ValueError("Os[0] must be a tensor [..., d]")
    for i in range(n):
        _merge_like(Os[i], f"Os[{i}]", ref, tuple(ref.shape), torch.bfloat16)
        _merge_like(Ls[i], f"Ls[{i}]", ref, tuple(ref.shape[:-1]), torch.float32)
    return n, ref.numel() // ref.shape[-1], ref.shape[-1]


def _merge_like(x, name, ref, shape, dtype):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if not x.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if tuple(x.shape) != shape:
        raise ValueError(f"{name}: shape {tuple(x.shape)} does not match {shape}")
    if x.dtype != dtype:
        raise ValueError(f"{name}: dtype {x.dtype}, expected {dtype}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous (got strides {tuple(x.stride())}; call .contiguous())")
    if x.device != ref.device:
        raise ValueError(f"{name} is on {x.device}, expected {ref.device}")
    return x


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def merge_states_forward(Os, Ls, O=None, L=None, stream=None):
    """O, L = the attention over the union of the key sets of n <= 8 partial results (fa2_merge_states): Os bf16 [..., d] (d = 64 |
    128) and Ls fp32 [...], the (O_i, L_i) of forwards of the SAME queries over disjoint keys ([B, H, N, d] or packed [H, T, d]).
    L = logsumexp_i L_i, O = sum_i exp(L_i - L) O_i (fp32 arithmetic, bf16 result).  A part with L_i = -inf on a row is left out
    of the row; every part -inf: O = 0, L = -inf; one part: its own bits."""
    n, rows, d = _merge_parts(Os, Ls)
    ref = Os[0]
    O = torch.empty_like(ref) if O is None else _merge_like(O, "O", ref, tuple(ref.shape), torch.bfloat16)
    L = torch.empty_like(Ls[0]) if L is None else _merge_like(L, "L", ref, tuple(ref.shape[:-1]), torch.float32)
    st = _capi.lib().fa2_merge_states(_ptr_array(Os), _ptr_array(Ls), n, O.data_ptr(), L.data_ptr(), rows, d, FA2_DTYPE_BF16, _stream_ptr(stream))
    check(st, "fa2_merge_states")
    return O, L


def merge_states_backward(Os, Ls, O, L, dO, dL=None, dOs=None, dLs=None, stream=None):
    """dOs, dLs = the gradients of the parts of merge_states_forward (fa2_merge_states_backward) from its results O, L and their
    gradients dO (bf16, like O) and dL (fp32, like L, or None = 0): dO_i = exp(L_i - L) dO, dL_i = exp(L_i - L) (dL + rowsum(dO o
    (O_i - O))), both 0 where L_i = -inf.  dOs / dLs: lists of tensors to write into (allocated when omitted)."""
    n, rows, d = _merge_parts(Os, Ls)
    ref = Os[0]
    oshape, lshape = tuple(ref.shape), tuple(ref.shape[:-1])
    _merge_like(O, "O", ref, oshape, torch.bfloat16)
    _merge_like(L, "L", ref, lshape, torch.float32)
    _merge_like(dO, "dO", ref, oshape, torch.bfloat16)
    if dL is not None:
        _merge_like(dL, "dL", ref, lshape, torch.float32)
    if dOs is None:
        dOs = [torch.empty_like(ref) for _ in range(n)]
    if dLs is None:
        dLs = [torch.empty_like(L) for _ in range(n)]
    if not isinstance(dOs, (list, tuple)) or not isinstance(dLs, (list, tuple)) or len(dOs) != n or len(dLs) != n:
        raise ValueError(f"dOs and dLs must be lists of {n} tensors")
    for i in range(n):
        _merge_like(dOs[i], f"dOs[{i}]", ref, oshape, torch.bfloat16)
        _merge_like(dLs[i], f"dLs[{i}]", ref, lshape, torch.float32)
    st = _capi.lib().fa2_merge_states_backward(_ptr_array(Os), _ptr_array(Ls), O.data_ptr(), L.data_ptr(), dO.data_ptr(),
                                               None if dL is None else dL.data_ptr(), _ptr_array(dOs), _ptr_array(dLs), n, rows, d,
                                               FA2_DTYPE_BF16, _stream_ptr(stream))
    check(st, "fa2_merge_states_backward")
    return list(dOs), list(dLs)


class _MergeStates(torch.autograd.Function):
    """merge_states_forward / _backward as one differentiable op over (O_0 .. O_n-1, L_0 .. L_n-1)."""

    @staticmethod
    def forward(ctx, n, *parts):
        Os, Ls = [t.contiguous() for t in parts[:n]], [t.contiguous() for t in parts[n:]]
        O, L = merge_states_forward(Os, Ls)
        ctx.save_for_backward(O, L, *Os, *Ls)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return O, L

    @staticmethod
    def backward(ctx, dO, dL=None):
        O, L, *parts = ctx.saved_tensors
        dO, dL = _grad_pair(O, dO, dL)
        dOs, dLs = merge_states_backward(parts[:ctx.n], parts[ctx.n:], O, L, dO, dL)
        return (None, *dOs, *dLs)


def merge_attention_states(Os, Ls):
    """O, L = merge_states_forward(Os, Ls) with gradients: (O_i, L_i) from attention_qk(..., return_lse=True) (or attention,
    attention_varlen) of the same queries over disjoint key sets become the attention over the union of the keys, and the
    gradients of O and of L flow back into every part's O_i and L_i."""
    Os, Ls = list(Os), list(Ls)
    if not 1 <= len(Os) <= MERGE_MAX_PARTS or len(Ls) != len(Os):
        raise ValueError(f"expected 1..{MERGE_MAX_PARTS} parts and as many Ls as Os, got {len(Os)} Os and {len(Ls)} Ls")
    return _MergeStates.apply(len(Os), *Os, *Ls)


def attention_segments(Q, segments, softmax_scale=None, causal=False, sink=None, return_lse=False):
    """attention_qk of Q [B, H, N_q, d] over the concatenation, along the key axis, of segments = [(K_0, V_0), ...] (at most 8, each
    [B, H_kv, N_s, d]) WITHOUT copying K or V: a prompt chunk against a prefix cache that lives in another allocation, a shared
    prefix.  One attention_qk(..., return_lse=True) per segment, then merge_attention_states; with gradients for Q and every
    segment.  causal: bottom-right aligned over the whole key axis, applied in the last segment only -- which therefore must hold
    at least N_q keys, so that every earlier segment lies wholly in every query's past.  sink joins the softmax once, in the last
    segment.  return_lse: (O, L)."""
    if not isinstance(segments, (list, tuple)) or not 1 <= len(segments) <= MERGE_MAX_PARTS:
        raise ValueError(f"segments: expected a list of 1..{MERGE_MAX_PARTS} (K, V) pairs")
    for seg in segments:
        if not isinstance(seg, (list, tuple)) or len(seg) != 2:
            raise ValueError("segments: every entry is a (K, V) pair")
    last = len(segments) - 1
    if causal and isinstance(Q, torch.Tensor) and Q.dim() == 4 and isinstance(segments[last][0], torch.Tensor) and segments[last][0].dim() == 4 \
            and segments[last][0].shape[2] < Q.shape[2]:
        raise ValueError(f"causal attention over segments applies the mask in the last segment only: it must hold at least N_q = "
                         f"{Q.shape[2]} keys, so that every earlier segment lies wholly in every query's past (got "
                         f"{segments[last][0].shape[2]}; per-segment shifts are not supported)")
    outs = [attention_qk(Q, K, V, softmax_scale, causal and i == last, sink=sink if i == last else None, return_lse=True)
            for i, (K, V) in enumerate(segments)]
    O, L = outs[0] if last == 0 else merge_attention_states([o for o, _ in outs], [l for _, l in outs])
    return (O, L) if return_lse else O


def read_clocks(stream=None):
    """One sample of fa2_read_clocks on `stream`: an int64 device tensor [16][2] = per XCC (shader-clock ticks, 100 MHz
    reference ticks); rows of XCCs the device does not have stay zero.  Asynchronous: synchronise before reading."""
    out = torch.zeros(16, 2, dtype=torch.int64, device="cuda")
    check(_capi.lib().fa2_read_clocks(out.data_ptr(), _stream_ptr(stream)), "fa2_read_clocks")
    return out


def mean_shader_clock_mhz(before, after):
    """Mean shader clock between two read_clocks samples (the caller has synchronised): per XCC present in both,
    d(ticks) / d(reference ticks) x 100 MHz; the mean over those XCCs.  s_memtime counts per CU at its XCC's clock (a sample
    holds, per XCC, the counter furthest ahead), so a difference is only ever taken within one XCC."""
    a, b = before.cpu().tolist(), after.cpu().tolist()
    vals = [(y[0] - x[0]) / (y[1] - x[1]) * 100.0 for x, y in zip(a, b) if x[1] and y[1] and y[1] > x[1]]
    if not vals:
        raise RuntimeError("fa2_read_clocks: no XCC present in both samples")
    return sum(vals) / len(vals)


def bare_mfma_tflops(seconds=0.15, workgroups=256):
    """What this device sustains on nothing but bf16 MFMAs on random operands (fa2_mfma_probe): TFLOP/s over about `seconds`
    of back-to-back launches after a ramp, and the mean shader clock it held.  A measurement aid for bench.py."""
    lib = _capi.lib()
    ops = (torch.rand(1024, 8, device="cuda") * 2 - 1).to(torch.bfloat16)
    out = torch.empty(workgroups * 256, device="cuda")
    s = _stream_ptr()
    iters = 20000                                        # 4 x 20000 MFMAs per wave: ~1.4 ms per launch
    run = lambda: check(lib.fa2_mfma_probe(ops.data_ptr(), out.data_ptr(), iters, workgroups, s), "fa2_mfma_probe")
    for _ in range(30):                                  # ramp: the clock settles under load
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0 = read_clocks()
    e0.record()
    n = 0
    while True:
        for _ in range(10):
            run()
        n += 10
        e1.record()
        e1.synchronize()
        if e0.elapsed_time(e1) >= seconds * 1e3:
            break
    c1 = read_clocks()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    flops = 4.0 * iters * workgroups * 4 * 32768.0 * n
    return flops / ms / 1e9, mean_shader_clock_mhz(c0, c1)
