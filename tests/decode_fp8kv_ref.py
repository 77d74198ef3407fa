"""Decode attention over fp8 (OCP e4m3) KV caches (fa2_forward_decode_fp8kv, fa2_forward_decode_paged_fp8kv): quantised forms of
tests/decode_ref.py's and tests/decode_paged_ref.py's inputs and their references (a helper module, no tests:
tests/test_decode_fp8kv_reference.py certifies what is here on the CPU, tests/test_gpu_decode_fp8kv.py runs the kernels on it).

THE PROBLEM (include/fa2_mi355x.h).  K and V hold e4m3 bytes; head h's stored value is x / descale[h], so the scores are
softmax_scale k_descale[h] (Q . K8) and O = v_descale[h] P V8.  Everything else is decode_ref's.

quantise(X): the descale of head h is amax_h / 448 (448: the largest e4m3 value), the stored tensor (X / descale) clamped to
+-448 -- torch's cast does not saturate -- and cast.  dequantise: X8.float() * descale, in fp32.

REFERENCE AND GATES.  decode_paged_ref.reference64 and decode_ref.emulate ON THE DEQUANTISED TENSORS, gated by decode_ref's own
gates (within_gates) and the row gate of O of tests/decode_rows_ref.py on the same tensors: quantisation error is the caller's choice of format and no part of any gate -- what is gated is what the
kernels do with the values the cache holds."""
import functools

import torch

import decode_paged_ref as pr
import decode_ref as dr

E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
NAN_CODES = (0x7F, 0xFF)
GARBAGE_BYTES = (0x7F, 0xFF, 0x7E)      # the two NaN codes and 448


def quantise(X, headroom=0.0):
    """(X8 e4m3, descale fp32 [H_kv]) of a host tensor X [*, H_kv, *, d]: one descale per K/V head (dimension 1), amax_h / 448.
    headroom: head h's descale is (1 + headroom h) times that -- a cache whose heads keep different margins below 448.  The
    cases' heads share one amax (their garbage rows reach the generator's bound in every head), and a kernel that read the wrong
    head's descale must not pass."""
    amax = X.float().abs().amax(dim=(0, 2, 3))
    descale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax)) * (1.0 + headroom * torch.arange(X.shape[1]))
    X8 = (X.float() / descale[None, :, None, None]).clamp(-E4M3_MAX, E4M3_MAX).to(E4M3)
    return X8, descale


def dequantise(X8, descale):
    return X8.float() * (1.0 if descale is None else descale[None, :, None, None])


@functools.lru_cache(maxsize=None)
def inputs(i):
    """decode_ref.inputs(i) with the caches quantised: (Q, K8, V8, k_descale, v_descale, scale, lens int32, sink), made once."""
    Q, K, V, scale, lens, sink = dr.inputs(i)
    K8, kd = quantise(K, headroom=0.25)
    V8, vd = quantise(V, headroom=0.375)
    return Q, K8, V8, kd, vd, scale, lens, sink


@functools.lru_cache(maxsize=None)
def dequantised(i):
    _, K8, V8, kd, vd, _, _, _ = inputs(i)
    return dequantise(K8, kd), dequantise(V8, vd)


@functools.lru_cache(maxsize=None)
def reference(i):
    """float64 O and L of CASES[i] on the dequantised caches."""
    c = dr.CASES[i]
    Q, _, _, _, _, scale, _, sink = inputs(i)
    K, V = dequantised(i)
    return pr.reference64(Q, K, V, c["lens"], scale, c["causal"], sink)


def emulate(i, n_splits):
    c = dr.CASES[i]
    Q, _, _, _, _, scale, lens, sink = inputs(i)
    K, V = dequantised(i)
    return dr.emulate(Q, K, V, lens.tolist(), scale, c["causal"], sink, n_splits)


def pools(K8, V8, lens, P, seed, full=False):
    """(K_pages, V_pages e4m3, table, unused) of contiguous e4m3 caches: decode_paged_ref.build on their exact bf16 images, cast
    back.  unused: bool like a pool, True where build copied no key (the tail of each last page, every spare page); those bytes
    are e4m3 NaNs as they come out (build's NaN fill, cast)."""
    Kp, Vp, table = pr.build(K8.to(torch.bfloat16), V8.to(torch.bfloat16), lens, P, seed, full=full)
    return Kp.to(E4M3), Vp.to(E4M3), table, torch.isnan(Kp.float())


def gather(pool8, table, lens, P):
    """decode_paged_ref.gather of an e4m3 pool (on its bytes)."""
    return pr.gather(pool8.view(torch.uint8), table, lens, P).view(E4M3)


def filled(X8, where, byte):
    """A copy of the e4m3 tensor X8 with the bytes at `where` (bool, X8's shape) set to `byte`."""
    out = X8.clone()
    out.view(torch.uint8)[where] = byte
    return out


def past_lengths(shape, lens):
    """bool [B, H_kv, N_cap, d]: the rows of a contiguous cache at and beyond each sequence's length."""
    out = torch.zeros(shape, dtype=torch.bool)
    for b, n in enumerate(lens):
        out[b, :, int(n):] = True
    return out


@functools.lru_cache(maxsize=None)
def paged_inputs(i, P):
    """CASES[i] behind pages of P keys: (K_pages, V_pages, table, lens list, capacity, unused), made once."""
    c = dr.CASES[i]
    _, K8, V8, _, _, _, _, _ = inputs(i)
    Kp, Vp, table, unused = pools(K8, V8, c["lens"], P, 93000 + 17 * i + P, full=not c["seqlens"])
    cap = table.shape[1] * P
    return Kp, Vp, table, ([cap] * len(c["lens"]) if not c["seqlens"] else list(c["lens"])), cap, unused


@functools.lru_cache(maxsize=None)
def edge_inputs(P, d):
    """decode_paged_ref's page-edge batch with e4m3 pools: (Q, K_pages, V_pages, table, k_descale, v_descale, scale, lens, sink)."""
    c = pr.edge_case(P, d)
    B = len(c["lens"])
    g = torch.Generator().manual_seed(66000 + 13 * P + d)
    mk = lambda h, n: (torch.rand(B, h, n, d, generator=g) - 0.5).bfloat16()
    Q, K, V = mk(c["hq"], c["nq"]), mk(c["hkv"], pr.EDGE_NCAP), mk(c["hkv"], pr.EDGE_NCAP)
    K8, kd = quantise(K, headroom=0.25)
    V8, vd = quantise(V, headroom=0.375)
    Kp, Vp, table, _ = pools(K8, V8, c["lens"], P, 67000 + 13 * P + d)
    sink = dr.sink_of(c["hq"], 300 + P) if c["sink"] else None
    return Q, Kp, Vp, table, kd, vd, 1.0 / d ** 0.5, torch.tensor(c["lens"], dtype=torch.int32), sink
