"""float64 references for a differentiable log-sum-exp and for merging partial attention results (a helper module, no tests:
tests/test_lse_reference.py pins it to regimes.ref_attention and sink_ref on the CPU, tests/test_gpu_lse.py runs the kernels
against it).

THE RULES (include/fa2_mi355x.h, fa2_backward_lse / fa2_merge_states).  A loss that uses both outputs of a forward hands the backward
dO = g and dL = gl.  dL/dS_ij = P_ij, so
    dS = P o (g v^T - D + gl),      D = rowsum(g o O):      the row constant D' = D - gl, everything else as it was;
a sink s_h has dL/ds_h = exp(s_h - L), so dsink[h] = - sum exp(s_h - L) D' as well.  A row with L = -inf ignores its gl.
MERGING n parts (O_i, L_i) of the same queries over disjoint key sets:
    L = log sum_i exp L_i,      w_i = exp(L_i - L),      O = sum_i w_i O_i
    dO_i = w_i dO,              dL_i = w_i (dL + rowsum(dO o (O_i - O)))
a part with L_i = -inf on a row is absent from the row (its O_i is not read; dO_i = dL_i = 0), every part absent: O = 0, L = -inf.

VISIBILITY.  `shift` = None: every key; an integer: key j is visible to query i iff j <= i + shift.  shift = N_k - N_q is the
bottom-right causal mask of regimes.ref_attention; a part holding keys [c0, c1) of such a problem has shift N_k - N_q - c0."""
import numpy as np


def _f64(t):
    return t.double().numpy() if hasattr(t, "double") else np.asarray(t, dtype=np.float64)


def _bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().double().numpy()


def _group_sum(x, hkv):
    *lead, hq, n, d = x.shape
    return x.reshape(*lead, hkv, hq // hkv, n, d).sum(axis=-3)


def _scores(q, k, s, shift):
    nq, nk = q.shape[-2], k.shape[-2]
    S = s * (q @ np.swapaxes(k, -1, -2))
    if shift is not None:
        i, j = np.arange(nq)[:, None], np.arange(nk)[None, :]
        S = np.where(j <= i + shift, S, -np.inf)
    return S


def forward(q, k, v, s, shift=None, sink=None):
    """float64 O [..., H_q, N_q, d], L [..., H_q, N_q] for q [..., H_q, N_q, d], k, v [..., H_kv, N_k, d], sink [H_q] or None."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    G = q.shape[-3] // k.shape[-3]
    k, v = np.repeat(k, G, axis=-3), np.repeat(v, G, axis=-3)
    S = _scores(q, k, s, shift)
    sk = np.full(q.shape[:-1], -np.inf) if sink is None else np.broadcast_to(_f64(sink)[:, None], q.shape[:-1])
    m = np.maximum(S.max(axis=-1, initial=-np.inf), sk)
    seen = np.isfinite(m)
    m0 = np.where(seen, m, 0.0)
    p, ps = np.exp(S - m0[..., None]), np.exp(sk - m0)
    l = np.where(seen, p.sum(axis=-1) + ps, 1.0)
    L = np.where(seen, m0 + np.log(l), -np.inf)
    return (p / l[..., None]) @ v, L


def flow(q, k, v, g, gl, s, shift, O, L, sink=None, kernel_formats=False):
    """float64 dQ, dK, dV (and dsink [H_q] with a sink) as the kernels are fed: P = exp(S - L) from the given L (0 on rows with
    L = -inf), D' = rowsum(g o O) - gl from the given O (gl dropped on rows with L = -inf; gl None = 0), dS = P (g v^T - D'),
    dQ = s dS k, dK = s dS^T q, dV = P^T g, K and V repeated per group and dK, dV summed over it, dsink = - sum exp(sink - L) D'.
    kernel_formats (regimes.emulate's convention): D' rounded to fp32, P and dS to bf16 before the three products."""
    q, k, v, g, O, L = (_f64(t) for t in (q, k, v, g, O, L))
    hkv = k.shape[-3]
    G = q.shape[-3] // hkv
    k, v = np.repeat(k, G, axis=-3), np.repeat(v, G, axis=-3)
    S = _scores(q, k, s, shift)
    seen = np.isfinite(L)
    L0 = np.where(seen, L, 0.0)
    P = np.where(seen[..., None], np.exp(S - L0[..., None]), 0.0)
    D = (g * O).sum(axis=-1)
    if gl is not None:
        D = D - np.where(seen, _f64(gl), 0.0)
    if kernel_formats:
        D = D.astype(np.float32).astype(np.float64)
    dS = P * (g @ np.swapaxes(v, -1, -2) - D[..., None])
    if kernel_formats:
        P, dS = _bf16(P), _bf16(dS)
    out = (s * (dS @ k), _group_sum(s * (np.swapaxes(dS, -1, -2) @ q), hkv), _group_sum(np.swapaxes(P, -1, -2) @ g, hkv))
    if sink is None:
        return out
    sk = np.broadcast_to(_f64(sink)[:, None], L.shape)
    with np.errstate(invalid="ignore"):
        ps = np.where(np.isfinite(sk) & seen, np.exp(sk - L0), 0.0)
    rows = tuple(a for a in range(L.ndim) if a != L.ndim - 2)
    return out + ((-ps * D).sum(axis=rows),)


def attention(q, k, v, g, gl, s, shift=None, sink=None):
    """The exact float64 O, L, dQ, dK, dV (, dsink) of a loss with dO = g and dL = gl."""
    O, L = forward(q, k, v, s, shift, sink)
    return (O, L) + flow(q, k, v, g, gl, s, shift, O, L, sink)


def merge_forward(Os, Ls):
    """float64 O, L of the merge of the parts (arrays or tensors; Os [n][..., d], Ls [n][...])."""
    Ls = np.stack([_f64(l) for l in Ls])
    m = Ls.max(axis=0)
    m0 = np.where(np.isfinite(m), m, 0.0)
    w = np.exp(Ls - m0)                                   # exp(-inf) = 0: absent parts
    tot = w.sum(axis=0)
    with np.errstate(divide="ignore"):
        L = np.where(tot > 0, m0 + np.log(np.where(tot > 0, tot, 1.0)), -np.inf)
    O = 0.0
    for wi, o in zip(w, Os):
        O = O + np.where((wi > 0)[..., None], wi[..., None] * np.where((wi > 0)[..., None], _f64(o), 0.0), 0.0)
    return O / np.where(tot > 0, tot, 1.0)[..., None], L


def merge_weights(Ls, L):
    """float64 w_i = exp(L_i - L) [n][...], 0 where L_i (or L) is -inf."""
    L = _f64(L)
    ok = np.isfinite(L)
    out = []
    for l in Ls:
        l = _f64(l)
        has = np.isfinite(l) & ok
        out.append(np.where(has, np.exp(np.where(has, l, 0.0) - np.where(ok, L, 0.0)), 0.0))
    return np.stack(out)


def merge_backward(Os, Ls, O, L, dO, dL=None):
    """float64 [dO_i], [dL_i] and, per part, A_i = rowsum(|dO| |O_i - O|) (what the rounding bound of dL_i is made of)."""
    O, dO = _f64(O), _f64(dO)
    gl = 0.0 if dL is None else _f64(dL)
    w = merge_weights(Ls, L)
    dOs, dLs, As = [], [], []
    for wi, o in zip(w, Os):
        has = wi > 0
        diff = np.where(has[..., None], _f64(o), 0.0) - O
        dOs.append(wi[..., None] * dO)
        dLs.append(np.where(has, wi * (gl + (dO * diff).sum(axis=-1)), 0.0))
        As.append(np.where(has, (np.abs(dO) * np.abs(diff)).sum(axis=-1), 0.0))
    return dOs, dLs, As


# ------------------------------------------------------------------------------------------------ the end-to-end cases
# attention_segments: Q [B, H, N_q, d] over key segments of the given lengths.  The causal mask lives in the last segment, which
# must hold at least N_q keys: N_q is the last segment's length where that is shorter than 256, 256 otherwise.
E2E_B, E2E_H = 2, 4
E2E_SPLITS = ((300, 70), (256, 256, 256), (33,) * 8)
E2E_REGIMES = ("default", "scale-one")


# Cases (regime, split, H_kv, d, causal) left out of the gradient gates against the exact gradient: composite_emulation, the
# formats alone, exceeds 2.5e-3 there (the worst figure beside each; tests/test_lse_reference.py asserts that it does), so the
# kernels would be left less than half of the 5e-3 gate.  Their O, L and the cross-check against attention_qk still run.
E2E_DROPPED = {("default", (256, 256, 256), 2, 128, True): 2.501e-3, ("scale-one", (300, 70), 2, 128, True): 2.510e-3,
               ("default", (256, 256, 256), 1, 128, True): 2.529e-3, ("scale-one", (300, 70), 2, 64, False): 2.534e-3,
               ("default", (256, 256, 256), 4, 128, True): 2.535e-3, ("scale-one", (300, 70), 4, 64, False): 2.576e-3}


def e2e_cases():
    import itertools
    return [c for c in itertools.product(E2E_REGIMES, E2E_SPLITS, (4, 2, 1), (64, 128), (False, True))]


def e2e_nq(split):
    return min(split[-1], 256)


def e2e_inputs(regime, split, hkv, d):
    """Host bf16 Q [B, H, N_q, d], K, V [B, H_kv, sum(split), d], dO like Q, and the softmax scale.  `default`: uniform +-0.5, dO
    +-0.2, scale d^-1/2 (tests/test_gpu_qk.py's inputs); `scale-one`: regimes.inputs per batch entry."""
    import torch
    import regimes as R
    nq, nk = e2e_nq(split), sum(split)
    seed = 7300 + 31 * len(split) + 5 * hkv + d
    if regime == "default":
        g = torch.Generator().manual_seed(seed)
        mk = lambda h, n, sc: ((torch.rand(E2E_B, h, n, d, generator=g) - 0.5) * sc).bfloat16()
        return mk(E2E_H, nq, 1.0), mk(hkv, nk, 1.0), mk(hkv, nk, 1.0), mk(E2E_H, nq, 0.4), 1.0 / d ** 0.5
    parts = [R.inputs(regime, nq, nk, E2E_H, hkv, d, seed + 17 * b) for b in range(E2E_B)]
    return tuple(torch.stack([p[j] for p in parts]) for j in range(4)) + (parts[0][4],)


def segment_bounds(split):
    c = np.concatenate([[0], np.cumsum(split)])
    return list(zip(c[:-1].tolist(), c[1:].tolist()))


def composite_emulation(Q, K, V, dO, s, causal, split):
    """The data flow of attention_segments on the CPU, in regimes.emulate's convention extended to the composite route: every
    segment's float64 forward rounded to a bf16 O_i and an fp32 L_i, the merge rounded to a bf16 O and an fp32 L, the merge's
    backward rounded to bf16 dO_i and fp32 dL_i, every segment's backward by flow(kernel_formats=True) -- D' in fp32, P and dS in
    bf16 -- and, as in regimes.emulate, the resulting gradients left in float64 (dQ summed over the segments)."""
    nq, nk = Q.shape[-2], K.shape[-2]
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    bounds = segment_bounds(split)
    shifts = [None] * len(bounds)
    if causal:
        shifts[-1] = nk - nq - bounds[-1][0]
    Os, Ls = [], []
    for (c0, c1), sh in zip(bounds, shifts):
        O, L = forward(Q, K[..., c0:c1, :], V[..., c0:c1, :], s, sh)
        Os.append(_bf16(O)); Ls.append(f32(L))
    O, L = merge_forward(Os, Ls)
    O, L = _bf16(O), f32(L)
    dOs, dLs, _ = merge_backward(Os, Ls, O, L, _f64(dO))
    dQ, dK, dV = 0.0, [], []
    for (c0, c1), sh, Oi, Li, gi, gli in zip(bounds, shifts, Os, Ls, dOs, dLs):
        a, b, c = flow(Q, K[..., c0:c1, :], V[..., c0:c1, :], _bf16(gi), f32(gli), s, sh, Oi, Li, kernel_formats=True)
        dQ = dQ + a
        dK.append(b); dV.append(c)
    return O, L, dQ, np.concatenate(dK, axis=-2), np.concatenate(dV, axis=-2)
