"""The float64 reference for attention with sinks (a helper module, no tests: tests/test_sink_reference.py pins it to
regimes.ref_attention on the CPU, tests/test_gpu_sink.py runs the kernels against it).

THE RULES (include/fa2_mi355x.h, fa2_forward_sink).  sink[h] is one logit per query head, in natural units (NOT multiplied by the
softmax scale), that joins every row's softmax and carries no value.  With S_ij = scale q_i . k_j over the keys visible to row i:

    L_i = log(exp(s_h) + sum_j exp S_ij)      P_ij = exp(S_ij - L_i)      O_i = sum_j P_ij v_j      P_sink,i = exp(s_h - L_i)

Backward under dO = g: D_i = rowsum(g_i o O_i) as always (the sink's value is 0, so dP_sink = 0), dS_ij = P_ij (g_i . v_j - D_i),
dQ = scale dS k, dK = scale dS^T q, dV = P^T g, and dsink[h] = sum over the batch and the rows of dS_sink = - sum P_sink D.
sink[h] = -inf: no sink for the head (plain attention, dsink[h] = 0).  A row that sees no key has O = 0, dQ = 0, D = 0 and
L = s_h (-inf only if s_h = -inf); it adds nothing to dsink."""
import numpy as np


def ref_attention_sink(q, k, v, g, scale, causal, sink):
    """float64 O, L, dQ, dK, dV, dsink and a dict of magnitudes.  q, g [..., H, Nq, d]; k, v [..., H, Nk, d] (the same leading
    dimensions: K and V already repeated per group); sink [H]; bottom-right causal mask; Nq or Nk may be 0.
    The magnitudes, per head (what the rounding bounds of tests/test_gpu_sink.py are made of):
        M  = sum_rows P_sink sum_c |g_c O_c|                                  the terms D sums, weighted as dsink weights them
        A  = sum_rows P_sink sum_c |g_c| (sum_j P_j |v_jc| + |O_c|)           what rounding P and O to bf16 moves them by, at most
        PD = sum_rows P_sink |D|                                              the terms dsink sums"""
    q, k, v, g = (np.asarray(t, dtype=np.float64) for t in (q, k, v, g))
    sink = np.asarray(sink, dtype=np.float64)
    nq, nk = q.shape[-2], k.shape[-2]
    assert sink.shape == (q.shape[-3],)
    s = scale * (q @ np.swapaxes(k, -1, -2))
    if causal:
        i, j = np.arange(nq)[:, None], np.arange(nk)[None, :]
        s = np.where(j <= i + (nk - nq), s, -np.inf)
    sk = np.broadcast_to(sink[:, None], q.shape[:-1])                # [..., H, Nq]: the row's sink
    m = np.maximum(s.max(axis=-1, initial=-np.inf), sk)
    seen = np.isfinite(m)                                            # false: no key and no sink
    m0 = np.where(seen, m, 0.0)
    p, ps = np.exp(s - m0[..., None]), np.exp(sk - m0)               # exp(-inf) = 0: masked keys, absent sinks
    l = np.where(seen, p.sum(axis=-1) + ps, 1.0)
    L = np.where(seen, m0 + np.log(l), -np.inf)
    P, Ps = p / l[..., None], ps / l
    O = P @ v
    D = (g * O).sum(axis=-1)
    dS = P * (g @ np.swapaxes(v, -1, -2) - D[..., None])
    dQ, dK, dV = scale * (dS @ k), scale * (np.swapaxes(dS, -1, -2) @ q), np.swapaxes(P, -1, -2) @ g
    rows = tuple(a for a in range(Ps.ndim) if a != Ps.ndim - 2)      # everything but the head axis
    per_head = lambda x: x.sum(axis=rows)
    mag = {"M": per_head(Ps * (np.abs(g) * np.abs(O)).sum(axis=-1)),
           "A": per_head(Ps * (np.abs(g) * (P @ np.abs(v) + np.abs(O))).sum(axis=-1)),
           "PD": per_head(Ps * np.abs(D))}
    return O, L, dQ, dK, dV, per_head(-Ps * D), mag


def dsink_from_kernel_feed(sink, L32, O16, g):
    """float64 -sum exp(s - L) rowsum(g o O) per head from the arrays the sink-gradient kernel is fed: the fp32 L and the bf16 O
    of a forward ([..., H, Nq] and [..., H, Nq, d]) and dO.  Rows with L = -inf (no key, no sink) add nothing."""
    sink, L, O, g = (np.asarray(t, dtype=np.float64) for t in (sink, L32, O16, g))
    sk = np.broadcast_to(sink[:, None], L.shape)
    with np.errstate(invalid="ignore"):
        ps = np.where(np.isfinite(sk), np.exp(sk - np.where(np.isfinite(L), L, 0.0)), 0.0)
    rows = tuple(a for a in range(L.ndim) if a != L.ndim - 2)
    return (-ps * (g * O).sum(axis=-1)).sum(axis=rows)
