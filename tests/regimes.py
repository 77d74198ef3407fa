"""Inputs and float64 references for the bf16 attention tests away from flat softmax and the default scale (a helper module, no
tests: tests/test_regimes_reference.py certifies what is here on the CPU, tests/test_gpu_regimes.py runs the kernels on it).

THE REGIMES (inputs()).  U is uniform on [0, 1); the amplitude a = sqrt(12 sigma / (s sqrt(d))) gives the scaled scores s q.k a
standard deviation of about sigma whatever the scale s is.  Q, K = (U - 1/2) a, V = (U - 1/2) + vbar, dO = 0.4 (U - 1/2) + gbar,
rounded to bf16 before anything else is derived from them.

    regime        s        sigma  vbar  gbar
    scale-one     1.0      1.5    0     0
    scale-small   2^-5     1.5    0     0
    peaked        d^-1/2   4      0     0     L spans about 11 to 19 at 1100 keys
    spikes        d^-1/2   0.08   0     0     two spike keys per chosen head (below)
    offsets       1.0      1.5    0.5   0.1   O is not about 0: D = rowsum(dO o O) is of the size of dP
    lift          d^-1/2   0.08   0     0     the first of the two spike keys only (below)
    low-level     1.0      --     0     0     Q = 3 + 0.25 (U - 1/2), K = -(c + 0.05 (U - 1/2)), c = 0.3 (d = 128) or 0.6 (d = 64):
                                              scores about -115, every finite L below -88, so exp(-L) overflows fp32

SPIKES.  In query head 1 and in the last query head, rows r1 = N_q - 41 and r2 = N_q - 6 (clamped at 0) each get a key of
their own in the K/V head their query head attends: key floor(0.28 N_k) = q_r1 28 / (s |q_r1|^2) and key floor(0.82 N_k) =
q_r2 130 / (s |q_r2|^2) -- scores of 28 and 130 natural units against a background of +-0.25, as in
test_fwd_rounds_without_maxima_late_spikes_and_the_restart (tests/test_gpu_parity.py).  The two heads must attend different
K/V heads (8 query heads on 2, or 3 on 3, do).  spike_rows() says where a spike is visible to its row under the mask; there
the reference has L[r1] > 25 and L[r2] > 120.  At N_k = 1100 the first spike (key 308) lies in a forward tile past the first,
where no lane maxima are taken any more, so the row's sum passes 2^30 and its reference is lifted at the next round start; the
second (key 902) lies in a later round and takes the sum past 2^80: the row block runs again with maxima.  That holds at both
head dims (a round is 256 keys at d = 128 and 512 at d = 64; 1100 is the smallest length with two full rounds at d = 64).
LIFT.  The restart runs the whole row block again with maxima, and r1 and r2 share a row block: in `spikes` at 1100 keys the
lifted sums are thrown away, and a lift that scaled them wrongly would go unseen (tried: a forward whose lift scales by 2^-32
fails `spikes` only at N = 1024, d = 128, causal, where the 130-unit key falls into the diagonal tiles, which keep their
maxima).  The `lift` regime sets the 28-unit key alone: no row sum reaches 2^80 (L < 45 everywhere), nothing restarts, and the
lift at the round start behind key floor(0.28 N_k) -- 1100 keys at both head dims, 600 keys at d = 128 -- is what O and L
come from, on the rectangular and packed routes as well.

REFERENCES.  ref_attention: float64 forward and backward of rectangular attention (bottom-right causal mask, the empty-row
rules of include/fa2_mi355x.h); tests/test_qk_plan.py pins it to the oracle.  ref_grouped: the same with K and V given per
K/V head.  ref_flow: the backward AS THE KERNELS ARE FED -- P = exp(S - L) from a given fp32 L and D = rowsum(dO o O) from a
given bf16 O, everything else float64.  The kernels take D from the bf16 O they are handed; where O is not about 0 (spikes, a
mean in V) the rounding of O alone moves dQ and dK 6e-3 to 9e-3 (rel-L2) away from the exact gradient, above the project's 5e-3
gate, without any kernel being wrong.  ref_flow fed the same two arrays is the reference that isolates the kernels' own error.
emulate: ref_flow with D rounded to fp32 and P and dS rounded to bf16 before the three products -- the kernels' data flow on the
CPU, used only to certify that an input leaves the kernels room under the gate."""
import numpy as np
import torch

REGIMES = ("scale-one", "scale-small", "peaked", "spikes", "offsets", "low-level", "lift")
SPIKED = {"spikes": (0, 1), "lift": (0,)}      # which of the two spike keys a regime sets
#                 s (None: d^-1/2), sigma, vbar, gbar
_TABLE = {"scale-one": (1.0, 1.5, 0.0, 0.0), "scale-small": (2.0 ** -5, 1.5, 0.0, 0.0), "peaked": (None, 4.0, 0.0, 0.0),
          "spikes": (None, 0.08, 0.0, 0.0), "lift": (None, 0.08, 0.0, 0.0), "offsets": (1.0, 1.5, 0.5, 0.1), "low-level": (1.0, None, 0.0, 0.0)}
SPIKE_SCORES = (28.0, 130.0)
SPIKE_L = (25.0, 120.0)                   # what the reference's L exceeds on a row that sees its spike
LOW_LEVEL_L = -88.0                       # every finite L of the low-level regime lies below: exp(-L) overflows fp32


# ------------------------------------------------------------------------------------------------ the float64 reference
def ref_attention(q, k, v, g, scale, causal, want_abs=False):
    """float64 O, L, dQ, dK, dV of softmax(scale q k^T [bottom-right causal]) v and its backward under dO = g.  q, g [..., Nq, d];
    k, v [..., Nk, d] (same leading dimensions); Nq or Nk may be 0.  A row without a visible key: O = 0, L = -inf, dQ = 0.
    want_abs: also the magnitudes of the terms that dQ and dK sum (the same formulas on absolute values)."""
    q, k, v, g = (np.asarray(t, dtype=np.float64) for t in (q, k, v, g))
    nq, nk = q.shape[-2], k.shape[-2]
    s = scale * (q @ np.swapaxes(k, -1, -2))
    if causal:
        i, j = np.arange(nq)[:, None], np.arange(nk)[None, :]
        s = np.where(j <= i + (nk - nq), s, -np.inf)
    m = s.max(axis=-1, initial=-np.inf)
    seen = np.isfinite(m)                                            # rows with a visible key
    p = np.exp(s - np.where(seen, m, 0.0)[..., None])                # exp(-inf) = 0 on masked keys and on rows without any
    l = p.sum(axis=-1)
    with np.errstate(divide="ignore"):
        L = np.where(seen, m + np.log(np.where(seen, l, 1.0)), -np.inf)
    P = p / np.where(seen, l, 1.0)[..., None]
    O = P @ v
    D = (g * O).sum(axis=-1)
    dP = g @ np.swapaxes(v, -1, -2)
    dS = P * (dP - D[..., None])
    dQ, dK, dV = scale * (dS @ k), scale * (np.swapaxes(dS, -1, -2) @ q), np.swapaxes(P, -1, -2) @ g
    if not want_abs:
        return O, L, dQ, dK, dV
    aS = P * (np.abs(g) @ np.swapaxes(np.abs(v), -1, -2) + (np.abs(g) * np.abs(O)).sum(axis=-1)[..., None])
    return (O, L, dQ, dK, dV), (scale * (aS @ np.abs(k)), scale * (np.swapaxes(aS, -1, -2) @ np.abs(q)))


def _group_sum(x, hkv):
    """[..., H_q, N, d] -> [..., H_kv, N, d]: the gradients of a K/V head are the sums over its group's query heads."""
    *lead, hq, n, d = x.shape
    return x.reshape(*lead, hkv, hq // hkv, n, d).sum(axis=-3)


def f64(t):
    return t.double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def ref_grouped(q, k, v, g, s, causal):
    """ref_attention for q, g [H_q, N_q, d] and k, v [H_kv, N_k, d]: K and V repeated per group, dK and dV summed over it."""
    q, k, v, g = (f64(t) for t in (q, k, v, g))
    hq, hkv = q.shape[0], k.shape[0]
    O, L, dQ, dK, dV = ref_attention(q, np.repeat(k, hq // hkv, axis=0), np.repeat(v, hq // hkv, axis=0), g, s, causal)
    return O, L, dQ, _group_sum(dK, hkv), _group_sum(dV, hkv)


def _bf16(x):
    """x rounded to bf16 (round to nearest even), as float64.  An Inf stays one."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().double().numpy()


def _flow(q, k, v, g, s, causal, O16, L32, kernel_formats):
    q, k, v, g, O16, L = (f64(t) for t in (q, k, v, g, O16, L32))
    hq, hkv = q.shape[0], k.shape[0]
    k, v = np.repeat(k, hq // hkv, axis=0), np.repeat(v, hq // hkv, axis=0)
    nq, nk = q.shape[-2], k.shape[-2]
    S = s * (q @ np.swapaxes(k, -1, -2))
    if causal:
        i, j = np.arange(nq)[:, None], np.arange(nk)[None, :]
        S = np.where(j <= i + (nk - nq), S, -np.inf)
    seen = np.isfinite(L)
    P = np.where(seen[..., None], np.exp(S - np.where(seen, L, 0.0)[..., None]), 0.0)
    D = (g * O16).sum(axis=-1)
    if kernel_formats:
        D = D.astype(np.float32).astype(np.float64)
    dS = P * (g @ np.swapaxes(v, -1, -2) - D[..., None])
    if kernel_formats:
        P, dS = _bf16(P), _bf16(dS)
    dQ, dK, dV = s * (dS @ k), s * (np.swapaxes(dS, -1, -2) @ q), np.swapaxes(P, -1, -2) @ g
    return dQ, _group_sum(dK, hkv), _group_sum(dV, hkv)


def ref_flow(q, k, v, g, s, causal, O16, L32):
    """float64 dQ [H_q, N_q, d], dK, dV [H_kv, N_k, d] from the two arrays the backward kernels are handed: P = exp(S - L32)
    (0 on the rows with L = -inf), D = rowsum(g o O16), dS = P (g v^T - D), dQ = s dS k, dK = s dS^T q, dV = P^T g; K and V
    repeated per group, dK and dV summed over each group."""
    return _flow(q, k, v, g, s, causal, O16, L32, False)


def emulate(q, k, v, g, s, causal, O16, L32):
    """ref_flow with D rounded to fp32 and P and dS rounded to bf16 before the three products (CPU only: certifies inputs)."""
    return _flow(q, k, v, g, s, causal, O16, L32, True)


def kernel_feed(O, L):
    """What the backward is handed: the reference's O rounded to bf16 and its L rounded to fp32 (host tensors)."""
    return torch.from_numpy(O).bfloat16(), torch.from_numpy(L).float()


def rel(a, b):
    a = f64(a)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------------ the inputs
def scale_of(regime, d):
    s = _TABLE[regime][0]
    return 1.0 / d ** 0.5 if s is None else s


def spike_rows(nq, nk, hq, causal, which=(0, 1)):
    """[(head, row, key, i)] of the spikes regime, i = 0 for the 28-unit spike and 1 for the 130-unit one (`which`: those wanted),
    with the spikes that the mask hides from their rows left out."""
    if nq < 1 or nk < 1:
        return []
    rows, keys = (max(nq - 41, 0), max(nq - 6, 0)), (int(0.28 * nk), int(0.82 * nk))
    heads = sorted({min(1, hq - 1), hq - 1})
    return [(h, r, j, i) for h in heads for i, (r, j) in enumerate(zip(rows, keys))
            if i in which and (not causal or j <= r + nk - nq)]


def inputs(regime, nq, nk, hq, hkv, d, seed):
    """Host bf16 Q [hq, nq, d], K, V [hkv, nk, d], dO [hq, nq, d] and the softmax scale s of a regime (the module's docstring)."""
    s, sigma, vbar, gbar = _TABLE[regime]
    s = scale_of(regime, d)
    gen = torch.Generator().manual_seed(seed)
    u = lambda h, n: torch.rand(h, n, d, generator=gen, dtype=torch.float64) - 0.5
    uq, uk, uv, ug = u(hq, nq), u(hkv, nk), u(hkv, nk), u(hq, nq)
    if regime == "low-level":
        c = {128: 0.3, 64: 0.6}[d]
        Q, K = 3.0 + 0.25 * uq, -(c + 0.05 * uk)
    else:
        a = (12.0 * sigma / (s * d ** 0.5)) ** 0.5
        Q, K = uq * a, uk * a
    Q, K, V, dO = (t.bfloat16() for t in (Q, K, uv + vbar, 0.4 * ug + gbar))
    if regime in SPIKED:
        G = hq // hkv
        spikes = spike_rows(nq, nk, hq, False, SPIKED[regime])       # the keys are set whether or not a mask will hide them
        assert len({h // G for h, *_ in spikes}) == len({h for h, *_ in spikes})
        K = K.double()
        for h, r, j, i in spikes:
            q = Q[h, r].double()
            K[h // G, j] = q * (SPIKE_SCORES[i] / (s * float(q @ q)))
        K = K.bfloat16()
    return Q, K, V, dO, s


def seed_of(regime, nq, nk, d):
    """One seed per (regime, shape, head_dim): a sequence has the same data wherever it appears, dense or packed."""
    return 91000 + 1009 * REGIMES.index(regime) + 7 * nq + 3 * nk + d


# ------------------------------------------------------------------------------------------------ what the GPU file runs
HEADS_PLAIN, HEADS_GQA = (3, 3), (8, 2)                    # H = 3: the plain block order; 8 query heads on 2 K/V heads
SQUARE_N = (1024, 1100)
QK_SHAPES = ((300, 1100), (1100, 300))
PACKED_ONE = ((1100, 1100), (300, 300), (0, 0), (40, 40))
PACKED_TWO = ((300, 1100), (1100, 600), (40, 0), (0, 40))
STEP_N, STEP_CUTS, STEP_REGIMES = 1100, (0, 300, 1100), ("scale-one", "scale-small", "peaked")


def problems():
    """Every (hq, hkv, nq, nk) that tests/test_gpu_regimes.py hands a kernel as one sequence with at least a row and a key."""
    out = [HEADS_PLAIN + (n, n) for n in SQUARE_N] + [HEADS_GQA + (n, n) for n in SQUARE_N] + [HEADS_GQA + s for s in QK_SHAPES]
    out += [HEADS_GQA + s for s in PACKED_ONE + PACKED_TWO if s[0] and s[1]]
    return tuple(dict.fromkeys(out))


def sequence(regime, hq, hkv, nq, nk, d):
    return inputs(regime, nq, nk, hq, hkv, d, seed_of(regime, nq, nk, d))
