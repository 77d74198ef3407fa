"""Inputs, a float64 reference, a CPU model of the data flow and a per-row gate for the fp8 (e4m3) forward (a helper module, no
tests: tests/test_fp8_reference.py certifies what is here on the CPU, tests/test_gpu_fp8_rows.py runs the kernel on it).

THE REGIMES (inputs()).  U is uniform on [0, 1), d = 128; the amplitude a = sqrt(12 sigma / (s sqrt(d))) gives the scaled scores
s q.k a standard deviation of about sigma whatever the scale s is (tests/regimes.py).  Q, K = (U - 1/2) a, V = (U - 1/2) + vbar,
rounded to e4m3 before anything else is derived from them.  Every (batch, head) draws from a generator of its own, so a row
block computed for the wrong head is wrong on every row, and head (0, 0) of any problem is the one-head problem of the same seed.

    regime          s        sigma  vbar
    flat            d^-1/2   0.08   0     what every other fp8 test runs
    scale-one       1.0      1.5    0
    scale-small     2^-5     1.5    0
    peaked          d^-1/2   4      0
    offsets         1.0      1.5    0.5   O is not about 0
    peaked-offsets  d^-1/2   4      0.5

(`flat` is not paired with a mean in V: nearly identical p values round the same way, the rounding errors add up coherently
along v-bar instead of as a root-sum-square, and the data flow alone takes 0.76 of the gate at 577 keys and 0.71 at 1100 --
no room left under the CPU file's 0.75.)

THE GATE (row_gate()).  The kernel rounds p = exp(S - reference) to e4m3 for the second product, takes the row sum l from the
unrounded fp32 p and writes O in bf16.  Per row i, in 2-norms over d, with P = softmax, max_i the row maximum, l_i = sum_j
exp(S_ij - max_i) >= 1:

    delta_ij = max(2^-4 P_ij, 2^-10 / l_i)                   on the visible keys
    F_i      = visible keys with exp(S_ij - max_i) < 2^-10
    gate_i   = 2 sqrt(sum_j delta_ij^2 |v_j|^2)  +  sum_{j in F_i} P_ij |v_j|  +  2^-8 |O_i|

  * delta: e4m3 rounds to nearest with 3 mantissa bits -- a relative error of at most 2^-4; below 2^-6 its spacing is 2^-9 -- an
    absolute error of at most 2^-10 of p, which is at most 2^-10 / l_i of P (the reference is <= max_i, so p >= exp(S - max_i)).
  * F_i: e4m3 has nothing between 0 and 2^-9, so p <= 2^-10 becomes 0.  The lazy reference of a row is a maximum the row has seen
    (<= max_i) that no score exceeds by more than kFwdRescaleThr = 6 (>= max_i - 6): whichever it is, only keys of F_i can be
    flushed.  The loss is one-sided (it never cancels), so it is counted linearly.
  * 2^-8 |O_i|: the bf16 output.
  * the factor 2: the first term is the root-sum-square of the rounding errors.  For a row with at most four visible keys it is
    the worst case (Cauchy-Schwarz: sum_j delta_j |v_j| <= sqrt(4) sqrt(sum ...)); beyond that about five times the expectation.
Nothing in it comes from the kernel under test.  With per-tensor descales everything is fed the DESCALED values.

L (l_gate()): from unrounded fp32 sums, so the project's two figures of tests/test_gpu_fp8.py hold per row: |dL| <= 1e-4 on a head
whose visible scaled scores all lie within +-8, 1e-3 otherwise (the 64-deep fp8 MFMA dot product is not an exact fp32 sum:
relative ~1e-5 of the score).  A key dropped or admitted wrongly by a mask moves L by about 1 / N: L is the
sharp detector of mask edges.  A row without a visible key has O = 0 and L = -inf exactly (include/fa2_mi355x.h).

emulate(): the kernel's data flow on the CPU, at ONE reference max_i - offset for the whole row; offset in [0, 6] spans the
references the lazy softmax may hold at the end.  (Keys met under an older, lower reference were rounded at finer absolute
spacing and with fewer flushes: inside what the gate admits.)  flow() is its body, open to the mutants of the CPU file."""
import functools

import numpy as np
import torch

D = 128
REGIMES = ("flat", "scale-one", "scale-small", "peaked", "offsets", "peaked-offsets")
#                 s (None: d^-1/2), sigma, vbar
_TABLE = {"flat": (None, 0.08, 0.0), "scale-one": (1.0, 1.5, 0.0), "scale-small": (2.0 ** -5, 1.5, 0.0), "peaked": (None, 4.0, 0.0),
          "offsets": (1.0, 1.5, 0.5), "peaked-offsets": (None, 4.0, 0.5)}
OFFSETS = (0.0, 1.5, 3.0, 4.5, 6.0)          # what the CPU file runs emulate() at
RESCALE_THR = 6.0                            # kFwdRescaleThr (fa2_fwd_softmax.h)
E4M3_MAX = 448.0
FLUSH = 2.0 ** -10                           # e4m3: p <= 2^-10 rounds to 0
L_GATE_SMALL, L_GATE_LARGE, L_SCORE_BOUND = 1e-4, 1e-3, 8.0
SPIKE_SCORE = 28.0


def scale_of(regime):
    s = _TABLE[regime][0]
    return D ** -0.5 if s is None else s


def e4m3(x):
    """x (array or tensor, any float type) rounded to e4m3 (round to nearest even, subnormals down to 2^-9): a host fp8 tensor."""
    t = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
    return t.float().to(torch.float8_e4m3fn)


def f64(t):
    if not isinstance(t, torch.Tensor):
        return np.asarray(t, dtype=np.float64)
    return (t.float() if t.dtype == torch.float8_e4m3fn else t).double().numpy()      # (fp8 -> fp32 is exact, and the fast cast)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().double().numpy()


# ------------------------------------------------------------------------------------------------ the inputs
def head_seed(seed, B, H, b, h):
    return seed + 7919 * (b * H + h)


def values(regime, B, H, N, seed):
    """Unrounded float64 Q, K, V [B, H, N, 128] of a regime and its scale: every (b, h) from its own generator."""
    _, sigma, vbar = _TABLE[regime]
    s = scale_of(regime)
    a = (12.0 * sigma / (s * D ** 0.5)) ** 0.5
    Q, K, V = (torch.empty(B, H, N, D, dtype=torch.float64) for _ in range(3))
    for b in range(B):
        for h in range(H):
            gen = torch.Generator().manual_seed(head_seed(seed, B, H, b, h))
            u = lambda: torch.rand(N, D, generator=gen, dtype=torch.float64) - 0.5
            Q[b, h], K[b, h], V[b, h] = u() * a, u() * a, u() + vbar
    return Q, K, V, s


def inputs(regime, B, H, N, seed):
    """Host e4m3 Q, K, V [B, H, N, 128] and the softmax scale s of a regime (the module's docstring)."""
    Q, K, V, s = values(regime, B, H, N, seed)
    return e4m3(Q), e4m3(K), e4m3(V), s


def scaled_inputs(regime, B, H, N, seed):
    """The regime's tensors as an fp8 producer that uses e4m3's range stores them: x / descale with descale = max|x| / 400 (an fp32
    number), rounded to e4m3.  -> Q8, K8, V8, (q, k, v descales), s."""
    *X, s = values(regime, B, H, N, seed)
    desc = tuple(float(np.float32(float(x.abs().max()) / 400.0)) for x in X)
    return tuple(e4m3(x / c) for x, c in zip(X, desc)) + (desc, s)


def _bh(head):
    return (0, head) if isinstance(head, int) else tuple(head)


def spike(K, Q, s, head, row, key, score=SPIKE_SCORE):
    """K with K[head, key] = q_row score / (s |q_row|^2), rounded to e4m3: `row` scores `score` natural units on `key`
    (tests/regimes.py's construction).  head: h (batch 0) or (b, h)."""
    b, h = _bh(head)
    q = Q[b, h, row].float().double()
    out = K.float().double()
    out[b, h, key] = q * (score / (s * float(q @ q)))
    return e4m3(out)


def loud_row(Q, head, row, factor):
    """Q with one query row multiplied by `factor` (a power of two: exact while it stays in e4m3's range)."""
    b, h = _bh(head)
    out = Q.float().double()
    out[b, h, row] *= factor
    return e4m3(out)


def heavy_quiet_key(K, head, key):
    """K with one key of large norm (4 in every component: |k| = 45) whose scores stay small: the signs are the key's own, unrelated to
    any query (tests/test_gpu_fp8.py, the outlier-round case)."""
    b, h = _bh(head)
    out = K.float().double()
    sign = torch.sign(out[b, h, key])
    out[b, h, key] = torch.where(sign == 0, torch.ones_like(sign), sign) * 4.0
    return e4m3(out)


# ------------------------------------------------------------------------------------------------ the float64 reference
def scores(Q, K, s, causal):
    """float64 s Q K^T [..., N, N]; -inf where the causal mask hides the key."""
    q, k = f64(Q), f64(K)
    S = s * (q @ np.swapaxes(k, -1, -2))
    if causal:
        n = S.shape[-1]
        S = np.where(np.arange(n)[None, :] <= np.arange(n)[:, None], S, -np.inf)
    return S


def reference(Q, K, V, s, causal):
    """float64 attention of the given (already rounded) values.  -> dict: O [..., N, d], L, P, S (-inf on hidden keys), m (row
    maxima), l = sum exp(S - m), seen (rows with a visible key; elsewhere O = 0, L = -inf, P = 0)."""
    S = scores(Q, K, s, causal)
    m = S.max(axis=-1, initial=-np.inf)
    seen = np.isfinite(m)
    p = np.exp(S - np.where(seen, m, 0.0)[..., None])
    l = p.sum(axis=-1)
    with np.errstate(divide="ignore"):
        L = np.where(seen, m + np.log(np.where(seen, l, 1.0)), -np.inf)
    P = p / np.where(seen, l, 1.0)[..., None]
    return dict(O=P @ f64(V), L=L, P=P, S=S, m=m, l=l, seen=seen)


# ------------------------------------------------------------------------------------------------ the kernel's data flow
def flow(S, V, m_ref, edit=None):
    """The kernel's arithmetic at the per-row reference m_ref: p = exp(S - m_ref), l = sum p (unrounded), P8 = p saturated at 448
    and rounded to e4m3, O = bf16((P8 V) / l), L = m_ref + log l.  edit(P8, p) -> P8: where a mutant alters the second product."""
    p = np.exp(S - m_ref[..., None])
    l = p.sum(axis=-1)
    p8 = f64(e4m3(np.minimum(p, E4M3_MAX)))
    if edit is not None:
        p8 = edit(p8, p)
    return _bf16((p8 @ f64(V)) / l[..., None]), m_ref + np.log(l)


def emulate(Q, K, V, s, causal, offset):
    """flow() at the reference row maximum - offset (offset in [0, 6]).  -> O (bf16 values as float64), L."""
    assert 0.0 <= offset <= RESCALE_THR
    S = scores(Q, K, s, causal)
    return flow(S, V, S.max(axis=-1) - offset)


# ------------------------------------------------------------------------------------------------ the gates
def row_gate(ref, V):
    """The per-row bound on |O - ref O| (2-norm over d) of the module's docstring, [..., N]."""
    vn = np.linalg.norm(f64(V), axis=-1)[..., None, :]                 # |v_j| along the key axis
    visible = np.isfinite(ref["S"])
    l = np.where(ref["seen"], ref["l"], 1.0)[..., None]
    delta = np.where(visible, np.maximum(ref["P"] / 16.0, FLUSH / l), 0.0)
    quad = 2.0 * np.sqrt(((delta * vn) ** 2).sum(axis=-1))
    with np.errstate(invalid="ignore"):
        flushed = visible & (np.exp(ref["S"] - np.where(ref["seen"], ref["m"], 0.0)[..., None]) < FLUSH)
    lin = np.where(flushed, ref["P"] * vn, 0.0).sum(axis=-1)
    return quad + lin + np.linalg.norm(ref["O"], axis=-1) / 256.0


def l_gate(ref):
    """[..., 1] per head: 1e-4 where every visible scaled score of the head lies within +-8, else 1e-3."""
    S = np.where(np.isfinite(ref["S"]), np.abs(ref["S"]), 0.0)
    return np.where(S.max(axis=(-1, -2)) <= L_SCORE_BOUND, L_GATE_SMALL, L_GATE_LARGE)[..., None]


def row_errors(O, L, ref):
    """(|O - ref O| per row, |L - ref L| per row) of a result; rows without a visible key must hold O = 0 and L = -inf exactly
    (their errors are 0 if they do and +inf if not)."""
    O, L = f64(O), f64(L)
    seen = ref["seen"]
    eo = np.linalg.norm(O - ref["O"], axis=-1)
    with np.errstate(invalid="ignore"):
        el = np.abs(L - ref["L"])
    empty_ok = (np.abs(O).max(axis=-1) == 0.0) & np.isneginf(L)
    eo = np.where(seen, eo, np.where(empty_ok, 0.0, np.inf))
    el = np.where(seen, el, np.where(empty_ok, 0.0, np.inf))
    return eo, el


# ------------------------------------------------------------------------------------------------ what the GPU file runs
EDGE_N = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 511, 512, 513, 575, 577, 641)
EDGE_REGIMES = ("flat", "offsets")
ORDER_N, ORDER_REGIME = 520, "scale-one"
ORDER_BH = ((1, 8), (1, 16), (1, 24), (2, 4), (2, 8), (3, 8), (1, 9), (1, 17))
REGIME_N, REGIME_H = (577, 1100), 3
ROUND_N, ROUND_H, ROUND_REGIME = 1600, 3, "flat"
ROUND_SPIKE_KEYS = (511, 512, 1023, 1024, 1535, 1536)      # the last and the first key of each 512-key round
ROUND_QUIET_KEYS = (512, 1023)
ROUND_LOUD_ROWS = (1568, 1599)                              # lanes 0 and 31 of the last wave
DESCALE_N, DESCALE_H, DESCALE_REGIMES = 577, 2, ("scale-one", "offsets")
POW2_DESCALES = (2.0 ** -3, 2.0 ** 2, 2.0 ** -1)
WORKSPACE_NS, WORKSPACE_H, WORKSPACE_REGIME = (577, 130, 577), 2, "offsets"
GUARD_NS, GUARD_H, GUARD_REGIME = (33, 257, 577), 2, "offsets"
GUARD_BYTES = 4096


def seed_of(regime, N):
    return 57000 + 1013 * REGIMES.index(regime) + 5 * N


@functools.lru_cache(maxsize=4)
def case_inputs(regime, B, H, N):
    """The e4m3 tensors of a plain case (the same data wherever the case appears) and its scale."""
    return inputs(regime, B, H, N, seed_of(regime, N))


@functools.lru_cache(maxsize=1)
def round_edge_inputs():
    """Case (d): N = 1600 (three full rounds of 512 keys), three heads of `flat`.  Head 0: rows N-1-i each get a 28-unit spike on
    the i-th of the round-edge keys (under the causal mask those rows see all six, and their wave runs the three rounds as full
    rounds).  Head 1: heavy quiet keys on 512 and 1023.  Head 2: rows 1568 and 1599 sixteen times as loud."""
    N = ROUND_N
    Q, K, V, s = case_inputs(ROUND_REGIME, 1, ROUND_H, N)
    for i, key in enumerate(ROUND_SPIKE_KEYS):
        K = spike(K, Q, s, 0, N - 1 - i, key)
    for key in ROUND_QUIET_KEYS:
        K = heavy_quiet_key(K, 1, key)
    for row in ROUND_LOUD_ROWS:
        Q = loud_row(Q, 2, row, 16.0)
    return Q, K, V, s


@functools.lru_cache(maxsize=2)
def descaled_case(regime):
    """Case (e): stored tensors, descales, scale, and the descaled values (float64) the reference is fed."""
    Q8, K8, V8, desc, s = scaled_inputs(regime, 1, DESCALE_H, DESCALE_N, seed_of(regime, DESCALE_N))
    return (Q8, K8, V8), desc, s, tuple(f64(t) * c for t, c in zip((Q8, K8, V8), desc))


def cpu_cases():
    """Every (label, Q, K, V, s) -- one head each, as float64 values or e4m3 tensors [N, 128] -- whose (regime, N) the GPU file
    hands the kernel; tests/test_fp8_reference.py runs both masks on each."""
    seen = set()
    for regime, N in ([(r, n) for r in EDGE_REGIMES for n in EDGE_N] + [(ORDER_REGIME, ORDER_N)]
                      + [(r, n) for r in REGIMES for n in REGIME_N]
                      + [(WORKSPACE_REGIME, n) for n in WORKSPACE_NS] + [(GUARD_REGIME, n) for n in GUARD_NS]):
        if (regime, N) in seen:
            continue
        seen.add((regime, N))
        Q, K, V, s = case_inputs(regime, 1, 1, N)
        yield f"{regime}-{N}", Q[0, 0], K[0, 0], V[0, 0], s
    Q, K, V, s = round_edge_inputs()
    for h, what in enumerate(("spikes", "quiet-keys", "loud-rows")):
        yield f"round-edges-{what}-{ROUND_N}", Q[0, h], K[0, h], V[0, h], s
    for regime in DESCALE_REGIMES:
        _, _, s, (q, k, v) = descaled_case(regime)
        yield f"descaled-{regime}-{DESCALE_N}", q[0, 0], k[0, 0], v[0, 0], s
