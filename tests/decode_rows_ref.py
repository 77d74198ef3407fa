"""The per-row gate of O for the cache-side attention family -- the split-KV decode (contiguous, paged, e4m3, windowed), extend and
ragged extend (a helper module, no tests: tests/test_decode_rows_reference.py certifies what is here on the CPU, the family's GPU
files and tests/test_gpu_decode_rows.py hold the kernels to it).

WHY.  decode_ref.errors takes the rel-L2 of O over a whole batch whose sequences have 0 to 2500 keys.  |O| of a sequence of n
keys is about |v| / sqrt(n), so the longest sequences carry almost none of the norm (0.07 % to 0.12 % of it in decode_ref.CASES[2],
[5] and [9]) and a fault on their P V side alone passes (DESIGN.md section 6d has the table).  L was gated per row already.

THE GATE.  2-norms over d; u = U = 2^-9, bf16's unit round-off; P_ij = exp(S_ij - L_i) the final probabilities, L_i including
the sink:

    O row i :  KAPPA u sqrt( sum_j P_ij^2 |v_j|^2 )  +  u |O_i|

the first line of tests/bf16_rows_ref.py's table.  First term: the kernels round P to bf16 for the second product, once per
(row, key); the roundings are independent and add in quadrature.  Second term: the one bf16 rounding of the output.  Nothing
else counts at this scale: a tile's second product accumulates in fp32 inside the matrix instruction (32 keys, relative 2^-24
each); a wave rescales its o by alpha once per tile, at most 20 times in a 2500-key sequence over 1 split, and the four waves, the
splits of the combine kernel (at most 64 here) and the sink's weight are one fp32 multiply-add each per element -- a chain of at
most 32 + 20 + 4 + 64 + 1 = 121 fp32 roundings of 2^-24 against the one bf16 rounding of 2^-9 = 2^15 of them, 0.4 % of the second term
in the worst case and about sqrt(121) / 2^15 = 0.03 % of it for independent roundings.
  * e4m3 caches: the gate is taken on the DEQUANTISED caches, as the references are; v_descale is an fp32 factor on the fp32 o.
  * a keyless row (no visible key; with a sink L = sink[h]): P = 0, O_ref = 0, the gate is 0 and O must be exactly 0.
  * merge_states_forward over two calls' bf16 O (test_a_cache_in_two_allocations_is_two_calls_and_a_merge): each partial was
    rounded to bf16 before the merge weighs it, so that gate gets u (w_a |O_a,i| + w_b |O_b,i|) on top (merged_extra), from the
    reference partials and their weights w = exp(L_part - L).
Everything in a gate comes from the float64 reference on the bf16 (or dequantised) inputs; nothing comes from a kernel.

Ref: what the family's cached references return -- the (O, L) pair they always were, with .quad = sqrt(sum_j P_ij^2 |v_j|^2) per
row beside it, so a reference and its gate are computed once and cached together (one more score matrix per reference), however
many split counts, layouts and cache kinds are checked against it.

KAPPA = 1.5: the project's rule -- the smallest multiple of 0.5 at which the CPU emulations (decode_ref.emulate,
decode_window_ref.emulate, on dequantised caches for e4m3) use at most ROOM = 0.75 of the gate on every row of every certified
case; the bound is 4.  Largest row ratios of the emulation per family at KAPPA (tests/test_decode_rows_reference.py prints them):
    decode 0.59   e4m3 decode 0.61   windowed 0.58   extend 0.62   ragged extend 0.63   the regime runs 0.62
at 1.0 they are 0.76, 0.76, 0.73, 0.78, 0.79 and 0.78; at 2.0 at most 0.54.  It comes from the emulation and the float64 reference, never from a kernel's output."""
import numpy as np
import torch

U =2.0 ** -9          # bf16's unit round-off
KAPPA = 1.5
ROOM = 0.75            # what the emulation may use of a gate
KAPPA_BOUND = 4.0


class Ref(tuple):
    """(O, L) of a float64 reference, with .quad [rows of L] beside it."""

    def __new__(cls, O, L, quad):
        self = super().__new__(cls, (O, L))
        self.quad = quad
        return self

    def head(self, n):
        """The first n rows of the leading axis (the owned tokens of a token-major reference)."""
        return Ref(self[0][:n], self[1][:n], self.quad[:n])


def quad64(Q, K, V, lens, scale, causal, sink, wl=None):
    """sqrt(sum_j P_ij^2 |v_j|^2) [B, hq, nq] in float64 on contiguous host caches: Q [B, hq, nq, d], K, V [B, hkv, ncap, d] of which
    sequence b uses lens[b] rows; the bottom-right causal mask if `causal`, the window wl beside it (None: none); sink fp32 [hq] or
    None.  P = exp(S - L) with L over the visible keys and the sink."""
    B, hq, nq, d = Q.shape
    G = hq // K.shape[1]
    out = np.zeros((B, hq, nq))
    sk = None if sink is None else np.broadcast_to(sink.double().numpy()[:, None], (hq, nq))
    Q32, K32, V32 = (t.float().numpy() for t in (Q, K, V))      # (exact; one conversion each: torch's per-call cost is the reference's largest)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b, n in enumerate(lens):
            n = int(n)
            if n <= 0:
                continue
            q = Q32[b].astype(np.float64)
            k = np.repeat(K32[b, :, :n].astype(np.float64), G, axis=0)
            v2 = np.repeat((V32[b, :, :n].astype(np.float64) ** 2).sum(axis=-1), G, axis=0)
            s = scale * (q @ np.swapaxes(k, -1, -2))
            pos, j = (np.arange(nq) + n - nq)[:, None], np.arange(n)[None, :]
            vis = np.ones((nq, n), dtype=bool)
            if causal:
                vis &= j <= pos
            if wl is not None:
                vis &= j >= pos - wl
            s = np.where(vis, s, -np.inf)
            m = s.max(axis=-1, initial=-np.inf)
            if sk is not None:
                m = np.maximum(m, sk)
            seen = np.isfinite(m)
            m0 = np.where(seen, m, 0.0)
            p = np.exp(s - m0[..., None])
            l = p.sum(axis=-1) + (0.0 if sk is None else np.exp(sk - m0))
            P = p / np.where(seen, l, 1.0)[..., None]
            out[b] = np.sqrt(((P * P) @ v2[..., None])[..., 0])
    return out


def gate(ref, kappa=KAPPA, extra=None):
    """The row gate of O, ref.quad's shape: kappa u quad + u |O_ref| (+ extra)."""
    out = kappa * U * ref.quad + U * np.linalg.norm(ref[0], axis=-1)
    return out if extra is None else out + extra


def row_errors(O, ref):
    """|O_i - O_ref,i| per row; 0 on the rows no reference exists for (NaN in a ragged reference: tokens no sequence owns)."""
    rO = ref[0]
    e = np.linalg.norm(np.asarray(O, dtype=np.float64) - rO, axis=-1)
    return np.where(np.isnan(rO).any(axis=-1), 0.0, e)


def ratios(O, ref, kappa=KAPPA, extra=None):
    """error / gate per row (0 / 0 = 0: an exact rule that holds; e / 0 = inf)."""
    e = row_errors(O, ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e == 0.0, 0.0, e / np.nan_to_num(gate(ref, kappa, extra), nan=0.0))


def where_of(index, cu=None):
    """'(sequence b, head h, token i)' of a row index -- [B, hq, nq] order, or token-major [T, hq] with the batch's cu."""
    if len(index) == 3:
        return "(sequence %d, head %d, token %d)" % tuple(index)
    t, h = (int(x) for x in index)
    if cu is None:
        return f"(token {t}, head {h})"
    b = max(b for b in range(len(cu) - 1) if cu[b] <= t) if t < cu[-1] else -1
    return f"(sequence {b}, head {h}, token {t - cu[b] if b >= 0 else t})"


def check(where, O, ref, extra=None, cu=None):
    """Asserts |O_i - O_ref,i| <= gate_i on every row; prints and returns the worst ratio with its place."""
    O = O.float().cpu().numpy() if isinstance(O, torch.Tensor) else O
    r = ratios(O, ref, extra=extra)
    worst = np.unravel_index(np.argmax(r), r.shape) if r.size else ()
    top = float(r[worst]) if r.size else 0.0
    print(where, f"O row ratio {top:.3f}" + (f" at {where_of(worst, cu)}" if r.size else ""))
    bad = r > 1.0
    assert not bad.any(), (f"{where}: O row gate missed on {int(bad.sum())} rows, worst {top:.2f} x gate at {where_of(worst, cu)}: error "
                           f"{row_errors(O, ref)[worst]:.3e}")
    return top


def merged_extra(parts, L):
    """u sum_p w_p |O_p,i| for a merge of bf16 partial results: parts = [(O_p, L_p)] float64 references, L the merged reference L."""
    out = 0.0
    with np.errstate(invalid="ignore"):
        for Op, Lp in parts:
            w = np.where(np.isneginf(Lp), 0.0, np.exp(Lp - np.where(np.isneginf(L), 0.0, L)))
            out = out + U * w * np.linalg.norm(Op, axis=-1)
    return out
