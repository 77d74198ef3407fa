"""The resumable forward step row by row: reference, gates, a CPU model of the carried state and mutants (a helper module, no
tests: tests/test_step_rows_reference.py certifies what is here on the CPU, tests/test_gpu_step_rows.py runs fa2_forward_step,
fa2_forward_step_strided and fa2_forward_state_finalize on it).  DESIGN.md section 6e.

A STEP PROBLEM is a bf16_rows_ref.Case (ungrouped heads, its own mask unused) and a list of SHARDS in the order they are folded
in.  A shard is (rows, keys, shift): the row range [r0, r1) of every head, the key range [k0, k1), and the causal shift of
fa2_forward_step_strided -- local key j is visible to local row i iff j <= i + shift -- or None for every key.  A row outside
the range sees nothing of the shard.
REFERENCE.  One float64 attention over the union of what each row sees across the shards: the score matrix with -inf where every
shard hides a key, then bf16_rows_ref's O gate and L gate on it (Rows below: the formulas of Case._gates, nothing else):
    O row i :  kappa u sqrt(sum_j P_ij^2 |v_j|^2) + u |O_i|,        |dL| <= 1e-4 where |L_ref| <= 25, else 1e-3.
The gate does not change with the number of steps: bf16 rounding of P is relative whatever reference a shard ran at.  What a
step adds is fp32 arithmetic on the carried state: one multiply of each accumulator element and of l by exp(m_old - m_new) per
reference move (at most one per shard on entry, one per lift, one per lazy update), each 2^-24 relative -- with three shards
fewer than ten such factors, 10 x 2^-24 = 6e-7 against u = 2e-3: not counted.
STATE INVARIANTS.  (Oacc, l, M) after a non-final step depend on the references the kernel happened to use, M + ln l and Oacc / l
do not: they are L and O over the keys seen so far (state_views), gated by the reference restricted to those keys.
EMULATION, shard by shard (Step.emulate): the reference of shard k is max(carried m, the shard's row maximum) - offset, offset in
bf16_rows_ref.FWD_OFFSETS; p = exp(S - r) in bf16 for the second product; the accumulator and l carried unrounded (scaled by
exp(m - r)); one bf16 rounding at the end.  A row that sees nothing in a shard keeps its state.
MUTANTS (fault= of Step.emulate), each what one fault would write:
  s1 (head)            the carried accumulator is not rescaled when the reference moves on entry to a resumed shard (l is)
  s2 (head, block)     the restart pass of a 256-row block starts from zero: the earlier shards are lost from O and L
  s3 ()                a row that sees no key in a step loses its carried state
  s4 (head, group)     causal_shift off by one on one 32-row group
  s5 ()                head h of a strided call reads its carried state q_len rows apart, not q_head_stride (head 0 is right)
  s6 (head, group, k)  keys k .. k + 31 of a resumed shard missing from P V alone on one 32-row group"""
import numpy as np

import bf16_rows_ref as B

f64, _bf16 = B.f64, B._bf16


class Rows(B.Case):
    """Reference and gates of a forward over any visibility: S [h, nq, nk] float64 scores with -inf on hidden keys, v [h, nk, d].
    The fields bf16_rows_ref.check reads from a Case, O and L only."""

    def __init__(self, regime, S, v):
        m = S.max(axis=-1, initial=-np.inf)
        seen = np.isfinite(m)
        m0 = np.where(seen, m, 0.0)
        p = np.exp(S - m0[..., None])
        l = np.where(seen, p.sum(axis=-1), 1.0)
        with np.errstate(divide="ignore"):
            L = np.where(seen, m0 + np.log(l), -np.inf)
        O = (p / l[..., None]) @ v
        L32 = L.astype(np.float32).astype(np.float64)
        P = np.where(seen[..., None], np.exp(S - np.where(seen, L32, 0.0)[..., None]), 0.0)
        self.regime, self.ref, self.part, self.keyless = regime, {"O": O, "L": L}, {}, ~seen
        self.quad = {"O": B.U * np.sqrt(np.einsum("hqk,hk->hq", P * P, B._norm(v) ** 2))}
        self.rest = {"O": B.U * B._norm(O)}
        self.l_gate = np.where(np.abs(L) <= B.L_NEAR, B.L_ABS, B.L_ABS_FAR)
        self.key_seen = None


def shard(keys, rows=None, shift=None):
    return (rows, keys, shift)


def state_views(Oacc, l, M):
    """{O, L} of a carried state: Oacc / l and M + ln l (0 and -inf where l = 0: a row that has seen no key)."""
    Oacc, l, M = f64(Oacc), f64(l), f64(M)
    has = l > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"O": np.where(has[..., None], Oacc / np.where(has, l, 1.0)[..., None], 0.0),
                "L": np.where(has, np.where(has, M, 0.0) + np.log(np.where(has, l, 1.0)), -np.inf)}


class Step:
    def __init__(self, case, shards):
        assert case.G == 1
        self.case, self.shards = case, [(rows or (0, case.nq), keys, shift) for rows, keys, shift in shards]
        self.S = case.s * (case.q @ np.swapaxes(case.k, -1, -2))
        self._rows = {}

    def visible(self, sh, shift_fix=None):
        """[nq, nk] bool of one shard; shift_fix = (row slice, delta): the shift moved by delta on those rows (mutant s4)."""
        (r0, r1), (k0, k1), shift = sh
        vis = np.zeros((self.case.nq, self.case.nk), dtype=bool)
        i, j = np.arange(r1 - r0)[:, None], np.arange(k1 - k0)[None, :]
        block = np.ones((r1 - r0, k1 - k0), dtype=bool) if shift is None else j <= i + shift
        if shift_fix is not None and shift is not None:
            rows, delta = shift_fix
            block[rows] = (j <= i + shift + delta)[rows]
        vis[r0:r1, k0:k1] = block
        return vis

    def rows(self, upto=None):
        """The reference and gates over the first `upto` shards (None: all), cached per set of shards."""
        idx = frozenset(range(len(self.shards) if upto is None else upto))
        return self.rows_of(idx)

    def rows_of(self, idx):
        idx = frozenset(idx)
        if idx not in self._rows:
            vis = np.zeros((self.case.nq, self.case.nk), dtype=bool)
            for i in idx:
                vis |= self.visible(self.shards[i])
            self._rows[idx] = Rows(self.case.regime, np.where(vis, self.S, -np.inf), self.case.v)
        return self._rows[idx]

    @B.one_thread
    def emulate(self, order, offset, fault=None):
        """-> (final {O, L}, [state_views after every step but the last], bool [h, nq]: the rows the fault touched)."""
        c, (what, *arg) = self.case, fault or (None,)
        h, nq, d = c.hq, c.nq, c.d
        m, l, acc = np.full((h, nq), -np.inf), np.zeros((h, nq)), np.zeros((h, nq, d))
        touched, states = np.zeros((h, nq), dtype=bool), []
        for n, si in enumerate(order):
            (r0, r1), (k0, k1), shift = sh = self.shards[si]
            fix = (slice(32 * arg[1] - r0, 32 * arg[1] + 32 - r0), 1) if what == "s4" else None
            vis = self.visible(sh)
            if fix is not None:
                one = self.visible(sh, fix)
                touched[arg[0]] |= (one != vis).any(axis=1)
                vis = np.where((np.arange(h) == arg[0])[:, None, None], one, vis)
            S = np.where(vis, self.S, -np.inf)[:, :, k0:k1]
            if n > 0 and what == "s2":                                   # the restart pass forgets what it was handed
                blk = slice(256 * arg[1], 256 * arg[1] + 256)
                m[arg[0], blk], l[arg[0], blk], acc[arg[0], blk] = -np.inf, 0.0, 0.0
                touched[arg[0], blk] = True
            if n > 0 and what == "s5" and (r1 - r0) < nq:                  # state rows read (r1 - r0) apart; stores are right
                stride, q_len = nq, r1 - r0
                flat = r0 + np.arange(h)[:, None] * q_len + np.arange(q_len)[None, :]
                hh, rr = flat // stride, flat % stride
                m[:, r0:r1], l[:, r0:r1], acc[:, r0:r1] = m[hh, rr], l[hh, rr], acc[hh, rr]
                touched[1:, r0:r1] = True
            top = S.max(axis=-1, initial=-np.inf)
            sees = np.isfinite(top)
            if n > 0 and what == "s3":
                lost = ~sees & (np.arange(nq) >= r0)[None, :] & (np.arange(nq) < r1)[None, :]
                m[lost], l[lost], acc[lost] = -np.inf, 0.0, 0.0
                touched |= lost
            r = np.where(sees, np.maximum(m, top) - offset, m)
            r0_ = np.where(np.isfinite(r), r, 0.0)
            with np.errstate(invalid="ignore"):
                alpha = np.where(np.isfinite(m), np.exp(m - r0_), 0.0)
            p = np.where(sees[..., None], np.exp(S - r0_[..., None]), 0.0)
            p16 = _bf16(p)
            if n > 0 and what == "s6":
                g = slice(32 * arg[1], 32 * arg[1] + 32)
                p16[arg[0], g, arg[2] - k0:arg[2] - k0 + 32] = 0.0
                touched[arg[0], g] = True
            a_acc = alpha
            if n > 0 and what == "s1":
                a_acc = np.where((np.arange(h) == arg[0])[:, None], 1.0, alpha)
                touched[arg[0]] |= alpha[arg[0]] != 1.0
            l = l * alpha + p.sum(axis=-1)
            acc = acc * a_acc[..., None] + p16 @ c.v[:, k0:k1]
            m = r
            if n < len(order) - 1:
                states.append(state_views(acc, l, m))
        fin = state_views(acc, l, m)
        return {"O": _bf16(fin["O"]), "L": fin["L"]}, states, touched


# ------------------------------------------------------------------------------------------------ what the GPU file runs
# Tiles and rounds of fa2_fwd1_bf16.hip: a tile is 64 keys at d = 128 and 128 at d = 64, a round four tiles (256 / 512 keys).  A
# pass takes lane maxima in its first tile and in the tail tiles behind the last whole round; a lift can happen at the start of
# every round but the first.  With 1100 keys the 28-unit key is 308, the 130-unit key 902 (tests/regimes.py).
#   TWO     [0, 40) [40, 1100)           the long shard (1060 keys = 4 rounds + 36 at d = 128, 2 rounds + 36 at d = 64; a ragged
#                                        tail) holds both spikes: key 308 at its key 268 -- tile 4 of 16 (d = 128), tile 2 of 8
#                                        (d = 64), past the first tile, with a round start behind it: resumed, it lifts on carried
#                                        state (`lift`); key 902 at 862 lies in a round without maxima: resumed, the block restarts
#                                        and its second init_pass reloads the state (`spikes`).  [0, 40) is shorter than a tile;
#                                        after the long shard it meets a carried m far above all it holds.
#   THREE   [0, 40) [40, 1076) [1076, 1100)    the same long shard (1036 keys: the same rounds, a 12-key tail) between two shards
#                                        shorter than a tile, in all six orders: resumed once behind one and once behind both
#   THIRDS  [0, 100) [100, 700) [700, 1100)    d = 128: key 308 at 208 of 600 (tile 3, round 0; the lift at tile 4), key 902 at 202
#                                        of 400 (tile 3 of a single whole round: the restart); d = 64: the shards have one whole
#                                        round and none -- 400 keys run with maxima throughout, on carried state
STEP_H, STEP_N = 3, 1100
CUTS = {"two": (0, 40, 1100), "three": (0, 40, 1076, 1100), "thirds": (0, 100, 700, 1100)}
STEP_REGIMES = ("scale-one", "peaked", "spikes", "lift", "low-level")


def dense_shards(cuts):
    return [shard((a, b)) for a, b in zip(cuts[:-1], cuts[1:])]


@B.one_thread
def dense_step(regime, d, cuts):
    return Step(B.dense_case(regime, STEP_H, STEP_H, STEP_N, STEP_N, d, False), dense_shards(CUTS[cuts]))


# fa2_forward_step_strided: rows [R0, R0 + QLEN) of heads Q_STRIDE rows apart against keys [K0, K0 + KLEN) of heads K_STRIDE apart
Q_STRIDE, R0, QLEN = 1100, 200, 700
K_STRIDE, K0, KLEN = 1100, 100, 900
STRIDED_SHIFTS = (-45, 203)              # a negative one (local rows 0 .. 44 see no key); no multiple of 32
STRIDED_CUT = 500                        # the keys in two steps: [K0, 500) without a mask, [500, K0 + KLEN) under the shift


def strided_step(regime, d, shift):
    """Two steps over a row range in the middle of every head: a shard without a mask, then one under `shift` (so that with a
    negative shift the rows without a key carry a real state through the second step)."""
    case = B.dense_case(regime, STEP_H, STEP_H, STEP_N, STEP_N, d, False)
    rows = (R0, R0 + QLEN)
    return Step(case, [shard((K0, STRIDED_CUT), rows), shard((STRIDED_CUT, K0 + KLEN), rows, shift)])


# The causal zig-zag ring on two ranks: the sequence in four chunks of 275, rank 0 holds chunks 0 and 3, rank 1 chunks 1 and 2.
CHUNK = 275


def zigzag_steps(d):
    """[(label, Step over the gathered local tensors, causal reference rows)]: rank 0's queries -- its own keys under the local
    causal mask, then ALL of rank 1's keys into the second HALF of its rows; rank 1's queries -- its own keys, then the first
    HALF of rank 0's keys into ALL of its rows.  The Case of each is the local Q against the four chunks in the order
    [own 0, own 1, other 0, other 1]."""
    import regimes as R
    Q, K, V, dO, s = R.sequence("spikes", STEP_H, STEP_H, STEP_N, STEP_N, d)
    chunk = lambda t, i: t[:, CHUNK * i:CHUNK * i + CHUNK]
    out = []
    for rank, (own, other) in enumerate((((0, 3), (1, 2)), ((1, 2), (0, 3)))):
        q, g = (torch_cat([chunk(t, i) for i in own]) for t in (Q, dO))
        k, v = (torch_cat([chunk(t, i) for i in own + other]) for t in (K, V))
        case = B.Case("spikes", q, k, v, g, s, False)
        n = 2 * CHUNK
        if rank == 0:
            shards = [shard((0, n), (0, n), 0), shard((n, 2 * n), (CHUNK, n))]
        else:
            shards = [shard((0, n), (0, n), 0), shard((n, n + CHUNK), (0, n))]
        whole = B.dense_case("spikes", STEP_H, STEP_H, STEP_N, STEP_N, d, True)
        rows = np.concatenate([np.arange(CHUNK * i, CHUNK * i + CHUNK) for i in own])
        out.append((f"rank {rank}", Step(case, shards), whole, rows))
    return out


def torch_cat(ts):
    import torch
    return torch.cat(ts, dim=1).contiguous()
