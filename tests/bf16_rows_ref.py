"""References, per-row gates, a CPU model of the data flow and mutants for the bf16 forward and backward (a helper module, no
tests: tests/test_bf16_rows_reference.py certifies what is here on the CPU, tests/test_gpu_bf16_rows.py runs the kernels on it).
Built on tests/regimes.py: its inputs, ref_attention / ref_grouped (the forward's reference, on the bf16 inputs), ref_flow (the
backward's reference: the float64 formulas fed bf16(O_ref) and fp32(L_ref), the two arrays the kernels are handed -- DESIGN.md
section 6a says why) and emulate (the backward's data flow).

THE GATES (Case.gate()).  2-norms over d; u = 2^-9, bf16's unit round-off; P the softmax, dP = dO V^T, D = rowsum(dO o O16),
dS = P o (dP - D), s the softmax scale; under grouped heads a K/V row's sums run over the rows of all its query heads.

    O   row i :  kappa u sqrt(sum_j P_ij^2 |v_j|^2)                            + u |O_i|
    dV  row j :  kappa u sqrt(sum_i P_ij^2 |dO_i|^2)                           + u |dV_j|
    dQ  row i :  s ( kappa u sqrt(sum_j dS_ij^2 |k_j|^2) + sum_j e_ij |k_j| )  + u |dQ_i|
    dK  row j :  s ( kappa u sqrt(sum_i dS_ij^2 |q_i|^2) + sum_i e_ij |q_i| )  + u |dK_j|
    e_ij = phi P_ij ( sum_c |dO_ic| |v_jc| + sum_c |dO_ic| |O16_ic| )

  * first term: the independent bf16 roundings of P (the forward's second product, dV) and of dS (dQ, dK) add in quadrature.
    The forward's lazy reference does not enter: bf16 rounding is relative.
  * last term: the bf16 output.
  * e_ij: the fp32 sums behind dS -- D as fa2_bwd_delta_kernel forms it from the bf16 O, and the dP accumulation -- counted
    linearly, because an error in D is common to a row's keys.  Without it the gate is 0 where dS is 0 (row 0 under a causal
    mask: P = 1, O16 = v_0, dP = D exactly; a row sitting on a spike).  phi = PHI = 2^-22.  The count: fa2_bwd_delta_kernel adds 8
    products per lane (d = 128; 4 or 8 at d = 64 over two steps at most) and then 4 shuffle steps -- a chain of at most 12 fp32
    roundings, each at most 2^-24 of a partial sum that is itself at most sum |dO||O|; dP is d products summed in fp32 inside
    the matrix instructions.  The worst case of those chains ((12 + d) 2^-24) lies above the 2^-18 allowed here and is never met:
    the roundings are independent and the partial sums are about sqrt(n) terms large, not n, which puts the expected error at
    2^-24 sqrt(d / 2) of the rms term -- about 2^-24 of sum |dO||v| at d = 128.  phi = 2^-22 (each of the two sums counted
    with four times that) is kept.
  * grouped heads on the single kernel (routes 7 and 8|1 where fa2_backward_plan says 1, G > 1): every query head's dK / dV
    partial is stored in bf16 and fa2_bwd_fused_dkdv_out_kernel adds the G partials in fp32.  There the
    dK and dV gates get u sum_{h in group} |partial_h,j| (gate(..., partials=True)); the dK/dV kernel of the two-kernel route
    sums a group in its fp32 accumulators and gets nothing.
  * L: |dL| <= 1e-4 where |L_ref| <= 25, else <= 1e-3 (the project's per-row figures).  A row without a visible key: L = -inf,
    O = 0 and dQ = 0 exactly; a key no query row exists for (a packed sequence without queries): dK = dV = 0 exactly.
Nothing in a gate comes from a kernel.

KAPPA = 2.5, one number for O, dQ, dK and dV: the smallest multiple of 0.5 at which the emulation below uses at most ROOM = 0.75
of the gate on every row of every case the GPU file runs (cpu_cases()); the bound is 4.  At 2.0 `scale-one` dV reaches 0.86
(N = 1025, d = 64, causal), at 2.5 it is 0.74, the largest of all (tests/test_bf16_rows_reference.py prints every case's ratios;
its docstring and DESIGN.md section 6c keep the largest per regime and tensor).  It comes from the emulation and the float64
reference, never from a kernel's output.
NOT ROW-GATED (TENSOR_GATED; no kappa <= 4 brings them under 0.75, and the gate is not widened for them):
  * `low-level` dQ and dK: Q and K are nearly collinear, so the summed rounding error of dS K is a scalar with Gaussian tails,
    not a 2-norm over d -- 1.50 and 1.55 of the gate at kappa = 2.5, 0.95 and 0.98 at 4.  They keep the tensor gates of
    tests/test_gpu_regimes.py (rel-L2 0.15 and 2e-2); the regime is row-gated on O, L and dV.
  * `offsets` O and dV: every component of O is about 0.5 (the mean of V), of dV about 0.1 sum_i P_ij -- just above a power of
    two, where bf16's spacing is widest relative to the value.  The output rounding alone, 2^-8 / sqrt(12) per component, is
    about 0.9 u |O_i| at u = 2^-9 and does not shrink with kappa: 0.97 (O) and 0.91 (dV) of the gate at kappa = 2.5, 0.89 and
    0.81 at 4.  They keep the suite's rel-L2 5e-3; the regime is row-gated on L, dQ and dK.

THE EMULATION.  emulate_forward: p = exp(S - r) rounded to bf16 for the second product, the row sum unrounded, O rounded to
bf16, at the reference r = row maximum - offset, offset in FWD_OFFSETS = (0, 6): the kernel's reference lags its maximum by up to
kFwdRescaleThr = 6.  emulate_backward: regimes.emulate (D in fp32, P and dS in bf16) with the outputs rounded to bf16; with
partials=True each query head's dK / dV is rounded to bf16 before the group is summed.

THE MUTANTS (m1 .. m10): what a specific fault would produce, built from the emulation -- the forward's flow with an edited
mask or second product, the backward's as regimes.emulate on the block of rows and keys the fault touches, taken out of the
whole and put back in its faulty form (the emulation's three products are sums over (row, key) pairs, so they split exactly)."""
import functools

import numpy as np
import torch

import regimes as R

U = 2.0 ** -9                                 # bf16's unit round-off
PHI = 2.0 ** -22                              # the fp32 sums behind dS (the docstring's count)
KAPPA = 2.5
ROOM = 0.75                                   # what the emulation may use of a gate
FWD_OFFSETS = (0.0, 6.0)                      # the forward's reference: at the row maximum and kFwdRescaleThr below it
L_ABS, L_ABS_FAR, L_NEAR = 1e-4, 1e-3, 25.0
BF16_REL = 5e-3                               # the suite's tensor gate
OUTPUTS = ("O", "L", "dQ", "dK", "dV")
GRADS = ("dQ", "dK", "dV")
TENSOR_GATED = {"low-level": {"dQ": 0.15, "dK": 2e-2}, "offsets": {"O": BF16_REL, "dV": BF16_REL}}      # rel-L2 in place of the row gate
GUARD = 64                                    # elements of NaN on either side of an output (case (e))

f64, _bf16 = R.f64, R._bf16


def _norm(x):
    return np.linalg.norm(x, axis=-1)


def one_thread(fn):
    """Run fn with torch on one thread: the conversions here are small, and torch's thread pool beside numpy's costs a multiple
    of the arithmetic (building one case: 1.0 s without this, 0.33 s with it).  The caller's setting is put back."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*args, **kwargs)
        finally:
            torch.set_num_threads(n)
    return wrapped


def single_kernel(n, d):
    """Rule (a) of include/fa2_mi355x.h: whether the bf16 backward of a square problem runs the single kernel."""
    up = lambda x, m: -(-x // m) * m
    return 5 * up(n, 256) <= 7 * up(n, 64) if d == 128 else 13 * up(n, 256) <= 14 * up(n, 64)


def visible(nq, nk, causal, shift=0):
    """[nq, nk] bool: key j visible to row i (bottom-right causal mask, moved by `shift` keys)."""
    if not causal:
        return np.ones((nq, nk), dtype=bool)
    return np.arange(nk)[None, :] <= np.arange(nq)[:, None] + (nk - nq) + shift


# ------------------------------------------------------------------------------------------------ a problem and its gates
class Case:
    """One sequence: host bf16 Q, dO [hq, nq, d] and K, V [hkv, nk, d] (.t), their float64 values (.q .k .v .g), the reference
    (.ref: O, L of ref_grouped; dQ, dK, dV of ref_flow fed .O16 and .L32) and the two parts of every row gate."""

    def __init__(self, regime, Q, K, V, dO, s, causal):
        self.regime, self.s, self.causal, self.t = regime, s, causal, (Q, K, V, dO)
        self.q, self.k, self.v, self.g = (f64(t) for t in self.t)
        (self.hq, self.nq, self.d), (self.hkv, self.nk, _) = self.q.shape, self.k.shape
        self.G = self.hq // self.hkv
        O, L, *_ = R.ref_grouped(Q, K, V, dO, s, causal)
        self.O16, self.L32 = R.kernel_feed(O, L)
        self.ref = dict(zip(OUTPUTS, (O, L) + tuple(R.ref_flow(Q, K, V, dO, s, causal, self.O16, self.L32))))
        self.key_seen = np.full((self.hkv, self.nk), self.nq > 0)       # the last row sees every key under either mask
        self._gates()

    def scores(self, causal=None, shift=0):
        """float64 s Q K^T [hq, nq, nk], -inf on hidden keys (causal: the case's own mask unless given)."""
        S = self.s * (self.q @ np.swapaxes(np.repeat(self.k, self.G, axis=0), -1, -2))
        return np.where(visible(self.nq, self.nk, self.causal if causal is None else causal, shift), S, -np.inf)

    def _gates(self):
        q, k, v, g, s, G = self.q, self.k, self.v, self.g, self.s, self.G
        O16, L32 = f64(self.O16), f64(self.L32)
        qn, kn, vn, gn = (_norm(x) for x in (q, k, v, g))
        vis = visible(self.nq, self.nk, self.causal)
        quad = {n: np.zeros(self.ref[n].shape[:2]) for n in ("O",) + GRADS}      # dK, dV: squares until the group is summed
        lin = {n: np.zeros(self.ref[n].shape[:2]) for n in ("dQ", "dK")}
        part = {n: np.zeros(self.ref[n].shape[:2]) for n in ("dK", "dV")}
        for h in range(self.hq):
            hk = h // G
            seen = np.isfinite(L32[h])
            S = np.where(vis, s * (q[h] @ k[hk].T), -np.inf)
            P = np.where(seen[:, None], np.exp(S - np.where(seen, L32[h], 0.0)[:, None]), 0.0)
            D = (g[h] * O16[h]).sum(axis=-1)
            dS = P * (g[h] @ v[hk].T - D[:, None])
            E = PHI * P * (np.abs(g[h]) @ np.abs(v[hk]).T + (np.abs(g[h]) * np.abs(O16[h])).sum(axis=-1)[:, None])
            quad["O"][h] = np.sqrt((P * P) @ (vn[hk] ** 2))
            quad["dQ"][h] = s * np.sqrt((dS * dS) @ (kn[hk] ** 2))
            lin["dQ"][h] = s * (E @ kn[hk])
            quad["dV"][hk] += (P * P).T @ (gn[h] ** 2)
            quad["dK"][hk] += (dS * dS).T @ (qn[h] ** 2)
            lin["dK"][hk] += s * (E.T @ qn[h])
            if G > 1:
                part["dK"][hk] += U * _norm(s * (dS.T @ q[h]))
                part["dV"][hk] += U * _norm(P.T @ g[h])
        quad["dK"], quad["dV"] = s * np.sqrt(quad["dK"]), np.sqrt(quad["dV"])
        self.quad = {n: U * x for n, x in quad.items()}
        self.rest = {n: lin.get(n, 0.0) + U * _norm(self.ref[n]) for n in quad}
        self.part = part
        near = np.abs(self.ref["L"]) <= L_NEAR
        self.l_gate = np.where(near, L_ABS, L_ABS_FAR)

    def gate(self, name, partials=False, kappa=KAPPA):
        """The row gate of `name` [heads, rows]: "L" or one of O, dQ, dK, dV (partials: the grouped single-kernel route)."""
        if name == "L":
            return self.l_gate
        out = kappa * self.quad[name] + self.rest[name]
        return out + self.part[name] if partials and name in self.part else out

    # ---- the data flow
    @one_thread
    def emulate_forward(self, offset):
        return forward_flow(self.scores(), np.repeat(self.v, self.G, axis=0), offset)

    @one_thread
    def emulate_backward_exact(self):
        """regimes.emulate as it stands: float64 sums of the bf16-rounded P and dS (what the mutants splice)."""
        return dict(zip(GRADS, R.emulate(*self.t, self.s, self.causal, self.O16, self.L32)))

    @one_thread
    def emulate_backward(self, partials=False):
        if partials and self.G > 1:
            K, V = (t.repeat_interleave(self.G, dim=0) for t in self.t[1:3])
            dQ, dK, dV = R.emulate(self.t[0], K, V, self.t[3], self.s, self.causal, self.O16, self.L32)
            dK, dV = (R._group_sum(_bf16(x), self.hkv) for x in (dK, dV))
            return dict(dQ=_bf16(dQ), dK=_bf16(dK), dV=_bf16(dV))
        return {n: _bf16(x) for n, x in self.emulate_backward_exact().items()}


class Packed(Case):
    """Sequences side by side along the row axis (a packed batch [H, T, d]): every array is the concatenation of the parts'."""

    def __init__(self, parts):
        self.parts = parts
        p0 = parts[0]
        self.regime, self.s, self.causal, self.G, self.hq, self.hkv, self.d = p0.regime, p0.s, p0.causal, p0.G, p0.hq, p0.hkv, p0.d
        cat = lambda xs: torch.cat(xs, dim=1) if isinstance(xs[0], torch.Tensor) else np.concatenate(xs, axis=1)
        self.t = tuple(cat([p.t[i] for p in parts]) for i in range(4))
        self.O16, self.L32 = cat([p.O16 for p in parts]), cat([p.L32 for p in parts])
        for field in ("ref", "quad", "rest", "part"):
            setattr(self, field, {n: cat([getattr(p, field)[n] for p in parts]) for n in getattr(p0, field)})
        self.l_gate, self.key_seen = cat([p.l_gate for p in parts]), cat([p.key_seen for p in parts])
        self.nq, self.nk = self.t[0].shape[1], self.t[1].shape[1]

    def emulate_forward(self, offset):
        outs = [p.emulate_forward(offset) for p in self.parts]
        return {n: np.concatenate([o[n] for o in outs], axis=1) for n in outs[0]}

    def emulate_backward(self, partials=False):
        outs = [p.emulate_backward(partials) for p in self.parts]
        return {n: np.concatenate([o[n] for o in outs], axis=1) for n in outs[0]}


@one_thread
def forward_flow(S, v, offset, edit=None):
    """The forward's arithmetic at the reference row maximum - offset: p = exp(S - r), l = sum p (unrounded), p in bf16 for the
    second product, O = bf16((p16 v) / l), L = r + log l.  S [..., nq, nk] with -inf on hidden keys, v [..., nk, d];
    edit(p16) -> p16: where a mutant alters the second product alone.  A row without a visible key: O = 0, L = -inf."""
    m = S.max(axis=-1, initial=-np.inf)
    seen = np.isfinite(m)
    r = np.where(seen, m - offset, 0.0)
    p = np.exp(S - r[..., None])
    l = np.where(seen, p.sum(axis=-1), 1.0)
    p16 = _bf16(p)
    if edit is not None:
        p16 = edit(p16)
    with np.errstate(divide="ignore"):
        L = np.where(seen, r + np.log(l), -np.inf)
    return dict(O=_bf16((p16 @ v) / l[..., None]), L=L)


# ------------------------------------------------------------------------------------------------ errors, ratios, the verdict
def row_errors(got, case):
    """{tensor: error per row [heads, rows]} of a result {tensor: array}: 2-norms over d, |dL| for L.  Where the rule is exact
    -- a row without a visible key (O = 0, L = -inf, dQ = 0), a key without query rows (dK = dV = 0) -- the error is 0 if the
    rule holds and +inf if not."""
    ref, out = case.ref, {}
    none = np.isneginf(ref["L"])
    for name, x in got.items():
        x = f64(x)
        if name == "L":
            with np.errstate(invalid="ignore"):
                e = np.abs(x - ref["L"])
            out[name] = np.where(none, np.where(np.isneginf(x), 0.0, np.inf), e)
            continue
        e, zero = _norm(x - ref[name]), np.abs(x).max(axis=-1, initial=0.0) == 0.0
        exact = none if name in ("O", "dQ") else ~case.key_seen
        out[name] = np.where(exact, np.where(zero, 0.0, np.inf), e)
    return out


def row_gated(case, name):
    return name not in TENSOR_GATED.get(case.regime, {})


def ratios(got, case, partials=False, kappa=KAPPA):
    """{tensor: error / gate per row} for the row-gated tensors of `got` (0 / 0 = 0: an exact rule that holds)."""
    out = {}
    for name, e in row_errors(got, case).items():
        if row_gated(case, name):
            gate = case.gate(name, partials, kappa)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[name] = np.where(e == 0.0, 0.0, e / gate)
    return out


def pattern(bad, heads=None):
    """'b h: rows, per 32-row group' of a [heads, rows] mask of failing rows (heads: H of a [B, H] problem folded into axis 0)."""
    out = []
    for h in np.nonzero(bad.any(axis=-1))[0]:
        rows = np.nonzero(bad[h])[0]
        groups = np.bincount(rows // 32)
        who = f"h{h}" if heads is None else f"b{h // heads} h{h % heads}"
        out.append(f"{who}: {rows.size} rows, per 32-row group " + " ".join(f"{g}:{n}" for g, n in enumerate(groups) if n))
    return "; ".join(out[:12]) + (f"; ... {len(out)} heads in all" if len(out) > 12 else "")


def check(label, got, case, partials=False, heads=None):
    """The checks in their order: no NaN left, the O / gradient gates on every row (the tensor gate for what TENSOR_GATED
    names), the L gate.  got: {tensor: array or tensor} -- any subset of O, L, dQ, dK, dV.  -> {tensor: largest ratio to the
    gate} with |dL| itself under "L" and the rel-L2 of a tensor-gated tensor under "<name> rel-L2"."""
    got = {n: f64(x.float().cpu() if isinstance(x, torch.Tensor) else x) for n, x in got.items()}
    for name, x in got.items():
        nan = np.isnan(x) if name == "L" else np.isnan(x).any(axis=-1)
        assert not nan.any(), f"{label}: NaN left in {name} (never written?): {pattern(nan, heads)}"
    rat, errs, report = ratios(got, case, partials), row_errors(got, case), {}
    for name in [n for n in ("O",) + GRADS + ("L",) if n in got]:
        if not row_gated(case, name):
            rel = report[f"{name} rel-L2"] = R.rel(got[name], case.ref[name])
            assert rel <= TENSOR_GATED[case.regime][name], f"{label}: {name} rel-L2 {rel:.3e}"
            continue
        r = rat[name]
        bad = r > 1.0
        if bad.any():
            h, i = np.unravel_index(np.argmax(r), r.shape)
            who = f"h {h}" if heads is None else f"b {h // heads}, h {h % heads}"
            raise AssertionError(f"{label}: {name} row gate missed at ({who}, row {i}): error {errs[name][h, i]:.3e} = {r[h, i]:.2f} x "
                                 f"gate; {int(bad.sum())} rows fail: {pattern(bad, heads)}")
        report[name] = float(errs["L"].max(initial=0.0)) if name == "L" else float(r.max(initial=0.0))
    return report


def report_line(label, report):
    """One line per case: the largest ratio per tensor and max |dL| (rel-L2 where a tensor keeps its tensor gate)."""
    return f"BF16ROWS {label}: " + "  ".join(f"max|dL| {v:.2e}" if n == "L" else f"{n} {v:.2e}" if n.endswith("rel-L2") else f"{n} {v:.3f}"
                                             for n, v in report.items())


# ------------------------------------------------------------------------------------------------ what the GPU file runs
EDGE_N = (31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 897, 1000, 1023, 1024, 1025, 1279, 1280, 1281)
EDGE_REGIMES, EDGE_H = ("scale-one", "peaked"), 2
ORDER_BH, ORDER_N, ORDER_REGIME = ((2, 4), (2, 8), (3, 8), (1, 9), (1, 17)), (768, 520), "scale-one"
REGIME_H, REGIME_N = 3, R.SQUARE_N
OTHER_REGIMES = ("scale-one", "peaked")
QK_SHAPES, PACKED, GQA_HEADS, GQA_N = R.QK_SHAPES, R.PACKED_TWO, R.HEADS_GQA, 1100
WORKSPACE_CASES = (("scale-one", 2, 1024, 128, True), ("scale-one", 2, 520, 64, True))       # single kernel; two kernels
HEAD_DIMS, MASKS = (64, 128), (False, True)


@functools.lru_cache(maxsize=6)
@one_thread
def dense_case(regime, hq, hkv, nq, nk, d, causal):
    """One dense problem on regimes.sequence's data; a [B, H] problem is the B H-head one (every head draws its own data)."""
    Q, K, V, dO, s = R.sequence(regime, hq, hkv, nq, nk, d)
    return Case(regime, Q, K, V, dO, s, causal)


@functools.lru_cache(maxsize=2)
@one_thread
def packed_case(regime, seqs, d, causal):
    hq, hkv = GQA_HEADS
    return Packed([Case(regime, *R.sequence(regime, hq, hkv, nq, nk, d), causal) for nq, nk in seqs])


def cpu_cases():
    """Every (label, builder, arguments) the GPU file hands a kernel.  Case (b) on the CPU: the (2, 4) and (1, 9) problems -- the
    heads of the others are further draws of the same regime at the same two lengths."""
    out = []
    for d in HEAD_DIMS:
        for causal in MASKS:
            tail = (d, causal)
            out += [(f"edges {r} N{n}", dense_case, (r, EDGE_H, EDGE_H, n, n) + tail) for r in EDGE_REGIMES for n in EDGE_N]
            out += [(f"order H{h} N{n}", dense_case, (ORDER_REGIME, h, h, n, n) + tail) for h in (8, 9) for n in ORDER_N]
            out += [(f"regimes {r} N{n}", dense_case, (r, REGIME_H, REGIME_H, n, n) + tail) for r in R.REGIMES for n in REGIME_N]
            for r in OTHER_REGIMES:
                out += [(f"qk {r} {nq}x{nk}", dense_case, (r,) + GQA_HEADS + (nq, nk) + tail) for nq, nk in QK_SHAPES]
                out += [(f"packed {r}", packed_case, (r, PACKED) + tail), (f"gqa {r} N{GQA_N}", dense_case, (r,) + GQA_HEADS + (GQA_N, GQA_N) + tail)]
            out += [(f"workspace {r} N{n}", dense_case, (r, h, h, n, n) + tail) for r, h, n, dd, c in WORKSPACE_CASES if (dd, c) == tail]
    return [(f"{label} d{args[-2]} {'causal' if args[-1] else 'full'}", build, args) for label, build, args in out]


# ------------------------------------------------------------------------------------------------ the mutants
# Each takes a dense multi-head Case (G = 1) and returns {tensor: what the faulty kernel would write}, bf16 values as float64.
# `group` is a 32-row group, `head` a head; the forward ones also take the reference's offset.
def _rows(group):
    return slice(32 * group, 32 * group + 32)


def _forward_with(case, offset, head, rows, S_rows=None, edit=None):
    """The emulated forward with rows `rows` of `head` recomputed from the scores S_rows / with the second product edited."""
    out = case.emulate_forward(offset)
    S = case.scores()[head, rows] if S_rows is None else S_rows
    new = forward_flow(S, case.v[head], offset, edit)
    for n in out:
        out[n][head, rows] = new[n]
    return out


def m1_key_block_missing_from_pv(case, offset, head, group, key0):
    """(m1) keys key0 .. key0 + 31 missing from P V alone for one 32-row group: L stays exact."""
    def edit(p16):
        p16 = p16.copy()
        p16[:, key0:key0 + 32] = 0.0
        return p16
    return _forward_with(case, offset, head, _rows(group), edit=edit)


def m2_mask_shifted_forward(case, offset, head, group):
    """(m2) the causal mask shifted by one key (a row sees the key behind its diagonal) on one 32-row group, forward."""
    assert case.causal
    return _forward_with(case, offset, head, _rows(group), S_rows=case.scores(True, 1)[head, _rows(group)])


@one_thread
def _block(case, head, rows, keys, causal, O16=None):
    """regimes.emulate on rows `rows` of `head` against keys `keys` (causal: bottom-right aligned INSIDE the block, so a block
    of keys 0 .. rows.stop - 1 + shift is the causal mask shifted by `shift`)."""
    O16 = f64(case.O16)[head:head + 1, rows] if O16 is None else O16
    return [x[0] for x in R.emulate(case.q[head:head + 1, rows], case.k[head:head + 1, keys], case.v[head:head + 1, keys],
                                    case.g[head:head + 1, rows], case.s, causal, O16, f64(case.L32)[head:head + 1, rows])]


def _splice(case, head, rows, right, wrong, which=GRADS):
    """The emulated backward with the block `right` = (keys, causal[, O16]) of rows `rows` taken out and `wrong` put in its
    place (None: nothing), on the tensors `which`; rounded to bf16 at the end, like the kernels' outputs."""
    assert case.G == 1
    out = {n: x.copy() for n, x in case.emulate_backward_exact().items()}
    for sign, blk in ((-1.0, right), (1.0, wrong)):
        if blk is None:
            continue
        keys = blk[0]
        for n, x in zip(GRADS, _block(case, head, rows, *blk)):
            if n in which:
                out[n][head, rows if n == "dQ" else keys] += sign * x
    return {n: _bf16(x) for n, x in out.items()}


def m3_mask_shifted_backward(case, head, group):
    """(m3) the causal mask shifted by one key on one 32-row group, backward (L is an input: nothing else notices)."""
    assert case.causal and case.nq == case.nk
    rows = _rows(group)
    return _splice(case, head, rows, (slice(0, rows.stop), True), (slice(0, rows.stop + 1), True))


def m4_other_mask(case, offset, head, group):
    """(m4) 32 rows under the other mask, forward and backward."""
    assert case.nq == case.nk
    rows = _rows(group)
    out = _forward_with(case, offset, head, rows, S_rows=case.scores(not case.causal)[head, rows])
    blocks = ((slice(0, rows.stop), True), (slice(0, case.nk), False))
    out.update(_splice(case, head, rows, *(blocks if case.causal else blocks[::-1])))
    return out


def m5_heads_swapped(case, offset, heads, block):
    """(m5) one 256-row block of two heads swapped, in all five outputs."""
    out = dict(case.emulate_forward(offset), **case.emulate_backward())
    a, b = heads
    rows = slice(256 * block, 256 * block + 256)
    for x in out.values():
        x[[a, b], rows] = x[[b, a], rows]
    return out


def m6_handoff_lost(case, head, group, key_block):
    """(m6) dQ of one 32-row sub-tile missing one 256-key block's contribution (the block wholly visible to the rows)."""
    keys = slice(256 * key_block, 256 * key_block + 256)
    assert keys.stop <= case.nk and (not case.causal or keys.stop <= 32 * group + 1)
    return _splice(case, head, _rows(group), (keys, False), None, which=("dQ",))


def m7_subtile_missing_from_dkdv(case, head, group, key_block):
    """(m7) one 256-key block's dK and dV missing one 32-row sub-tile."""
    keys = slice(256 * key_block, 256 * key_block + 256)
    assert keys.stop <= case.nk and (not case.causal or keys.stop <= 32 * group + 1)
    return _splice(case, head, _rows(group), (keys, False), None, which=("dK", "dV"))


def m8_neighbours_d(case, head, row):
    """(m8) one row taking its neighbour's D.  regimes.emulate forms D = rowsum(dO o O16) itself, so the row is handed an O16
    moved along dO by exactly what gives it row + 1's D."""
    rows, O16, g = slice(row, row + 1), f64(case.O16), case.g
    D = (g[head] * O16[head]).sum(axis=-1)
    moved = O16[head:head + 1, rows] + g[head, rows] * ((D[row + 1] - D[row]) / float(g[head, row] @ g[head, row]))
    keys = slice(0, row + 1 + case.nk - case.nq) if case.causal else slice(0, case.nk)
    return _splice(case, head, rows, (keys, False), (keys, False, moved))


@one_thread
def m9_next_heads_keys(case, offset, head):
    """(m9) at a ragged N under the full mask, the last 64-key tile reading the next head's first keys as if they were visible:
    the forward's O and L, and the backward's dQ (nothing past the end is stored, so dK and dV are untouched)."""
    assert not case.causal and case.nk % 64 and case.G == 1 and head + 1 < case.hq
    pad = -case.nk % 64
    k2, v2 = case.k[head + 1, :pad], case.v[head + 1, :pad]
    S = np.concatenate([case.scores()[head], case.s * (case.q[head] @ k2.T)], axis=-1)
    out = case.emulate_forward(offset)
    new = forward_flow(S, np.concatenate([case.v[head], v2]), offset)
    for n in out:
        out[n][head] = new[n]
    dQ = case.emulate_backward_exact()["dQ"].copy()
    dQ[head] += R.emulate(case.q[head:head + 1], k2[None], v2[None], case.g[head:head + 1], case.s, False,
                          f64(case.O16)[head:head + 1], f64(case.L32)[head:head + 1])[0][0]
    out["dQ"] = _bf16(dQ)
    return out


def m10_key_half_left_out(case, head, group, key0):
    """(m10) at d = 64, one 128-key half's dQ running sum left out of one 32-row tile."""
    assert case.d == 64
    keys = slice(key0, key0 + 128)
    assert keys.stop <= case.nk and (not case.causal or keys.stop <= 32 * group + 1)
    return _splice(case, head, _rows(group), (keys, False), None, which=("dQ",))
