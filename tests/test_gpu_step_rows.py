"""GPU: the resumable forward step row by row -- fa2_forward_step, fa2_forward_step_strided and fa2_forward_state_finalize through
the C entry points, against tests/step_rows_ref.py (certified on the CPU by
tests/test_step_rows_reference.py).

Every ring step runs the `STATE && p.resume` branches of fa2_fwd1_impl: init_pass() reloads O^T, l and m_run from memory, the
restart calls it a second time, m_run arrives as a reference that may already lag, and a lift moves it by 64 ln 2 before it is
stored again.  The one test that called the step directly used one cut, flat regimes and a gate per tensor.  Here O and L are gated
per row after the last step (bf16_rows_ref's O gate and L figures on the float64 attention over the union of the shards), and after
every step before it the two quantities of the carried state that do not depend on its representation are: M + ln l is the L,
Oacc / l the O, over the keys seen so far.  O, L, Oacc and M are the caller's, NaN-filled before the first step, between
64-element NaN bands that stay NaN.

DENSE (fa2_forward_step; H = 3, N_q = 1100, 1100 keys, both head dims; step_rows_ref.CUTS says where the cuts come from: a tile is
64 keys at d = 128 and 128 at d = 64, a round four tiles).  [0, 40) [40, 1100) and [0, 40) [40, 1076) [1076, 1100) in every order:
the long shard holds the 28-unit key past its first tile with a round start behind it (`lift`: a lift on carried state whenever
it is resumed) and the 130-unit key in a round without maxima (`spikes`: a restart whose second init_pass reloads the state); run
first, the short flat shards that follow meet a carried m far above all they hold; the short shards are shorter than a tile and
the long one has a ragged tail.  [0, 100) [100, 700) [700, 1100): at d = 128 the lift and the restart in two different resumed
shards.  Regimes: scale-one, peaked, spikes, lift, low-level.
FINALIZE: fa2_forward_state_finalize on a stored state: gated per row, Oacc and M untouched.
STRIDED (fa2_forward_step_strided): rows [200, 900) of heads 1100 rows apart against keys of heads 1100 apart, q_head_stride >
q_len and kv_head_stride > kv_len; causal with causal_shift -45 (rows 0 .. 44 of the range see no key in that step: their state
passes through bit for bit), 203 (no multiple of 32) and kv_len (bit for bit the call without a mask); every row outside the
range keeps its sentinel bits in O, L, Oacc and M.  The two step shapes of the causal zig-zag ring, once each, on `spikes`: all
keys into half of the rows, half of the keys into all rows, against the causal reference of the whole problem.
Every case prints one BF16ROWS line per order; a failure names head, row and the failing rows per 32-row group."""
import itertools

import numpy as np
import pytest
import torch

import bf16_rows_ref as B
import step_rows_ref as T

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT32 = 0x7FA5A5A5                      # a NaN pattern no kernel computes


def _lib():
    import cuda_flashattention_amd as fa
    return fa._capi.lib()


def _banded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * B.GUARD,), NAN, dtype=dtype, device="cuda")
    return buf, buf[B.GUARD:B.GUARD + n].view(shape)


class State:
    """O (bf16), L, Oacc, M (fp32) for [H, rows(, d)], NaN-filled between NaN bands."""

    def __init__(self, H, rows, d):
        self.bufs, self.t = {}, {}
        for n, shape, dt in (("O", (H, rows, d), torch.bfloat16), ("L", (H, rows), torch.float32), ("Oacc", (H, rows, d), torch.float32),
                             ("M", (H, rows), torch.float32)):
            self.bufs[n], self.t[n] = _banded(shape, dt)

    def fill(self):
        for b in self.bufs.values():
            b.fill_(NAN)

    def ptrs(self, row0=0):
        return [self.t[n][0, row0:].data_ptr() for n in ("O", "L", "Oacc", "M")]

    def views(self):
        return T.state_views(self.t["Oacc"].cpu(), self.t["L"].cpu(), self.t["M"].cpu())

    def result(self):
        return {"O": self.t["O"].float().cpu(), "L": self.t["L"].cpu()}

    def bands_are_nan(self, label):
        for n, b in self.bufs.items():
            assert torch.isnan(b[:B.GUARD].float()).all() and torch.isnan(b[-B.GUARD:].float()).all(), f"{label}: a guard band of {n} was written"


def _dense_step(Q, K, V, st, keys, d, s, first, last):
    k0, k1 = keys
    ks, vs = (t[:, k0:k1].contiguous() for t in (K, V))
    rc = _lib().fa2_forward_step(Q.data_ptr(), ks.data_ptr(), vs.data_ptr(), *st.ptrs(), 1, Q.shape[0], Q.shape[1], k1 - k0, d, s, 0, int(first), int(last),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()


def _strided_step(Q, K, V, st, sh, d, s, first, last, q_stride, k_stride, causal=None):
    """One fa2_forward_step_strided over the shard's row and key range of [H, stride, d] tensors."""
    (r0, r1), (k0, k1), shift = sh
    causal = shift is not None if causal is None else causal
    rc = _lib().fa2_forward_step_strided(Q[0, r0:].data_ptr(), K[0, k0:].data_ptr(), V[0, k0:].data_ptr(), *st.ptrs(r0), 1, Q.shape[0], r1 - r0, k1 - k0, d, s, 0,
                                         int(first), int(last), q_stride, k_stride, int(causal), shift or 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()


def _report(label, report):
    print(B.report_line(label, report))


# ------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("cuts", list(T.CUTS))
@pytest.mark.parametrize("regime", T.STEP_REGIMES)
def test_dense_steps_in_every_shard_order(regime, cuts, d):
    step = T.dense_step(regime, d, cuts)
    c = step.case
    Q, K, V = (t.cuda() for t in c.t[:3])
    st = State(c.hq, c.nq, d)
    for order in itertools.permutations(range(len(step.shards))):
        st.fill()
        label, report = f"step {regime} {cuts} d{d} order {order}", {}
        for n, si in enumerate(order):
            last = n == len(order) - 1
            _dense_step(Q, K, V, st, step.shards[si][1], d, c.s, n == 0, last)
            got = st.result() if last else st.views()
            new = B.check(f"{label} after step {n}" + ("" if last else " (state)"), got, step.rows_of(order[:n + 1]))
            for k, v in new.items():
                report[k] = max(report.get(k, 0.0), v)
        st.bands_are_nan(label)
        _report(label, report)


@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("regime", ("scale-one", "spikes"))
def test_finalize_turns_a_stored_state_into_results(regime, d):
    step = T.dense_step(regime, d, "two")
    c = step.case
    Q, K, V = (t.cuda() for t in c.t[:3])
    st = State(c.hq, c.nq, d)
    st.fill()
    for n, si in enumerate((0, 1)):
        _dense_step(Q, K, V, st, step.shards[si][1], d, c.s, n == 0, False)
    acc, M = st.t["Oacc"].clone(), st.t["M"].clone()
    rc = _lib().fa2_forward_state_finalize(*st.ptrs(), c.hq * c.nq, d, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    label = f"finalize {regime} d{d}"
    _report(label, B.check(label, st.result(), step.rows()))
    assert torch.equal(st.t["Oacc"], acc) and torch.equal(st.t["M"], M), f"{label}: the state was written"
    st.bands_are_nan(label)


# ------------------------------------------------------------------------------------------------ strided
def _strided_tensors(case, q_stride, k_stride):
    """Q [H, q_stride, d] and K, V [H, k_stride, d]: the case's rows and keys, NaN behind them where a stride is longer."""
    def pad(t, n):
        out = torch.full((t.shape[0], n, t.shape[2]), NAN, dtype=t.dtype)
        out[:, :t.shape[1]] = t
        return out.cuda()
    return pad(case.t[0], q_stride), pad(case.t[1], k_stride), pad(case.t[2], k_stride)


def _sentinel(st):
    for n in ("L", "Oacc", "M"):
        st.t[n].view(torch.int32).fill_(SENT32)
    st.t["O"].view(torch.int16).fill_(0x7FA5)


def _outside_keeps_its_bits(st, r0, r1, label):
    for n, want in (("L", SENT32), ("Oacc", SENT32), ("M", SENT32), ("O", 0x7FA5)):
        bits = st.t[n].view(torch.int32 if n != "O" else torch.int16)
        assert (bits[:, :r0] == want).all() and (bits[:, r1:] == want).all(), f"{label}: {n} was written outside the row range"


@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("shift", T.STRIDED_SHIFTS + (T.KLEN,))
@pytest.mark.parametrize("regime", ("scale-one", "spikes"))
def test_strided_steps_over_a_row_range(regime, shift, d):
    step = T.strided_step(regime, d, shift)
    c = step.case
    assert T.Q_STRIDE > T.QLEN and T.K_STRIDE > T.KLEN and T.R0 + T.QLEN <= T.Q_STRIDE and T.K0 + T.KLEN <= T.K_STRIDE
    Q, K, V = _strided_tensors(c, T.Q_STRIDE, T.K_STRIDE)
    st = State(c.hq, T.Q_STRIDE, d)
    _sentinel(st)
    r0, r1 = step.shards[0][0]
    label = f"strided {regime} shift {shift} d{d}"
    _strided_step(Q, K, V, st, step.shards[0], d, c.s, True, False, T.Q_STRIDE, T.K_STRIDE)
    inside = lambda got: {n: x[:, r0:r1] for n, x in got.items()}
    ref0, ref = step.rows(1), step.rows()
    cut = lambda rows: _Cut(rows, r0, r1)
    report = B.check(f"{label} after step 0 (state)", inside(st.views()), cut(ref0))
    before = {n: st.t[n].clone() for n in ("L", "Oacc", "M")}
    _strided_step(Q, K, V, st, step.shards[1], d, c.s, False, False, T.Q_STRIDE, T.K_STRIDE)
    _outside_keeps_its_bits(st, r0, r1, label)
    for k, v in B.check(f"{label} after step 1 (state)", inside(st.views()), cut(ref)).items():
        report[k] = max(report.get(k, 0.0), v)
    if shift < 0:                        # the rows without a key in the second step: the state passes through bit for bit
        for n, t in before.items():
            assert torch.equal(st.t[n][:, r0:r0 - shift], t[:, r0:r0 - shift]), f"{label}: {n} of a row without a key changed"
    if shift >= T.KLEN:                  # a shift of at least kv_len hides nothing: the call without a mask, bit for bit
        plain = State(c.hq, T.Q_STRIDE, d)
        _sentinel(plain)
        _strided_step(Q, K, V, plain, step.shards[0], d, c.s, True, False, T.Q_STRIDE, T.K_STRIDE)
        _strided_step(Q, K, V, plain, step.shards[1], d, c.s, False, False, T.Q_STRIDE, T.K_STRIDE, causal=False)
        for n in ("L", "Oacc", "M"):
            assert torch.equal(plain.t[n].view(torch.int32), st.t[n].view(torch.int32)), f"{label}: {n} differs from the call without a mask"
    # a last step over no new key would be another problem: finish with the state's own finalize, head by head
    for h in range(c.hq):
        ptrs = [st.t[n][h, r0:].data_ptr() for n in ("O", "L", "Oacc", "M")]
        assert _lib().fa2_forward_state_finalize(*ptrs, r1 - r0, d, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for k, v in B.check(f"{label} finalized", inside(st.result()), cut(ref)).items():
        report[k] = max(report.get(k, 0.0), v)
    assert (st.t["Oacc"].view(torch.int32)[:, :r0] == SENT32).all() and (st.t["O"].view(torch.int16)[:, r1:] == 0x7FA5).all()
    st.bands_are_nan(label)
    _report(label, report)


class _Cut:
    """Rows [r0, r1) of a step_rows_ref.Rows, as bf16_rows_ref.check reads a Case."""

    def __init__(self, rows, r0, r1, index=None):
        pick = (lambda x: x[:, r0:r1]) if index is None else (lambda x: x[:, index])
        self.regime, self.part, self.key_seen = rows.regime, {}, None
        self.ref = {n: pick(x) for n, x in rows.ref.items() if n in ("O", "L")}
        self.quad, self.rest = {"O": pick(rows.quad["O"])}, {"O": pick(rows.rest["O"])}
        self.l_gate, self.keyless = pick(rows.l_gate), pick(rows.keyless)

    gate = B.Case.gate


@pytest.mark.parametrize("d", B.HEAD_DIMS)
def test_the_two_step_shapes_of_the_zigzag_ring(d):
    """Rank 0: its own keys under the local causal mask, then all of rank 1's keys into the second half of its rows (the first half
    is finished by fa2_forward_state_finalize).  Rank 1: its own keys, then the first half of rank 0's keys into all rows, last."""
    for rank, (name, step, whole, rows) in enumerate(T.zigzag_steps(d)):
        c = step.case
        n = c.nq
        Q, K, V = (t.cuda() for t in c.t[:3])
        st = State(c.hq, n, d)
        _sentinel(st)
        label = f"zigzag {name} d{d}"
        _strided_step(Q, K, V, st, step.shards[0], d, c.s, True, False, n, c.nk)
        report = B.check(f"{label} after the own keys (state)", st.views(), step.rows(1))
        (r0, r1), _, _ = step.shards[1]
        _strided_step(Q, K, V, st, step.shards[1], d, c.s, False, True, n, c.nk)
        if rank == 0:                    # the rows the last step did not touch
            for h in range(c.hq):
                ptrs = [st.t[k][h].data_ptr() for k in ("O", "L", "Oacc", "M")]
                assert _lib().fa2_forward_state_finalize(*ptrs, r0, d, 0, torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
        for k, v in B.check(f"{label} against the causal problem", st.result(), _Cut(whole, 0, 0, rows)).items():
            report[k] = max(report.get(k, 0.0), v)
        st.bands_are_nan(label)
        _report(label, report)
