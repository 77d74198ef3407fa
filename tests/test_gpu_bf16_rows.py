"""GPU: the bf16 forward and backward row by row against the float64 references of tests/bf16_rows_ref.py.

Where every other bf16 GPU test has one number per tensor (rel-L2 <= 5e-3), every row of O, dQ, dK and dV here has a gate of its
own (bf16_rows_ref.Case.gate: what bf16's rounding of P, of dS and of the output and the fp32 sums behind dS can cost that row;
derived from the number formats and certified on the CPU by tests/test_bf16_rows_reference.py, KAPPA = 2.5), and L is gated per
row (1e-4 where |L_ref| <= 25, else 1e-3).  The forward is judged against ref_attention on the bf16 inputs; the backward is
handed bf16(O_ref) and fp32(L_ref) and judged against ref_flow fed those two arrays.  The caller owns
every output and fills it with NaN before each call.  Order of the checks: no NaN left, the O / gradient gates on every row,
the L gate.  A failure names (case, tensor, b, h, row), the ratio to the gate, and the failing rows per head and per 32-row
group -- the pattern says which mechanism broke: one 32-row group = a sub-tile's mask or row constants, one 256-row block of
one head = the unit-to-head order or a hand-off, every row from some length on = the padding of a ragged length or a body.
`low-level` dQ, dK and `offsets` O, dV keep their tensor gates (why: tests/test_bf16_rows_reference.py).

Backward routes of a dense square problem: phases 7; 1 then 6; 8 | 1 wherever fa2_backward_plan says 1 (asserted against rule
(a) of include/fa2_mi355x.h, so a changed rule is noticed).  Rectangles: 7; 1 then 6.  Packed: the one route there is.  Grouped
heads on the single kernel: the dK / dV gates include the bf16 per-head partials (bf16_rows_ref's docstring).

  (a) length edges: one off a 32-row sub-tile, a 64-key tile, a 256-row workgroup / 256-key block, a d = 64 forward round (512),
      the single kernel's thresholds (768 / 897 at d = 64) and lengths padded to 1024 and 1280;  (b) unit and head order:
      B H = 8, 16, 24, 9, 17 with B > 1, three key blocks on the single kernel (N = 768) and N = 520;  (c) every regime of
      tests/regimes.py at N = 1024 and 1100;  (d) the qk, varlen and grouped-query entry points on the same checker;
  (e) a 0xFF-filled reused workspace (bit-equal to a fresh one) and 64-element NaN guard bands around all five outputs.

Every case prints one BF16ROWS line (pytest -s); DESIGN.md section 6c keeps the largest ratio per regime, entry point and tensor."""
import ctypes
import itertools

import pytest
import torch

import bf16_rows_ref as B
import regimes as R

pytestmark = pytest.mark.gpu

_mask = lambda c: "causal" if c else "full"
NAN = float("nan")


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def _plan_says(batch, hq, n, d, causal):
    return _fa()._capi.lib().fa2_backward_plan(batch, hq, n, d, 0, int(causal), ctypes.POINTER(ctypes.c_char_p)())


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ the calls
class Dense:
    """A Case on the device as [batch, H, N, d] tensors (batch > 1: the Case's heads are batch x H, multi-head only)."""

    def __init__(self, case, batch=1):
        self.case, self.batch = case, batch
        hq, hkv = case.hq // batch, case.hkv // batch
        shape = lambda t, h: t.reshape(batch, h, t.shape[1], *t.shape[2:]).contiguous().cuda()
        Q, K, V, dO = case.t
        self.Q, self.K, self.V, self.dO = shape(Q, hq), shape(K, hkv), shape(V, hkv), shape(dO, hq)
        self.O16, self.L32 = shape(case.O16, hq), shape(case.L32, hq)
        self.square = case.nq == case.nk
        self.heads = hq if batch > 1 else None

    def flat(self, t):
        return t.reshape(-1, *t.shape[2:])

    def forward(self, O=None, L=None):
        fa, c = _fa(), self.case
        O = _nan(self.Q.shape, torch.bfloat16) if O is None else O
        L = _nan(self.Q.shape[:3], torch.float32) if L is None else L
        call = fa.flash_attention_2_forward if self.square else fa.flash_attention_2_qk_forward
        O2, L2 = call(self.Q, self.K, self.V, c.s, causal=c.causal, O=O, L=L)
        torch.cuda.synchronize()
        assert O2 is O and L2 is L
        return {"O": self.flat(O), "L": self.flat(L)}

    def workspace(self):
        lib, c = _fa()._capi.lib(), self.case
        hq, hkv = c.hq // self.batch, c.hkv // self.batch
        if self.square:
            return lib.fa2_backward_gqa_workspace_bytes(self.batch, hq, hkv, c.nq, c.d, 0)
        return lib.fa2_backward_qk_workspace_bytes(self.batch, hq, hkv, c.nq, c.nk, c.d, 0)

    def backward(self, phases, workspace=None, out=None):
        fa, c = _fa(), self.case
        dQ, dK, dV = out or (_nan(self.Q.shape, torch.bfloat16), _nan(self.K.shape, torch.bfloat16), _nan(self.V.shape, torch.bfloat16))
        ws = torch.empty(self.workspace(), dtype=torch.uint8, device="cuda") if workspace is None else workspace
        call = fa.flash_attention_2_backward if self.square else fa.flash_attention_2_qk_backward
        for ph in phases:
            call(self.Q, self.K, self.V, self.O16, self.L32, self.dO, c.s, causal=c.causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph)
        torch.cuda.synchronize()
        return {"dQ": self.flat(dQ), "dK": self.flat(dK), "dV": self.flat(dV)}

    def routes(self):
        """[(phases, whether the single kernel runs)]; the plan is asserted against rule (a)."""
        c = self.case
        if not self.square:
            return [((7,), False), ((1, 6), False)]
        single = B.single_kernel(c.nq, c.d)
        says = _plan_says(self.batch, c.hq // self.batch, c.nq, c.d, c.causal)
        assert says == (1 if single else 2), f"fa2_backward_plan says {says} at N = {c.nq}, d = {c.d}: rule (a) has changed"
        return [((7,), single), ((1, 6), False)] + ([((9,), True)] if single else [])


def _merge(report, new):
    for n, v in new.items():
        report[n] = max(report.get(n, 0.0), v)


def _dense(label, case, batch=1):
    """The forward and every backward route of a dense case through the checker; one BF16ROWS line."""
    dev = Dense(case, batch)
    report = B.check(f"{label} forward", dev.forward(), case, heads=dev.heads)
    for phases, single in dev.routes():
        _merge(report, B.check(f"{label} phases {phases}", dev.backward(phases), case, partials=single and case.G > 1, heads=dev.heads))
    print(B.report_line(label, report))
    return report


def _square(regime, hq, hkv, n, d, causal, label, batch=1):
    return _dense(f"{label} {regime} B{batch} H{hq // batch}/{hkv // batch} N{n} d{d} {_mask(causal)}", B.dense_case(regime, hq, hkv, n, n, d, causal), batch)


# ---- (a)
@pytest.mark.parametrize("regime", B.EDGE_REGIMES)
@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("N", B.EDGE_N)
def test_length_edges(N, d, causal, regime):
    _square(regime, B.EDGE_H, B.EDGE_H, N, d, causal, "edges")


# ---- (b)
@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("N", B.ORDER_N)
@pytest.mark.parametrize("batch,H", B.ORDER_BH)
def test_unit_and_head_order(batch, H, N, d, causal):
    """N = 768: three key blocks on the single kernel at both head dims (causal heads are taken in groups of two); N = 520: the
    two kernels at d = 64.  Every head has its own data, so a block computed for the wrong head is wrong on every row."""
    assert B.single_kernel(768, d) and not B.single_kernel(520, 64)
    _square(B.ORDER_REGIME, batch * H, batch * H, N, d, causal, "order", batch)


# ---- (c)
@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("N", B.REGIME_N)
@pytest.mark.parametrize("regime", R.REGIMES)
def test_regimes(regime, N, d, causal):
    _square(regime, B.REGIME_H, B.REGIME_H, N, d, causal, "regimes")


# ---- (d)
@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("regime", B.OTHER_REGIMES)
@pytest.mark.parametrize("nq,nk", B.QK_SHAPES)
def test_rectangles_through_the_qk_calls(nq, nk, regime, d, causal):
    """(300, 1100) and (1100, 300): the bottom-right causal offset (+-800) is no multiple of 32 rows; at (1100, 300) causal the
    first 800 rows see no key."""
    hq, hkv = B.GQA_HEADS
    _dense(f"qk {regime} {nq}x{nk} d{d} {_mask(causal)}", B.dense_case(regime, hq, hkv, nq, nk, d, causal))


@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("regime", B.OTHER_REGIMES)
def test_grouped_heads(regime, d, causal):
    """8 query heads on 2 K/V heads at N = 1100: the single kernel with bf16 partials at d = 128, the two kernels at d = 64."""
    _square(regime, *B.GQA_HEADS, B.GQA_N, d, causal, "gqa")


@pytest.mark.parametrize("causal", B.MASKS, ids=_mask)
@pytest.mark.parametrize("d", B.HEAD_DIMS)
@pytest.mark.parametrize("regime", B.OTHER_REGIMES)
def test_a_packed_batch_through_the_varlen_calls(regime, d, causal):
    fa = _fa()
    case = B.packed_case(regime, B.PACKED, d, causal)
    cq, ck = ([0] + list(itertools.accumulate(x)) for x in zip(*B.PACKED))
    plan = fa.VarlenPlan(cq, ck)
    assert plan.two_sided
    Q, K, V, dO, O16, L32 = (t.contiguous().cuda() for t in case.t + (case.O16, case.L32))
    O, L = _nan(Q.shape, torch.bfloat16), _nan(Q.shape[:2], torch.float32)
    dQ, dK, dV = _nan(Q.shape, torch.bfloat16), _nan(K.shape, torch.bfloat16), _nan(V.shape, torch.bfloat16)
    fa.flash_attention_2_varlen_forward(Q, K, V, plan, case.s, causal=causal, O=O, L=L)
    fa.flash_attention_2_varlen_backward(Q, K, V, O16, L32, dO, plan, case.s, causal=causal, dQ=dQ, dK=dK, dV=dV)
    torch.cuda.synchronize()
    label = f"packed {regime} d{d} {_mask(causal)}"
    report = B.check(f"{label} forward", {"O": O, "L": L}, case)
    _merge(report, B.check(f"{label} backward", {"dQ": dQ, "dK": dK, "dV": dV}, case))
    print(B.report_line(label, report))


# ---- (e)
def _banded(shape, dtype):
    """A NaN-filled tensor inside a larger NaN-filled allocation: GUARD elements on either side.  -> (whole buffer, the view)."""
    n = 1
    for x in shape:
        n *= x
    buf = _nan((n + 2 * B.GUARD,), dtype)
    return buf, buf[B.GUARD:B.GUARD + n].view(shape)


@pytest.mark.parametrize("regime,H,N,d,causal", B.WORKSPACE_CASES)
def test_a_dirty_workspace_and_guard_bands(regime, H, N, d, causal):
    """The route the rule picks (phases 7: the single kernel at N = 1024, d = 128; the two kernels at N = 520, d = 64) on a
    0xFF-filled workspace, on the same workspace again, and on a fresh zeroed one: the same bits three times.  The outputs of the
    first run (and the forward's) lie between 64-element NaN bands, which stay NaN."""
    case = B.dense_case(regime, H, H, N, N, d, causal)
    dev = Dense(case)
    assert _plan_says(1, H, N, d, causal) == (1 if B.single_kernel(N, d) else 2) == (1 if N == 1024 else 2)
    label = f"workspace {regime} H{H} N{N} d{d} {_mask(causal)}"
    bands = {n: _banded(s, dt) for n, s, dt in (("O", dev.Q.shape, torch.bfloat16), ("L", dev.Q.shape[:3], torch.float32), ("dQ", dev.Q.shape, torch.bfloat16),
                                                ("dK", dev.K.shape, torch.bfloat16), ("dV", dev.V.shape, torch.bfloat16))}
    report = B.check(f"{label} forward", dev.forward(bands["O"][1], bands["L"][1]), case)
    ws = torch.full((dev.workspace(),), 0xFF, dtype=torch.uint8, device="cuda")
    first = dev.backward((7,), ws, tuple(bands[n][1] for n in B.GRADS))
    _merge(report, B.check(f"{label} dirty workspace", first, case))
    again = dev.backward((7,), ws)
    fresh = dev.backward((7,), torch.zeros(dev.workspace(), dtype=torch.uint8, device="cuda"))
    for n in B.GRADS:
        assert torch.equal(first[n], again[n]), f"{label}: {n} differs on the reused workspace"
        assert torch.equal(first[n], fresh[n]), f"{label}: {n} on the 0xFF-filled workspace differs from a fresh one"
    for n, (buf, view) in bands.items():
        assert not torch.isnan(view.float()).any(), n
        for side, band in (("below", buf[:B.GUARD]), ("above", buf[-B.GUARD:])):
            assert torch.isnan(band.float()).all(), f"{label}: the guard band {side} {n} was written"
    print(B.report_line(label, report))
