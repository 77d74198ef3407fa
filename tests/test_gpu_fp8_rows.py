"""GPU: the fp8 (e4m3) forward -- BASELINE configs[4] -- row by row against the float64 reference of tests/fp8_ref.py.

Where tests/test_gpu_fp8.py has one number per tensor, every row here has a gate of its own (fp8_ref.row_gate: what e4m3's
rounding of P, the flush below 2^-10 and the bf16 output can cost that row, derived from the number formats and certified on the
CPU by tests/test_fp8_reference.py), and L is gated per row (1e-4 on heads whose scaled scores stay within +-8, 1e-3 otherwise).
The caller owns O and L and fills them with NaN first: a row block that no workgroup computed cannot inherit an earlier result
from the allocator.  Order of the checks: no NaN left, the O gate on every row, the L gate on every row.  A failure names (case,
b, h, row), the ratio to the gate, and the failing rows per head and per 32-row group (a wave's rows) -- the pattern says which
mechanism broke: one 32-row group = a wave's mask or maxima, one 256-row block of one head = the block-to-head order, every row
from some length on = a ring round or a body.

  (a) length edges: one below, at and above 32 rows (a wave), 64 keys (a body), 128 (an LDS tile), 256 (a workgroup), 512 (a ring
      round) and 576 (a round and a body);  (b) the causal kernel's block-to-head remap in its three forms (B*H = 8: one head
      per XCD; 16: one pair; 24: a pair and a single), with B > 1, and B*H = 9 and 17 (no remap);  (c) six softmax regimes;
  (d) dominant keys on the first and last key of each ring round, heavy quiet keys, loud rows in lanes 0 and 31;
  (e) per-tensor descales;  (f) a dirty, reused workspace;  (g) guard bands around all five tensors.

Measured ratios per regime: DESIGN.md section 6b."""
import functools

import numpy as np
import pytest
import torch

import fp8_ref as F

pytestmark = pytest.mark.gpu

MASKS = (False, True)
_mask = lambda c: "causal" if c else "full"


def _fa():
    import cuda_flashattention_amd as fa
    return fa


def run(Q, K, V, s, causal, workspace=None, descale=None, O=None, L=None):
    """One call with caller-owned, NaN-filled O and L and a caller workspace.  Q, K, V: host or device e4m3 tensors."""
    fa = _fa()
    Q, K, V = (t.cuda() for t in (Q, K, V))
    B, H, N, d = Q.shape
    if O is None:
        O = torch.full((B, H, N, d), float("nan"), dtype=torch.bfloat16, device="cuda")
    if L is None:
        L = torch.full((B, H, N), float("nan"), dtype=torch.float32, device="cuda")
    if workspace is None:
        workspace = fa.ops.forward_fp8_workspace(B, H, N, d)
    O2, L2 = fa.flash_attention_2_forward(Q, K, V, s, causal=causal, O=O, L=L, workspace=workspace, descale=descale)
    torch.cuda.synchronize()
    assert O2 is O and L2 is L
    return O, L


def _pattern(bad):
    """'b h: rows per 32-row group' of a [B, H, N] mask of failing rows."""
    out = []
    for b, h in zip(*np.nonzero(bad.any(axis=-1))):
        rows = np.nonzero(bad[b, h])[0]
        groups = np.bincount(rows // 32)
        out.append(f"b{b} h{h}: {rows.size} rows, per 32-row group " + " ".join(f"{g}:{n}" for g, n in enumerate(groups) if n))
    return "; ".join(out[:12]) + (f"; ... {len(out)} heads in all" if len(out) > 12 else "")


def check(case, O, L, ref, V, l_gate=None):
    """The three checks in their order.  -> (largest ratio to the O gate, largest |dL|) for the report."""
    O, L = O.float().cpu().numpy(), L.cpu().numpy()
    nan = np.isnan(O).any(axis=-1) | np.isnan(L)
    assert not nan.any(), f"{case}: NaN left in O or L (never written?): {_pattern(nan)}"
    gate = F.row_gate(ref, V)
    lg = F.l_gate(ref) if l_gate is None else l_gate
    eo, el = F.row_errors(O, L, ref)
    for name, err, g in (("O", eo, gate), ("L", el, np.broadcast_to(lg, el.shape))):
        bad = err > g
        if bad.any():
            b, h, r = np.unravel_index(np.argmax(np.where(bad, err / g, 0.0)), err.shape)
            raise AssertionError(f"{case}: {name} row gate missed at (b {b}, h {h}, row {r}): error {err[b, h, r]:.3e} = "
                                 f"{err[b, h, r] / g[b, h, r]:.2f} x gate; {int(bad.sum())} rows fail: {_pattern(bad)}")
    ratio, dl = float((eo / gate).max()), float(el.max())
    print(f"FP8ROWS {case}: max O error / gate {ratio:.3f}  max|dL| {dl:.2e} (gate {float(np.max(lg)):.0e})")
    return ratio, dl


@functools.lru_cache(maxsize=2)
def _reference(regime, B, H, N, causal):
    Q, K, V, s = F.case_inputs(regime, B, H, N)
    return F.reference(Q, K, V, s, causal)


def _plain(regime, B, H, N, causal, label):
    Q, K, V, s = F.case_inputs(regime, B, H, N)
    O, L = run(Q, K, V, s, causal)
    return check(f"{label} {regime} B{B} H{H} N{N} {_mask(causal)}", O, L, _reference(regime, B, H, N, causal), V)


# ---- (a)
@pytest.mark.parametrize("regime", F.EDGE_REGIMES)
@pytest.mark.parametrize("causal", MASKS, ids=_mask)
@pytest.mark.parametrize("N", F.EDGE_N)
def test_length_edges(N, causal, regime):
    _plain(regime, 1, 2, N, causal, "edges")


# ---- (b)
@pytest.mark.parametrize("causal", MASKS, ids=_mask)
@pytest.mark.parametrize("B,H", F.ORDER_BH)
def test_block_to_head_order(B, H, causal):
    """N = 520: three row blocks, the last of 8 rows, a full ring round for the rows from 511.  Every head has its own data."""
    _plain(F.ORDER_REGIME, B, H, F.ORDER_N, causal, "order")


# ---- (c)
@pytest.mark.parametrize("causal", MASKS, ids=_mask)
@pytest.mark.parametrize("N", F.REGIME_N)
@pytest.mark.parametrize("regime", F.REGIMES)
def test_regimes(regime, N, causal):
    _plain(regime, 1, F.REGIME_H, N, causal, "regimes")


# ---- (d)
@pytest.mark.parametrize("causal", MASKS, ids=_mask)
def test_round_edges(causal):
    """fp8_ref.round_edge_inputs: dominant keys on the last and first key of each 512-key round (a key-norm lookup shifted by a
    block or a round runs that round without maxima), heavy quiet keys (their head keeps |dL| <= 1e-4: no reference moved late),
    loud rows in lanes 0 and 31 of the last wave."""
    Q, K, V, s = F.round_edge_inputs()
    ref = F.reference(Q, K, V, s, causal)
    assert F.l_gate(ref)[0, 1, 0] == F.L_GATE_SMALL
    for i, key in enumerate(F.ROUND_SPIKE_KEYS):
        assert ref["P"][0, 0, F.ROUND_N - 1 - i, key] > 0.99
    O, L = run(Q, K, V, s, causal)
    check(f"round-edges N{F.ROUND_N} {_mask(causal)}", O, L, ref, V)


# ---- (e)
@pytest.mark.parametrize("causal", MASKS, ids=_mask)
@pytest.mark.parametrize("regime", F.DESCALE_REGIMES)
def test_descaled_tensors(regime, causal):
    (Q8, K8, V8), desc, s, (q, k, v) = F.descaled_case(regime)
    assert max(float(t.float().abs().max()) for t in (Q8, K8, V8)) > 350.0          # the stored tensors use e4m3's range
    O, L = run(Q8, K8, V8, s, causal, descale=desc)
    check(f"descaled {regime} N{F.DESCALE_N} {_mask(causal)}", O, L, F.reference(q, k, v, s, causal), v)


@pytest.mark.parametrize("causal", MASKS, ids=_mask)
def test_power_of_two_descales_change_no_bit(causal):
    """Descales (2^-3, 2^2, 2^-1) against descales 1 and scale * 2^-1: the same L bit for bit, and O times 2^-1 exactly."""
    Q, K, V, s = F.case_inputs("scale-one", 1, F.DESCALE_H, F.DESCALE_N)
    dq, dk, dv = F.POW2_DESCALES
    O1, L1 = run(Q, K, V, s * dq * dk, causal, descale=(1.0, 1.0, 1.0))
    O2, L2 = run(Q, K, V, s, causal, descale=F.POW2_DESCALES)
    assert not torch.isnan(L1).any() and not torch.isnan(O1.float()).any()
    assert torch.equal(L1, L2)
    assert torch.equal((O1.float() * dv).bfloat16(), O2) and torch.equal(O1.float() * dv, O2.float())


# ---- (f)
def test_a_dirty_reused_workspace_is_harmless():
    """One workspace sized for the longest call and filled with 0xFF (a NaN as e4m3 and as fp32) serves N = 577, 130, 577: every
    result equals bit for bit the call on a fresh zeroed workspace and fa2_forward(dtype = fp8), the third equals the first."""
    fa = _fa()
    H, regime = F.WORKSPACE_H, F.WORKSPACE_REGIME
    ws = fa.ops.forward_fp8_workspace(1, H, max(F.WORKSPACE_NS), F.D)
    ws.fill_(0xFF)
    got = []
    for i, N in enumerate(F.WORKSPACE_NS):
        Q, K, V, s = (t.cuda() if isinstance(t, torch.Tensor) else t for t in F.case_inputs(regime, 1, H, N))
        O, L = run(Q, K, V, s, True, workspace=ws)
        check(f"workspace call {i} N{N}", O, L, _reference(regime, 1, H, N, True), F.case_inputs(regime, 1, H, N)[2])
        fresh = torch.zeros(fa._capi.lib().fa2_forward_fp8_workspace_bytes(1, H, N, F.D), dtype=torch.uint8, device="cuda")
        Of, Lf = run(Q, K, V, s, True, workspace=fresh)
        assert torch.equal(O, Of) and torch.equal(L, Lf), f"call {i} (N = {N}): the dirty workspace changed the result"
        Oa, La = torch.full_like(O, float("nan")), torch.full_like(L, float("nan"))
        fa.flash_attention_2_forward(Q, K, V, s, causal=True, O=Oa, L=La)          # no workspace=: fa2_forward(dtype = fp8)
        torch.cuda.synchronize()
        assert torch.equal(O, Oa) and torch.equal(L, La), f"call {i} (N = {N}): differs from fa2_forward(dtype = fp8)"
        got.append((O, L))
    assert torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[2][1])


# ---- (g)
def _guarded(nbytes, fill):
    """A device allocation of nbytes + two guard bands filled with `fill`; -> (whole buffer, the payload's byte view)."""
    buf = torch.full((nbytes + 2 * F.GUARD_BYTES,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[F.GUARD_BYTES:F.GUARD_BYTES + nbytes]


@pytest.mark.parametrize("causal", MASKS, ids=_mask)
@pytest.mark.parametrize("N", F.GUARD_NS)
def test_nothing_is_written_outside_o_and_l(N, causal):
    """Q, K, V (bands of 0x7F: NaN as e4m3), O and L (bands of 0xFF: NaN as bf16 and fp32) each inside a larger allocation with
    4096 bytes on either side: the gates hold (no input band was read into a result) and the output bands are untouched."""
    H, regime = F.GUARD_H, F.GUARD_REGIME
    Q, K, V, s = F.case_inputs(regime, 1, H, N)
    dev, keep = [], []
    for t in (Q, K, V):
        buf, view = _guarded(t.numel(), 0x7F)
        view.copy_(t.view(torch.uint8).reshape(-1).cuda())
        keep.append(buf)
        dev.append(view.view(torch.float8_e4m3fn).view(1, H, N, F.D))
    obuf, oview = _guarded(H * N * F.D * 2, 0xFF)
    lbuf, lview = _guarded(H * N * 4, 0xFF)
    O, L = oview.view(torch.bfloat16).view(1, H, N, F.D), lview.view(torch.float32).view(1, H, N)
    assert torch.isnan(O.float()).all() and torch.isnan(L).all()
    run(*dev, s, causal, O=O, L=L)
    check(f"guards N{N} {_mask(causal)}", O, L, _reference(regime, 1, H, N, causal), V)
    for name, buf in (("O", obuf), ("L", lbuf)):
        for side, band in (("below", buf[:F.GUARD_BYTES]), ("above", buf[-F.GUARD_BYTES:])):
            assert bool((band == 0xFF).all()), f"{name}: the guard band {side} was written (N = {N}, {_mask(causal)})"
    for buf, t in zip(keep, (Q, K, V)):
        assert bool((buf[:F.GUARD_BYTES] == 0x7F).all()) and bool((buf[-F.GUARD_BYTES:] == 0x7F).all())
        assert torch.equal(buf[F.GUARD_BYTES:-F.GUARD_BYTES].cpu(), t.view(torch.uint8).reshape(-1))
