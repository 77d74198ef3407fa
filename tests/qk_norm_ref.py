"""The ragged rotary KV-cache append with a per-head QK RMSNorm in front of the rotation (fa2_norm_rope_kv_append_ragged, _paged;
include/fa2_rope_norm_mi355x.h) as a model of the whole contract (a helper module, no tests: tests/test_qk_norm_reference.py
certifies what is here, tests/test_gpu_qk_norm.py runs the kernels against it).

THE MODEL is written from the header's words (ARITHMETIC, steps 1-5), in numpy float32 with ONE numpy operation per rounding:
    q = x * x                                            (x: the bf16 row widened to float32, exact)
    per chunk of eight, left to right: s = q0 + q1; s = s + q2; ... s = s + q7
    a butterfly over the row's d / 8 chunks: for m = 1, 2, 4 (8): s = s + s[lane ^ m]; every lane ends with the same bits
    r = np.float32(1) / np.sqrt(s * np.float32(1 / d) + np.float32(eps))
    n = ((x * r) * w) rounded ONCE to bf16, to nearest even
ragged_append normalises the Q and K sources with it and hands over to rope_ragged_ref.ragged_append: the call is the sibling
applied to the normalised bf16 tensors, V untouched.
MUTANTS: wrong models that differ from the contract in one word each (`mutant=`).  FORMS: other ways to evaluate the same
formula (`form=`), for the witness search."""
import contextlib
import functools

import numpy as np
import torch

import rope_ragged_ref as gr
import rope_ref as rr

EPS = 0.05                                      # large enough that leaving it out, or adding it elsewhere, changes most elements
MUTANTS = ("swapped_weights", "weight_column_off_by_8", "eps_outside_sqrt", "weight_before_r", "norm_after_rotation",
           "no_round_before_rotation", "v_normalised", "mean_over_rot_dim")
# sequential_sum: the d squares summed left to right in one chain.  contracted_squares: fma(x_i, x_i, s) for the lane's sum, the
# exact square added and rounded once (evaluated in float64).  contracted_scale: x * r * w evaluated in float64 and rounded
# once to fp32, the rounding of x * r left out.  weight_before_r: fl(fl(x * w) * r), the mutant of that name, which differs from
# the contract in the last fp32 bit only and therefore shows on searched rows alone.
FORMS = ("sequential_sum", "contracted_squares", "contracted_scale", "weight_before_r")
F32 = np.float32


def lane_sums(xf):
    """Steps 1 and 2 on float32 rows [..., d]: [..., d / 8], each chunk's eight squares summed left to right."""
    q = xf * xf
    q = q.reshape(xf.shape[:-1] + (xf.shape[-1] // 8, 8))
    s = q[..., 0]
    for k in range(1, 8):
        s = s + q[..., k]
    return s


def butterfly(s):
    """Step 3 on [..., lanes]: every lane adds its partner's value, m = 1, 2, 4, ...; returns all lanes."""
    lanes = np.arange(s.shape[-1])
    m = 1
    while m < s.shape[-1]:
        s = s + s[..., lanes ^ m]
        m <<= 1
    return s


def _sum_squares(xf, form):
    if form == "sequential_sum":
        q = xf * xf
        s = q[..., 0]
        for k in range(1, xf.shape[-1]):
            s = s + q[..., k]
        return s[..., None]
    if form == "contracted_squares":
        xd = xf.astype(np.float64).reshape(xf.shape[:-1] + (xf.shape[-1] // 8, 8))
        s = (xd[..., 0] * xd[..., 0]).astype(F32)
        for k in range(1, 8):
            s = (s.astype(np.float64) + xd[..., k] * xd[..., k]).astype(F32)
        return butterfly(s)[..., :1]
    s = butterfly(lane_sums(xf))
    assert (s.view(np.int32) == s[..., :1].view(np.int32)).all(), "the butterfly leaves every lane of a row the same bits"
    return s[..., :1]


def rms_rows(x, w, eps, form=None, mutant=None, rot=None, rounded=True):
    """x: bf16 torch rows [..., d] (any strides); w: fp32 torch [d]; eps: a Python float.  Returns the normalised rows, bf16 and
    contiguous (rounded=False: the fp32 values before the one rounding)."""
    assert form is None or form in FORMS
    d = x.shape[-1]
    xf = x.float().contiguous().numpy()
    wf = w.contiguous().numpy().astype(F32)
    assert xf.dtype == F32 and wf.shape == (d,)
    part, n_mean = xf, d
    if mutant == "mean_over_rot_dim":
        part, n_mean = xf[..., :rot], rot
    s = _sum_squares(part, form)
    mean = s * F32(1.0 / n_mean)
    if mutant == "eps_outside_sqrt":
        r = F32(1) / (np.sqrt(mean) + F32(eps))
    else:
        v = mean + F32(eps)
        r = F32(1) / np.sqrt(v)
    if mutant == "weight_before_r" or form == "weight_before_r":
        n = (xf * wf) * r
    elif form == "contracted_scale":
        n = (xf.astype(np.float64) * r.astype(np.float64) * wf.astype(np.float64)).astype(F32)
    else:
        a = xf * r
        n = a * wf
    assert n.dtype == F32
    n = torch.from_numpy(np.ascontiguousarray(n))
    return n.bfloat16() if rounded else n


@contextlib.contextmanager
def _rotation(fn):
    """rope_ref.rotate_bf16 replaced for the two mutants that change what the rotation sees."""
    keep = rr.rotate_bf16
    rr.rotate_bf16 = fn
    try:
        yield keep
    finally:
        rr.rotate_bf16 = keep


def ragged_append(Q, K_new, V_new, K, V, table, cos, sin, q_weight, k_weight, eps, cu, lens, interleaved=False, k_descale=None,
                  v_descale=None, mutant=None):
    """The call on host tensors, IN PLACE on the caches (table None) or the pools: rope_ragged_ref.ragged_append's arguments with
    q_weight, k_weight, eps behind sin.  Returns (Q_out or None, the lists of written tokens)."""
    assert mutant is None or mutant in MUTANTS
    rot = 0 if cos is None else 2 * cos.shape[-1]
    if mutant == "swapped_weights":
        q_weight, k_weight = k_weight, q_weight
    if mutant == "weight_column_off_by_8":
        q_weight, k_weight = (None if w is None else torch.roll(w, 8) for w in (q_weight, k_weight))
    if mutant in ("norm_after_rotation", "no_round_before_rotation"):
        assert rot, "these mutants need a rotation"

        def patched(w, keep):
            if mutant == "norm_after_rotation":
                return lambda x, c, s, il: rms_rows(keep(x, c, s, il), w, eps)
            return lambda x, c, s, il: rr.rotate(rms_rows(x, w, eps, rounded=False), c.float(), s.float(), il).bfloat16()

        keep = rr.rotate_bf16
        with _rotation(patched(k_weight, keep)):
            _, written = gr.ragged_append(None, K_new, V_new, K, V, table, cos, sin, cu, lens, interleaved, k_descale, v_descale)
        q_out = None
        if Q is not None:
            with _rotation(patched(q_weight, keep)):
                q_out, _ = gr.ragged_append(Q, K_new, V_new, K.clone(), V.clone(), table, cos, sin, cu, lens, interleaved, k_descale,
                                            v_descale)
        return q_out, written
    inner = mutant if mutant in ("eps_outside_sqrt", "weight_before_r", "mean_over_rot_dim") else None
    qn = None if Q is None else rms_rows(Q, q_weight, eps, mutant=inner, rot=rot)
    kn = rms_rows(K_new, k_weight, eps, mutant=inner, rot=rot)
    vn = rms_rows(V_new, k_weight, eps) if mutant == "v_normalised" else V_new
    return gr.ragged_append(qn, kn, vn, K, V, table, cos, sin, cu, lens, interleaved, k_descale, v_descale)


def weights(d, seed):
    """(q_weight, k_weight): fp32 [d] each, 2 d DISTINCT magnitudes in (0.5, 1.5) -- so a wrong column or the other tensor's
    weight changes bits --, a few entries negative (a signed zero then follows the weight's sign)."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * d
    v = ((torch.randperm(n, generator=g).double() + 0.25 + 0.5 * torch.rand(n, generator=g).double()) / n + 0.5).float()
    assert v.unique().numel() == n and (v > 0.5).all() and (v < 1.5).all()
    for i in (3, 13, d - 1, d + 0, d + 9, n - 6):
        v[i] = -v[i]
    return v[:d].contiguous(), v[d:].contiguous()


# ---- the inputs tests/test_gpu_qk_norm.py runs on (the certification's mutants must change bytes on THESE)
ZERO_TOKEN = 5                                  # owned and live in PLACEMENT (sequence 2), in HOSTILE and in MANY


def source(d, seed, T=gr.T):
    """rope_ragged_ref.source with ONE all-zero token (every Q, K and V head; a few of the zeros negative): r = 1 / sqrt(eps)
    there, and the signed zeros of n follow the signs of x and w."""
    x = gr.source(d, seed, T=T)
    x[ZERO_TOKEN] = 0
    x.view(torch.int16)[ZERO_TOKEN, :, 2::5] = -0x8000
    return x


WITNESS_ROWS = 1 << 15


WEIGHT_SEED = 77                                # the weights of the GPU tests and of the witness search: weights(d, WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def witnesses(d, head, seed=2025, rows=WITNESS_ROWS):
    """Rows that tell the contract from another evaluation of the same formula.  A seeded search over `rows` = 2^15 rows of d bf16
    elements in (-3, 3), normalised with the GPU tests' weight of that kind of head ("q" or "k") and EPS: {form: the rows [n, d] whose bf16 result differs between the
    contract and that form}, for every form of FORMS.  Such rows are rare -- r moves by an fp32 ulp, and a bf16 result changes
    only where the fp32 value lies within that ulp of a rounding boundary, about one element in 2^15 -- which is why they are
    searched for.  contracted_squares yields NONE, at any number of draws: the square of a bf16 value has 16 significant bits
    and is exact in fp32, so fma(x, x, s) and fl(fl(x * x) + s) are the same number; the form is therefore not among the
    witness forms the GPU test places (tests/test_qk_norm_reference.py asserts that the search finds none)."""
    w = weights(d, WEIGHT_SEED)[("q", "k").index(head)]
    g = torch.Generator().manual_seed(seed + d + ("q", "k").index(head))
    x = ((torch.rand(rows, d, generator=g) - 0.5) * 6).bfloat16()
    want = rms_rows(x, w, EPS).view(torch.int16)
    out = {}
    for form in FORMS:
        other = rms_rows(x, w, EPS, form=form).view(torch.int16)
        out[form] = x[(want != other).any(dim=-1)].clone()
    return out


WITNESS_FORMS = ("sequential_sum", "contracted_scale", "weight_before_r")      # the forms of FORMS that yield witnesses
WITNESS_CASE = dict(cu=(0, gr.T), lens=(40,))   # ONE sequence owns every token: rows 12 .. 39 of its cache


def witness_source(d, seed):
    """The fused [T, H_q + 2 H_kv, d] source of the witness test: every Q row a witness found with q_weight, every K row one found
    with k_weight, the forms of WITNESS_FORMS taking turns (a form's rows repeat where it has fewer than its share); V random."""
    x = gr.source(d, seed)
    for head, lo, hi in (("q", 0, gr.HQ), ("k", gr.HQ, gr.HQ + gr.HKV)):
        found = witnesses(d, head)
        slot = 0
        for t in range(gr.T):
            for h in range(lo, hi):
                rows = found[WITNESS_FORMS[slot % len(WITNESS_FORMS)]]
                x[t, h] = rows[(slot // len(WITNESS_FORMS)) % rows.shape[0]]
                slot += 1
    return x
