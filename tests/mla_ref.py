"""The MLA decode (fa2_forward_mla_decode / _paged) and the MLA latent-cache append (fa2_mla_kv_append / _paged) held to the
cache-side family's certified row gates (a helper module, no tests: tests/test_mla_rows_reference.py certifies what is here on
the CPU, tests/test_gpu_mla_rows.py runs the kernels on it).

THE PROBLEM (include/fa2_mla_mi355x.h).  Q [B, H, N_q, 576] against ONE latent cache row per token, C [B, N_cap, 576]: the score
uses all 576 columns, the value is C[..., :512] of the same row; sequence b attends keys [0, len_b), the N_q queries are its last
tokens (bottom-right causal mask); a row without a visible key has O = 0 and L = -inf.

REFERENCE (reference64): float64 on the bf16 inputs, the meaning of tests/test_gpu_mla_decode.py's _reference, a
decode_rows_ref.Ref whose .quad is quad64 on (C, C[..., :512]).

EMULATION (emulate): fa2_mla_decode.hip's data flow in NumPy fp32, in the style of decode_ref.emulate.  It differs from the
family's in three ways: the four waves split the COLUMNS (wave w owns latent columns [128 w, +128) and rotary columns
[512 + 16 w, +16)) and their partial S meet in fp32 in wave order 0..3 before the scale; ONE online softmax (m, l, o) runs per
split over consecutive 32-key tiles; a split starts on a multiple of 32 (chunk = roundup(ceil(len / n_splits), 32)).  The rest is
the family's: masked P selected to 0, l from the fp32 P, P rounded to bf16 for the second product, one output rounding with one
split, else fp32 partials (O_s, L_s), L_s = -inf for an empty split, folded in ascending s by fa2_mla_combine_kernel's arithmetic
with one rounding.  It follows the kernel's order of operations, not its bits.

INPUTS.  uniform_inputs: tests/test_gpu_mla_decode.py's _inputs, generator and all (the CPU file asserts the bits), at any
(H, N_q).  regime_inputs: `peaked`, `spikes`, `scale-one` and `low-level` of tests/regimes.py at d = 576, (H, N_q) = (11, 3):
M = 33, so head 10's last token is the one row of a second row block.  Amplitudes and scales are regimes._TABLE's with
s = 576^-1/2 where the table says None.  regimes.inputs cannot be called as it is: its spike assertion needs two K/V heads, and one
cache row is both K and V here.
  * spikes: the 28-unit key floor(0.28 n) is set for (head 1, token 0), the 130-unit key floor(0.82 n) for (head 10, token 2) --
    the row of the second block; every other row sees the two as keys of the shared cache like any other.
  * low-level: the offset sits in the ROTARY columns only, Q[..., 512:] = 3 + 0.25 (U - 1/2), C[..., 512:] = -(0.6 + 0.05 (U - 1/2))
    (regimes' own d = 64 numbers: 64 x 3 x 0.6 = 115); the 512 latent columns are zero-mean at the `scale-one` amplitude of d = 512.
    WHY NOT regimes' low-level over all 576 columns: V is K's first 512 columns, so V would be a near-constant -c, every element
    of O would round the same way, the output roundings add coherently and the emulation uses the whole row gate (0.99 to 1.05 of it
    over the variants tried on the CPU) -- a property of that input, not of a kernel.  The input was changed; the gate was not.

MUTANTS, built on the emulation and the bf16 inputs (what each breaks is what a plausible fault of THIS kernel would):
    a1  the score of the longest sequence leaves out the 64 rotary columns (a wave's ninth k-step)
    a2  one wave's 128 columns of O of the longest sequence come from the neighbouring wave's columns of V; L untouched
    a3  the causal kmax takes the row within the block (r % q_len), not rho % q_len
    a4  the second product of the longest sequence misses the last full 32-key tile of a MIDDLE split (V rows zeroed; L untouched)
    a5  an empty split's partial enters the combine with weight exp(0 - m): its -inf is read as 0

THE APPEND'S MODEL (append_model): the contract of include/fa2_mla_append_mi355x.h on host tensors, the one of
tests/test_gpu_mla_append.py with the capacity and the page size as arguments (the CPU file asserts that the two agree)."""
import functools

import numpy as np
import torch

import decode_ref as dr
import decode_rows_ref as rows
import qk_norm_ref as nr
import regimes
import rope_ref as rr

D, DV, ROPE = 576, 512, 64
TILE, WAVES = 32, 4              # kMlaTile: keys of a tile, rows of a block, a split's grain; kMlaWaves
WAVE_COLS = DV // WAVES          # latent columns of a wave
WAVE_ROPE = ROPE // WAVES        # rotary columns of a wave
MIN_SPLIT_KEYS, CUS, MAX_SPLITS = 256, 256, 256

# what tests/test_gpu_mla_decode.py runs (the CPU file asserts that these are that file's)
UNIFORM_CAP, UNIFORM_SCALE = 384, 0.0913
UNIFORM_LENS = (0, 1, 31, 32, 33, 127, 128, 129, 300, UNIFORM_CAP)
OLD_SHAPES = ((16, 1), (16, 2), (5, 3), (40, 1))
# (11, 3): M = 33, a head's tokens straddle the block edge; (2, 17): M = 34; (128, 1): four row blocks
NEW_SHAPES = ((11, 3), (2, 17), (128, 1))
UNIFORM_SPLITS = (0, 1, 2, 5)
FAR_SHAPE, FAR_LENS = (1, 1), (300, 33)      # the contiguous cache past 4 GiB: its last two sequences
FAR_B, FAR_CAP = 10, 466048                  # 10 x 466048 x 1152 bytes = 5.37 GB: sequences 8 and 9 start beyond byte 2^32

# the regime runs
REGIMES = ("peaked", "spikes", "scale-one", "low-level")
H, NQ = 11, 3
N_CAP, PAGE = 1120, 32
LENS = (300, 1100)
SPLITS = (1, 7, 0)
SPIKES = ((1, 0, 0), (H - 1, NQ - 1, 1))      # (head, token, which of regimes.SPIKE_SCORES)

_f32 = np.float32
_LOG2E, _LN2 = dr._LOG2E, dr._LN2
_bf16 = dr._bf16


def num_splits(B, H_, nq, ncap):
    """What n_splits = 0 stands for (fa2_mla_decode_num_splits)."""
    groups = B * -(-H_ * nq // TILE)
    return min(-(-CUS // groups), max(1, ncap // MIN_SPLIT_KEYS), MAX_SPLITS)


def split_range(n, n_splits, s):
    """Keys [begin, end) of split s of a sequence of n keys: the kernel's rule."""
    chunk = -(-(-(-n // n_splits)) // TILE) * TILE
    return s * chunk, min((s + 1) * chunk, n)


# ------------------------------------------------------------------------------------------------ the float64 reference
def reference64(Q, C, lens, scale, causal):
    """float64 O [B, H, nq, 512], L [B, H, nq] and the row gate's .quad: Q [B, H, nq, 576], C [B, ncap, 576] host bf16."""
    B, H_, nq, _ = Q.shape
    O, L = np.zeros((B, H_, nq, DV)), np.full((B, H_, nq), -np.inf)
    for b, n in enumerate(lens):
        n = int(n)
        if n <= 0:
            continue
        q, c = regimes.f64(Q[b]), regimes.f64(C[b, :n])
        s = scale * (q @ c.T)                                            # [H, nq, n]
        if causal:
            s = np.where(np.arange(n)[None, :] <= np.arange(nq)[:, None] + n - nq, s, -np.inf)
        m = s.max(axis=-1)
        seen = np.isfinite(m)
        p = np.exp(s - np.where(seen, m, 0.0)[..., None])
        l = p.sum(axis=-1)
        with np.errstate(divide="ignore"):
            L[b] = np.where(seen, m + np.log(np.where(seen, l, 1.0)), -np.inf)
        O[b] = (p / np.where(seen, l, 1.0)[..., None]) @ c[:, :DV]
    return rows.Ref(O, L, rows.quad64(Q, C[:, None], C[:, None, :, :DV], [int(n) for n in lens], scale, causal, None))


# ------------------------------------------------------------------------------------------------ the emulation
def _split_partial(q, k, v, kmax, begin, end, sc):
    """One split's normalised fp32 O_s [M, 512] and L_s [M]: q [M, 576], k [ncap, 576], v [ncap, 512] fp32, kmax [M]; begin < end."""
    M = q.shape[0]
    m, l, o = np.full(M, -np.inf, _f32), np.zeros(M, _f32), np.zeros((M, DV), _f32)
    cols = [np.r_[WAVE_COLS * w:WAVE_COLS * (w + 1), DV + WAVE_ROPE * w:DV + WAVE_ROPE * (w + 1)] for w in range(WAVES)]
    with np.errstate(invalid="ignore", divide="ignore"):
        for kb in range(begin, end, TILE):
            ke = min(kb + TILE, end)
            S = (q[:, cols[0]] @ k[kb:ke, cols[0]].T).astype(_f32)
            for w in range(1, WAVES):                                    # the partials meet in wave order, in fp32, before the scale
                S = S + (q[:, cols[w]] @ k[kb:ke, cols[w]].T).astype(_f32)
            S = S * sc
            vis = np.arange(kb, ke)[None, :] < kmax[:, None]
            m_new = np.maximum(m, np.where(vis, S, -np.inf).max(axis=-1).astype(_f32))
            m0 = np.where(np.isneginf(m_new), _f32(0.0), m_new)
            alpha = np.exp2(m - m0, dtype=_f32)
            p = np.where(vis, np.exp2(S - m0[:, None], dtype=_f32), _f32(0.0))
            l = l * alpha + p.sum(axis=-1, dtype=_f32)
            o = o * alpha[:, None] + (_bf16(p) @ v[kb:ke]).astype(_f32)
            m = m_new
        has = l > 0
        inv = _f32(1.0) / np.where(has, l, _f32(1.0))
        Os = np.where(has[:, None], o * inv[:, None], _f32(0.0)).astype(_f32)
        Ls = np.where(has, (m + np.log2(np.where(has, l, _f32(1.0)), dtype=_f32)) * _LN2, -np.inf).astype(_f32)
    return Os, Ls


def _flow(Q, K, V, lens, scale, causal, n_splits, row_in_block=False, empty_L=-np.inf):
    """emulate with the score side K [B, ncap, 576] and the value side V [B, ncap, 512] given apart, and the two faults a mutant
    cannot make from the inputs: row_in_block (a3) and empty_L (a5: what an empty split's L_s is read as)."""
    B, H_, nq, _ = Q.shape
    ncap, M = K.shape[1], H_ * nq
    sc = _f32(scale) * _LOG2E
    O, L = np.zeros((B, H_, nq, DV), _f32), np.zeros((B, H_, nq), _f32)
    rho = np.arange(M)                                                   # row rho of the slab: head rho // nq, token rho % nq
    token = (rho % TILE if row_in_block else rho) % nq
    for b in range(B):
        n = min(max(int(lens[b]), 0), ncap)
        q, k, v = Q[b].float().numpy().reshape(M, D), K[b].float().numpy(), V[b].float().numpy()
        kmax_all = (token + n - nq + 1) if causal else np.full(M, n)
        parts = []
        for s in range(n_splits):
            begin, end = split_range(n, n_splits, s)
            if begin >= end:
                parts.append((np.zeros((M, DV), _f32), np.full(M, empty_L, _f32)))
            else:
                parts.append(_split_partial(q, k, v, np.minimum(kmax_all, end), begin, end, sc))
        if n_splits == 1:
            Ob, Lb = parts[0]
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                m = np.maximum.reduce([p[1] for p in parts])
                m0 = np.where(np.isneginf(m), _f32(0.0), m)
                tot, acc = np.zeros(M, _f32), np.zeros((M, DV), _f32)
                for Os, Ls in parts:                                     # ascending s
                    has = ~np.isneginf(Ls)
                    w = np.where(has, np.exp2((Ls - m0) * _LOG2E, dtype=_f32), _f32(0.0))
                    tot, acc = tot + w, acc + w[:, None] * Os
                none = np.isneginf(m)
                inv = _f32(1.0) / np.where(none, _f32(1.0), tot)
                Lb = np.where(none, -np.inf, m + np.log2(np.where(none, _f32(1.0), tot), dtype=_f32) * _LN2).astype(_f32)
                Ob = np.where(none[:, None], _f32(0.0), acc * inv[:, None]).astype(_f32)
        O[b], L[b] = _bf16(Ob).reshape(H_, nq, DV), Lb.reshape(H_, nq)
    return O, L


def emulate(Q, C, lens, scale, causal, n_splits):
    """The MLA kernels' data flow on the CPU: O (bf16 values as fp32) [B, H, nq, 512] and L fp32 [B, H, nq] for an explicit
    n_splits >= 1; Q [B, H, nq, 576] and C [B, ncap, 576] host bf16, lens clamped to [0, ncap] as the kernel does."""
    return _flow(Q, C, C[..., :DV], lens, scale, causal, n_splits)


# ------------------------------------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def uniform_inputs(H_, nq):
    """tests/test_gpu_mla_decode.py's _inputs at any (H, nq): Q [B, H, nq, 576] (scores of standard deviation 2) and the latent
    cache [B, 384, 576], finite everywhere; the last two sequences start with the same 96 rows."""
    B = len(UNIFORM_LENS)
    g = torch.Generator().manual_seed(576 + 7 * H_ + nq)
    Q = ((torch.rand(B, H_, nq, D, generator=g) - 0.5) * 12).bfloat16()
    C = (torch.rand(B, UNIFORM_CAP, D, generator=g) - 0.5).bfloat16()
    C[B - 1, :96] = C[B - 2, :96]
    return Q, C


@functools.lru_cache(maxsize=None)
def uniform_reference(H_, nq, causal):
    return reference64(*uniform_inputs(H_, nq), UNIFORM_LENS, UNIFORM_SCALE, causal)


@functools.lru_cache(maxsize=None)
def far_inputs():
    """Q [2, 1, 1, 576] and the first 384 cache rows [2, 384, 576] of the two sequences of FAR_LENS: what the last two sequences
    of the contiguous cache past 4 GiB hold (uniform_inputs' distributions)."""
    g = torch.Generator().manual_seed(4 << 10)
    return ((torch.rand(2, 1, 1, D, generator=g) - 0.5) * 12).bfloat16(), (torch.rand(2, UNIFORM_CAP, D, generator=g) - 0.5).bfloat16()


@functools.lru_cache(maxsize=None)
def far_reference(causal):
    return reference64(*far_inputs(), FAR_LENS, UNIFORM_SCALE, causal)


def scale_of(regime):
    s = regimes._TABLE[regime][0]
    return 1.0 / D ** 0.5 if s is None else s


def _amplitude(s, sigma, d):
    return (12.0 * sigma / (s * d ** 0.5)) ** 0.5


def _sequence(regime, n):
    """Host bf16 Q [H, NQ, 576] and the n cache rows [n, 576] of one sequence of a regime (the module's docstring)."""
    s, sigma = scale_of(regime), regimes._TABLE[regime][1]
    gen = torch.Generator().manual_seed(576000 + 1009 * REGIMES.index(regime) + 3 * n)
    uq = torch.rand(H, NQ, D, generator=gen, dtype=torch.float64) - 0.5
    uc = torch.rand(n, D, generator=gen, dtype=torch.float64) - 0.5
    if regime == "low-level":
        a = _amplitude(s, regimes._TABLE["scale-one"][1], DV)
        Q, C = uq * a, uc * a
        Q[..., DV:], C[..., DV:] = 3.0 + 0.25 * uq[..., DV:], -(0.6 + 0.05 * uc[..., DV:])
    else:
        a = _amplitude(s, sigma, D)
        Q, C = uq * a, uc * a
    Q, C = Q.bfloat16(), C.bfloat16()
    if regime == "spikes":
        C = C.double()
        for (h, r, i), j in zip(SPIKES, spike_keys(n)):
            q = Q[h, r].double()
            C[j] = q * (regimes.SPIKE_SCORES[i] / (s * float(q @ q)))
        C = C.bfloat16()
    return Q, C


def spike_keys(n):
    """The keys of the 28-unit and of the 130-unit spike in a sequence of n keys (regimes.spike_rows' places)."""
    return int(0.28 * n), int(0.82 * n)


def spike_rows(causal):
    """[((b, h, r), i)]: the rows of the regime batch that see spike i under the mask."""
    return [((b, h, r), i) for b, n in enumerate(LENS) for (h, r, i), j in zip(SPIKES, spike_keys(n)) if not causal or j <= r + n - NQ]


@functools.lru_cache(maxsize=None)
def regime_inputs(regime):
    """Host tensors (made once, never written): Q [2, 11, 3, 576], the cache [2, 1120, 576] whose rows past a length hold finite
    garbage, the scale, the lengths int32."""
    g = torch.Generator().manual_seed(577000 + REGIMES.index(regime))
    C = ((torch.rand(len(LENS), N_CAP, D, generator=g) - 0.5) * 8.0).bfloat16()
    Qs = []
    for b, n in enumerate(LENS):
        q, c = _sequence(regime, n)
        Qs.append(q)
        C[b, :n] = c
    return torch.stack(Qs), C, float(scale_of(regime)), torch.tensor(LENS, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def regime_reference(regime, causal):
    Q, C, scale, lens = regime_inputs(regime)
    return reference64(Q, C, lens.tolist(), scale, causal)


def paged(C, lens, P, seed, fill=float("nan")):
    """(pool [n_pages, P, 576], table int32 [B, ncap / P]) of the host cache C: shuffled pages, three spare; page p of sequence b
    holds its rows p P ..+P up to the length and `fill` past it and in the spare pages."""
    B, ncap, _ = C.shape
    mp = ncap // P
    table = torch.randperm(B * mp + 3, generator=torch.Generator().manual_seed(seed))[:B * mp].to(torch.int32).view(B, mp)
    pool = torch.full((B * mp + 3, P, D), fill, dtype=torch.bfloat16)
    for b, n in enumerate(lens):
        for p in range(mp):
            if p * P < n:
                pool[table[b, p], :min(P, n - p * P)] = C[b, p * P:min((p + 1) * P, n)]
    return pool, table


# ------------------------------------------------------------------------------------------------ the gates per row
def l_ratios(L, ref):
    """|dL| over decode_ref's L gate per row (1e-4 where |L_ref| <= 25, 1e-3 above); inf where the -inf rows differ."""
    rL = ref[1]
    L = np.asarray(L, dtype=np.float64)
    none = np.isneginf(rL)
    with np.errstate(invalid="ignore"):
        r = np.abs(L - rL) / np.where(np.abs(rL) <= dr.L_LARGE, dr.L_ABS, dr.L_ABS_LARGE)
    return np.where(none, np.where(np.isneginf(L), 0.0, np.inf), np.where(np.isfinite(L), r, np.inf))


# ------------------------------------------------------------------------------------------------ the mutants
def longest(lens):
    return int(np.argmax(lens))


def a1_no_rotary_columns(Q, C, lens, scale, causal, n_splits):
    """(a1) -> (O, L, b): the longest sequence's score over the 512 latent columns alone."""
    b = longest(lens)
    Q = Q.clone()
    Q[b, ..., DV:] = 0.0
    return emulate(Q, C, lens, scale, causal, n_splits) + (b,)


def a2_neighbours_columns(Q, C, lens, scale, causal, n_splits, wave=1):
    """(a2) -> (O, L, b): columns [128 wave, +128) of the longest sequence's O come from the next wave's columns of V; L untouched."""
    b = longest(lens)
    V = C[..., :DV].clone()
    V[b, :, WAVE_COLS * wave:WAVE_COLS * (wave + 1)] = C[b, :, WAVE_COLS * (wave + 1):WAVE_COLS * (wave + 2)]
    return _flow(Q, C, V, lens, scale, causal, n_splits) + (b,)


def a3_row_within_the_block(Q, C, lens, scale, causal, n_splits):
    """(a3) -> (O, L): the causal kmax from r % q_len, r the row within its 32-row block."""
    return _flow(Q, C, C[..., :DV], lens, scale, causal, n_splits, row_in_block=True)


def a3_touched(H_, nq, lens):
    """[B, H, nq] bool: the rows whose token a3 gets wrong, in the sequences with a key."""
    rho = np.arange(H_ * nq)
    wrong = ((rho % TILE) % nq != rho % nq).reshape(H_, nq)
    return np.asarray([n > 0 for n in lens])[:, None, None] & wrong[None]


def a4_middle_split_tile(Q, C, lens, scale, causal, n_splits):
    """(a4) -> (O, L, b, first key): V's rows of the last full 32-key tile of split n_splits // 2 of the longest sequence zeroed."""
    b = longest(lens)
    s = n_splits // 2
    begin, end = split_range(int(lens[b]), n_splits, s)
    assert 0 < s < n_splits - 1 and end - begin >= TILE and split_range(int(lens[b]), n_splits, s + 1)[0] < int(lens[b])
    t0 = begin + ((end - begin) // TILE - 1) * TILE
    V = C[..., :DV].clone()
    V[b, t0:t0 + TILE] = 0.0
    return _flow(Q, C, V, lens, scale, causal, n_splits) + (b, t0)


def a5_empty_split_read_as_zero(Q, C, lens, scale, causal, n_splits):
    """(a5) -> (O, L, [b with an empty split and a key]): an empty split's L_s read as 0, its O_s = 0 weighed by exp(0 - m)."""
    touched = [b for b, n in enumerate(lens) if n > 0 and any(split_range(int(n), n_splits, s)[0] >= int(n) for s in range(n_splits))]
    return _flow(Q, C, C[..., :DV], lens, scale, causal, n_splits, empty_L=0.0) + (touched,)


# ------------------------------------------------------------------------------------------------ the append's model
APPEND_SENTINEL = -1234.0


def append_sources(B, H_, n_new, seed):
    """The fused host tensors the views are cut from: kv [B, n_new, 1536 + 576], q [B, n_new, H, 192], nope [H, B n_new, 512],
    in (-3, 3) (tests/test_gpu_mla_append.py's _sources without its zero token)."""
    g = torch.Generator().manual_seed(seed)
    return tuple(((torch.rand(s, generator=g) - 0.5) * 6).bfloat16() for s in ((B, n_new, 2112), (B, n_new, H_, 192), (H_, B * n_new, 512)))


def append_views(kv, q, nope):
    """(q_nope [B, H, n_new, 512], q_pe [B, H, n_new, 64], kv_new [B, n_new, 576]) as strided views of append_sources."""
    B, n_new = kv.shape[:2]
    return nope.view(nope.shape[0], B, n_new, 512).permute(1, 0, 2, 3), q[..., 128:].permute(0, 2, 1, 3), kv[..., 1536:]


def append_model(cache, table, views, lens, w, cos, sin, interleaved, eps=nr.EPS):
    """The contract on host tensors, IN PLACE on the cache [B, cap, 576] (table None) or the pool [n_pages, P, 576] behind
    table [B, max_pages]; returns Q_out, or None without queries.  pos = len - n_new + t; a row is written iff 0 <= pos < cap and
    (paged) its table entry lies in [0, n_pages); every Q_out row is written, +0.0 for a dropped position."""
    q_nope, q_pe, kv = views
    B, n_new = kv.shape[:2]
    cap = cache.shape[1] if table is None else table.shape[1] * cache.shape[1]
    P = cache.shape[1]
    latent = nr.rms_rows(kv[..., :DV], w, eps)
    Q_out = None if q_nope is None else torch.zeros(B, q_nope.shape[1], n_new, D, dtype=torch.bfloat16)
    for b in range(B):
        for t in range(n_new):
            pos = int(lens[b]) - n_new + t
            if not 0 <= pos < cap:
                continue
            if Q_out is not None:
                Q_out[b, :, t] = torch.cat((q_nope[b, :, t], rr.rotate_bf16(q_pe[b, :, t], cos[pos], sin[pos], interleaved)), dim=-1)
            row = torch.cat((latent[b, t], rr.rotate_bf16(kv[b, t, DV:], cos[pos], sin[pos], interleaved)))
            if table is None:
                cache[b, pos] = row
            elif 0 <= int(table[b, pos // P]) < cache.shape[0]:
                cache[int(table[b, pos // P]), pos % P] = row
    return Q_out
