"""The ragged rotary-embedding KV-cache append (fa2_rope_kv_append_ragged, _paged; include/fa2_rope_ragged_mi355x.h) as a model of
the whole contract (a helper module, no tests: tests/test_rope_ragged_reference.py certifies what is here,
tests/test_gpu_rope_ragged.py runs the kernels against it, tests/test_rope_ragged_owner.py the owner header).

THE MODEL is written from the contract's words and from the models the siblings already have, not from the product's code:
    owners: extend_ragged_ref.sanitised(cu, T) gives (start_b, q_b); packed token t belongs to the b with start_b <= t < start_b + q_b
    per sequence with q_b > 0: rope_ref.rope_append (rope_append_paged) with n_new = q_b on the sequence's cache slice (its table
        row) and on the [1, H, q_b, d] transposed slice of the token-major sources, at the length lens[b]
    Q_out [T, H_q, d]: the sibling's rows for owned tokens (rotated, or +0.0 where the position has no row), +0.0 throughout for
        a token no sequence owns; EVERY row is written
    rot_dim = 0 (cos = sin = None): tables of zero columns -- rope_ref.rotate_bf16 then keeps every element's bits
MUTANTS, for the certification: wrong models that differ from the contract in one word each (`mutant=`)."""
import torch

import extend_ragged_ref as xr
import rope_ref as rr

MUTANTS = ("start_off_by_one", "neighbours_q", "position_from_T", "unowned_unwritten", "raw_cu")


def owners(cu, T):
    """[(b, t - start_b, q_b) or None] for t in 0 .. T - 1 of ANY list of B + 1 ints, through the sanitised pairs."""
    out = [None] * T
    for b, (start, q) in enumerate(xr.sanitised(cu, T)):
        for i in range(q):
            assert out[start + i] is None
            out[start + i] = (b, i, q)
    return out


def _pairs(cu, T, mutant):
    seq = xr.sanitised(cu, T)
    if mutant == "raw_cu":
        seq = [(int(cu[b]), int(cu[b + 1]) - int(cu[b])) for b in range(len(cu) - 1)]
        seq = [(s, q) if s >= 0 and q > 0 and s + q <= T else (0, 0) for s, q in seq]      # (a model must stay inside its tensors)
    if mutant == "start_off_by_one":
        seq = [(s + 1, q) if s + 1 + q <= T else (s, q) for s, q in seq]
    return seq


def ragged_append(Q, K_new, V_new, K, V, table, cos, sin, cu, lens, interleaved=False, k_descale=None, v_descale=None, mutant=None,
                  Q_out=None):
    """The call on host tensors, IN PLACE on the caches (table None) or the pools.  Q [T, H_q, d] or None, K_new, V_new
    [T, H_kv, d] (any strides); cu: B + 1 ints; lens: B ints, the lengths after the append.  Returns (Q_out [T, H_q, d] or None,
    the siblings' lists of written tokens, one list per sequence).  Q_out=: the tensor a call would have found there (only the
    mutant that leaves rows unwritten shows it)."""
    assert mutant is None or mutant in MUTANTS
    T = K_new.shape[0]
    cap = K.shape[2] if table is None else table.shape[1] * K.shape[2]
    if cos is None:
        cos = sin = torch.zeros(cap, 0)
    seq = _pairs(cu, T, mutant)
    out = None
    if Q is not None:
        out = torch.zeros(Q.shape, dtype=torch.bfloat16)
        if mutant == "unowned_unwritten" and Q_out is not None:
            out = Q_out.clone()
    written = []
    for b, (start, q) in enumerate(seq):
        if q <= 0:
            written.append([])
            continue
        rows = slice(start, start + q)
        qb, kb, vb = (None if x is None else x[rows].permute(1, 0, 2)[None] for x in (Q, K_new, V_new))
        n = q
        if mutant == "neighbours_q":
            n = seq[(b + 1) % len(seq)][1]
        if mutant == "position_from_T":
            n = T
        # the sibling places token i at len - n_new + i: a length of len - q + n makes its n_new the mutant's n and leaves the model
        # itself (n = q) at len
        length = [int(lens[b]) - n + q]
        if table is None:
            q_ref, w = rr.rope_append(qb, kb, vb, K[b:b + 1], V[b:b + 1], cos, sin, length, interleaved, k_descale, v_descale)
        else:
            q_ref, w = rr.rope_append_paged(qb, kb, vb, K, V, table[b:b + 1], cos, sin, length, interleaved, k_descale, v_descale)
        written.append(w)
        if out is not None:
            out[rows] = q_ref[0].permute(1, 0, 2)
    return out, written


# ---- the inputs tests/test_gpu_rope_ragged.py runs on (the certification's mutants must change bytes on THESE)
HQ, HKV, CAP, PAGE, MAX_PAGES, N_PAGES, T = 4, 2, 96, 32, 3, 16, 28
UNUSED = (-1, 0x7FFFFFFF)                      # what table entries no written row needs hold
# q = 0, 1, 19, 5; token 0 and tokens 26, 27 un-owned; the 8-token group 0..7 holds an un-owned token and two sequences
PLACEMENT = dict(cu=(1, 1, 2, 21, 26), lens=(40, 1, 50, 96))      # row 0, rows 31..49 across a page, a sequence ending on the last row
# a negative position (len 0, q 1), nine leading tokens before row 0 (len 10, q 19), rows 94..98 of 96: 94 and 95 written
DROPS = dict(cu=(1, 1, 2, 21, 26), lens=(5, 0, 10, 99))
# not non-decreasing, out of range: sanitised to (5, 0), (5, 23), (28, 0), (28, 0)
HOSTILE = dict(cu=(5, 3, 30, 2, 40), lens=(40, 60, 50, 96))
# B = 37, six searches steps, runs of equal starts: q_b > 0 at b = 3, 4, 17, 18, 35, 36 only; tokens 0, 1 and 25..27 un-owned
MANY_Q = {3: 2, 4: 1, 17: 9, 18: 1, 35: 7, 36: 3}


def _many():
    cu = [2]
    for b in range(37):
        cu.append(cu[-1] + MANY_Q.get(b, 0))
    return dict(cu=tuple(cu), lens=tuple(10 + 2 * b for b in range(37)))


MANY = _many()


def source(d, seed, T=T, scale=6.0):
    """ONE fused [T, H_q + 2 H_kv, d] projection output; views() slices it."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(T, HQ + 2 * HKV, d, generator=g) - 0.5) * scale).bfloat16()


def views(x):
    """Q [T, H_q, d], K_new and V_new [T, H_kv, d]: the three slices of the fused tensor, as they are."""
    return x[:, :HQ], x[:, HQ:HQ + HKV], x[:, HQ + HKV:]


def table_for(cu, lens, seed, T=T, bad=()):
    """A block table for one call: every logical page a written row needs gets a pool page of its own from a seeded permutation
    (so pages written by the call belong to one sequence each), every other entry is UNUSED; then bad: (b, p, value)."""
    import kv_append_ref as ar
    B = len(lens)
    perm = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(seed)).tolist()
    table = torch.tensor([[UNUSED[(b * MAX_PAGES + p) % 2] for p in range(MAX_PAGES)] for b in range(B)], dtype=torch.int32)
    for b, (_, q) in enumerate(xr.sanitised(cu, T)):
        for i in range(q):
            pos = ar.position(lens[b], q, i, MAX_PAGES * PAGE)
            if pos is not None and int(table[b, pos // PAGE]) in UNUSED:
                table[b, pos // PAGE] = perm.pop()
    for b, p, value in bad:
        table[b, p] = value
    return table
