"""The rotary-embedding KV-cache append (fa2_rope_kv_append, fa2_rope_kv_append_paged; include/fa2_rope_mi355x.h) as a torch model
of the whole contract (a helper module, no tests: tests/test_rope_reference.py certifies what is here,
tests/test_gpu_rope_append.py runs the kernels against it).

THE MODEL is written from the contract's words, in Python integers and separate torch ops, not from the product's code:
    pos = len - n_new + t                      (Python ints: no width, no overflow); the cache row AND the table row
    pairs: (i, i + rot_dim/2) rotate-half, (2i, 2i + 1) interleaved; both use table column i; elements past rot_dim pass through
    a = x1*c;  b = x2*s;  y1 = (a - b).bfloat16();  e = x2*c;  f = x1*s;  y2 = (e + f).bfloat16()      (fp32, one op each)
    K: the rotated bf16 rows through kv_append_ref.append / append_paged; V: unrotated through the same
    Q_out[b, h, t]: the rotated row if 0 <= pos < capacity, else +0.0 throughout; EVERY row is written"""
import torch

import kv_append_ref as ar


def rotate(x, c, s, interleaved):
    """x [..., d] in fp32 or fp64, c and s [..., rot_dim / 2] broadcastable against it: the rotated rows in x's dtype, one torch
    op per product and per sum (torch fuses nothing on the host)."""
    half = c.shape[-1]
    rot = 2 * half
    assert rot <= x.shape[-1]
    if interleaved:
        x1, x2 = x[..., 0:rot:2], x[..., 1:rot:2]
    else:
        x1, x2 = x[..., :half], x[..., half:rot]
    a = x1 * c
    b = x2 * s
    y1 = a - b
    e = x2 * c
    f = x1 * s
    y2 = e + f
    y = x.clone()
    if interleaved:
        y[..., 0:rot:2], y[..., 1:rot:2] = y1, y2
    else:
        y[..., :half], y[..., half:rot] = y1, y2
    return y


def rotate_bf16(x, c, s, interleaved):
    """bf16 rows -> bf16 rows: widened to fp32 (exact), rotated in fp32, rounded to nearest even; the tail keeps its BITS."""
    rot = 2 * c.shape[-1]
    y = rotate(x.float(), c.float(), s.float(), interleaved).bfloat16()
    y.view(torch.int16)[..., rot:] = x.contiguous().view(torch.int16)[..., rot:]
    return y


def rope(X, cos, sin, lens, capacity, interleaved):
    """X [B, H, n_new, d] bf16 (any strides) -> contiguous bf16 [B, H, n_new, d]: row (b, :, t) rotated at table row
    pos = lens[b] - n_new + t where 0 <= pos < capacity, +0.0 throughout elsewhere (the Q_out rule; the append drops such a
    token's K anyway)."""
    B, H, n_new, d = X.shape
    out = torch.zeros(B, H, n_new, d, dtype=torch.bfloat16)
    for b in range(B):
        for t in range(n_new):
            pos = ar.position(lens[b], n_new, t, capacity)
            if pos is not None:
                out[b, :, t] = rotate_bf16(X[b, :, t], cos[pos], sin[pos], interleaved)
    return out


def rope_append(Q, K_new, V_new, K_cache, V_cache, cos, sin, lens, interleaved=False, k_descale=None, v_descale=None):
    """The fused call on host tensors, IN PLACE on the caches; returns (Q_out or None, the append's list of written tokens)."""
    cap = K_cache.shape[2]
    assert cos.shape[0] >= cap
    written = ar.append(rope(K_new, cos, sin, lens, cap, interleaved), V_new, K_cache, V_cache, lens, k_descale, v_descale)
    return (None if Q is None else rope(Q, cos, sin, lens, cap, interleaved)), written


def rope_append_paged(Q, K_new, V_new, K_pages, V_pages, table, cos, sin, lens, interleaved=False, k_descale=None, v_descale=None):
    """The paged form.  A bad table entry drops K and V only (append_paged's rule): Q_out depends on the position alone."""
    cap = table.shape[1] * K_pages.shape[2]
    assert cos.shape[0] >= cap
    written = ar.append_paged(rope(K_new, cos, sin, lens, cap, interleaved), V_new, K_pages, V_pages, table, lens, k_descale, v_descale)
    return (None if Q is None else rope(Q, cos, sin, lens, cap, interleaved)), written


def random_tables(n_positions, rot_dim, seed):
    """cos and sin as the GPU tests want them: seeded random fp32 in (-1, 1), a DISTINCT value per (table, position, column) --
    not a real rotation, so a wrong row, a wrong column, swapped tables, a wrong sign or a wrong partner each changes bits."""
    g = torch.Generator().manual_seed(seed)
    n = 2 * n_positions * (rot_dim // 2)
    # value k of n lies in the k-th of n disjoint intervals of (-1, 1), at a random place in its middle half: distinct by construction
    v = ((torch.randperm(n, generator=g).double() + 0.25 + 0.5 * torch.rand(n, generator=g).double()) / n * 2 - 1).float()
    assert v.unique().numel() == n and (v.abs() < 1).all()
    return v[:n // 2].view(n_positions, rot_dim // 2).contiguous(), v[n // 2:].view(n_positions, rot_dim // 2).contiguous()


def real_tables(n_positions, rot_dim, base=10000.0, dtype=torch.float64):
    """cos and sin of a real rotation: angle pos * base^(-2i / rot_dim)."""
    inv = base ** (-torch.arange(0, rot_dim, 2, dtype=torch.float64) / rot_dim)
    ang = torch.arange(n_positions, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dtype), ang.sin().to(dtype)


def witnesses(seed=2024, draws=1 << 22):
    """Elements that tell the contract's y1 from a CONTRACTED one.  Over seeded draws of (x1, x2, c, s) -- x bf16 in (-3, 3),
    c and s fp32 in (-1, 1) -- returns {form: (x1, x2, c, s)} of the draws whose bf16 result differs between
        the contract     bf16(fl(fl(x1*c) - fl(x2*s)))
    and  "fma_first"     bf16(fl(x1*c - fl(x2*s)))           fma(x1, c, -fl(x2*s))
    or   "fma_second"    bf16(fl(fl(x1*c) - x2*s))           fma(-x2, s, fl(x1*c))
    The contracted forms are evaluated in float64 (a bf16 x fp32 product is exact there) and rounded once to fp32."""
    g = torch.Generator().manual_seed(seed)
    x1 = ((torch.rand(draws, generator=g) - 0.5) * 6).bfloat16().float()
    x2 = ((torch.rand(draws, generator=g) - 0.5) * 6).bfloat16().float()
    c = torch.rand(draws, generator=g) * 2 - 1
    s = torch.rand(draws, generator=g) * 2 - 1
    a = x1 * c
    b = x2 * s
    want = (a - b).bfloat16()
    first = (x1.double() * c.double() - b.double()).float().bfloat16()
    second = (a.double() - x2.double() * s.double()).float().bfloat16()
    out = {}
    for name, other in (("fma_first", first), ("fma_second", second)):
        hit = (want.view(torch.int16) != other.view(torch.int16)).nonzero().flatten()
        out[name] = tuple(t[hit].clone() for t in (x1.bfloat16(), x2.bfloat16(), c, s))
    return out
