"""The KV-cache append (fa2_kv_append, fa2_kv_append_paged; include/fa2_kvcache_mi355x.h) as a torch model of the whole contract
(a helper module, no tests: tests/test_kv_append_reference.py certifies what is here, tests/test_kv_append_addr.py enumerates
the product's address header against it, tests/test_gpu_kv_append.py runs the kernels against it).

THE MODEL is written from the contract's words, in Python integers and torch's own casts, not from the product header:
    pos = len - n_new + t                 (Python ints: no width, no overflow)
    written  iff  0 <= pos < capacity     (and, paged, 0 <= block_table[b][pos // page_size] < n_pages); else dropped
    bf16 cache: the source bits;  e4m3 cache: (x.float() / descale[h]).clamp(-448, 448).to(torch.float8_e4m3fn)
Everything works on BYTES of host tensors (uint8 / int16 views), so a NaN compares like any other value."""
import torch

E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
NAN_CODES = (0x7F, 0xFF)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def position(length, n_new, t, capacity):
    """The logical row token t goes to, or None: dropped."""
    pos = int(length) - int(n_new) + int(t)
    return pos if 0 <= pos < capacity else None


def row_contiguous(length, n_new, t, capacity, b, h, H_kv):
    """The row index into a cache viewed as [B * H_kv * capacity, d], or None."""
    pos = position(length, n_new, t, capacity)
    return None if pos is None else (b * H_kv + h) * capacity + pos


def table_index(pos, page_size):
    return pos // page_size


def row_paged(length, n_new, t, page_size, max_pages, entry, n_pages, h, H_kv):
    """The row index into a pool viewed as [n_pages * H_kv * page_size, d], or None.  entry: what the table holds at
    [b][pos // page_size] (only looked at when the position itself is in range)."""
    pos = position(length, n_new, t, max_pages * page_size)
    if pos is None or not 0 <= int(entry) < n_pages:
        return None
    return (int(entry) * H_kv + h) * page_size + pos % page_size


def quantise(x, descale=None):
    """e4m3 of a host tensor x [*, H_kv, *, d] (any float dtype; widened to fp32 exactly), head h divided by descale[h] (fp32
    [H_kv] or None = 1): the documented expression, word for word."""
    xf = x.float()
    if descale is not None:
        xf = xf / descale.float()[None, :, None, None]
    return xf.clamp(-E4M3_MAX, E4M3_MAX).to(E4M3)


def _stored(x, fp8, descale):
    """[B, H_kv, n_new, d] -> what the cache holds for it, as a byte-comparable integer tensor (int16 bits or uint8 codes)."""
    return quantise(x, descale).view(torch.uint8) if fp8 else x.contiguous().view(torch.int16)


def _bits(cache):
    return cache.view(torch.uint8) if cache.dtype == E4M3 else cache.view(torch.int16)


def append(K_new, V_new, K_cache, V_cache, lens, k_descale=None, v_descale=None):
    """The append on host tensors, IN PLACE on K_cache, V_cache [B, H_kv, N_cap, d] (bf16 or e4m3).  lens: B Python ints, the
    lengths after the append.  Returns the list of (b, t, pos) written."""
    B, H, n_new, d = K_new.shape
    cap = K_cache.shape[2]
    fp8 = K_cache.dtype == E4M3
    written = []
    for new, cache, ds in ((K_new, K_cache, k_descale), (V_new, V_cache, v_descale)):
        src, dst = _stored(new, fp8, ds), _bits(cache)
        for b in range(B):
            for t in range(n_new):
                pos = position(lens[b], n_new, t, cap)
                if pos is not None:
                    dst[b, :, pos] = src[b, :, t]
                    if cache is K_cache:
                        written.append((b, t, pos))
    return written


def append_paged(K_new, V_new, K_pages, V_pages, table, lens, k_descale=None, v_descale=None):
    """The paged append on host tensors, IN PLACE on the pools [n_pages, H_kv, page_size, d].  table: int32 [B, max_pages] host
    tensor.  Returns the list of (b, t, page, row) written."""
    B, H, n_new, d = K_new.shape
    n_pages, _, P, _ = K_pages.shape
    max_pages = table.shape[1]
    fp8 = K_pages.dtype == E4M3
    written = []
    for new, pool, ds in ((K_new, K_pages, k_descale), (V_new, V_pages, v_descale)):
        src, dst = _stored(new, fp8, ds), _bits(pool)
        for b in range(B):
            for t in range(n_new):
                pos = position(lens[b], n_new, t, max_pages * P)
                if pos is None:
                    continue
                entry = int(table[b, table_index(pos, P)])
                if 0 <= entry < n_pages:
                    dst[entry, :, pos % P] = src[b, :, t]
                    if pool is K_pages:
                        written.append((b, t, entry, pos % P))
    return written


# fp32 inputs at descale 1 and their e4m3 bytes (None: a NaN code), checked with torch
BYTE_TABLE = ((1e9, 126), (-1e9, 254), (float("inf"), 126), (float("-inf"), 254), (float("nan"), None), (448.0, 126), (464.0, 126),
              (479.9, 126), (2.0 ** -10, 0), (1e-10, 0), (-0.0, 128))


def special_values():
    """bf16 values (a 1-d host tensor) that exercise the quantiser at descale 1 and at the tests' descales: overflow both ways,
    +-inf, NaN, the largest finite e4m3 and just beyond, exact ties of the normal and the subnormal range, values below half the
    smallest subnormal, both zeros."""
    v = [1e9, -1e9, float("inf"), float("-inf"), float("nan"), 448.0, -448.0, 464.0, 480.0, 432.0, 416.0, 2.0 ** -10, -2.0 ** -10,
         3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 1e-10, -1e-10, 0.0, -0.0, 1.0625, 1.1875, 17.0, 19.0, 0.0146484375,
         2.0 ** -6, 2.0 ** -7, 1.5 * 2.0 ** -9, 3e38, -3e38, 1e-38]
    return torch.tensor(v, dtype=torch.float32).bfloat16()
