"""CPU: the plan of a packed variable-length batch (fa2_varlen_plan_build, cuda_flashattention_amd.VarlenPlan) and the argument
checking of the packed entry points -- everything that must hold before a kernel runs.  No GPU: the plan is host code, and the
launch calls are only driven into the returns that come before any device call (never-dereferenced pointers, the
`one = c_void_p(16)` idiom of test_capi_symbols.py)."""
import ctypes

import numpy as np
import pytest
import torch

LENGTHS = (1, 63, 0, 64, 65, 255, 256, 257, 600, 0)
HEADER_BYTES, ITEM_INTS = 32, 5


def _lib():
    from cuda_flashattention_amd import _capi
    return _capi.lib()


def _cu(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def _build(cu, nbytes=None):
    """(status, blob) of fa2_varlen_plan_build on a buffer of fa2_varlen_plan_bytes (or nbytes) bytes."""
    lib = _lib()
    cu = np.ascontiguousarray(cu, dtype=np.int32)
    n = lib.fa2_varlen_plan_bytes(len(cu) - 1, int(cu[-1])) if nbytes is None else nbytes
    blob = np.zeros(max(n, 1), dtype=np.uint8)
    return lib.fa2_varlen_plan_build(cu.ctypes.data, len(cu) - 1, blob.ctypes.data, n), blob


def _lists(blob):
    head = blob[:HEADER_BYTES].view(np.int32)
    n_row, n_key = int(head[4]), int(head[5])
    items = blob[HEADER_BYTES:HEADER_BYTES + 4 * ITEM_INTS * (n_row + n_key)].view(np.int32).reshape(-1, ITEM_INTS)
    return head, items[:n_row], items[n_row:]


@pytest.mark.parametrize("cu", [[0, 5, 3], [0, 0, 0], [1, 4], [0, -1], [0, 4, 4, 2, 9], [0, (0x7fffffff // 512) + 1]])
def test_invalid_cu_seqlens_are_refused(cu):
    """cu_seqlens[0] != 0, a decreasing entry, T < 1, T past the 2 GiB-per-plane rule (at head_dim 128, 4 bytes): -2."""
    lib = _lib()
    arr = np.asarray(cu, dtype=np.int32)
    blob = np.zeros(1 << 16, dtype=np.uint8)
    assert lib.fa2_varlen_plan_build(arr.ctypes.data, len(cu) - 1, blob.ctypes.data, blob.size) == -2
    with pytest.raises(ValueError):
        import cuda_flashattention_amd as fa
        fa.VarlenPlan(cu)


def test_plan_build_null_pointers_sizes_and_n_seqs():
    lib = _lib()
    cu = _cu((5, 300))
    blob = np.zeros(1 << 12, dtype=np.uint8)
    assert lib.fa2_varlen_plan_build(None, 2, blob.ctypes.data, blob.size) == -1
    assert lib.fa2_varlen_plan_build(cu.ctypes.data, 2, None, blob.size) == -1
    assert lib.fa2_varlen_plan_build(cu.ctypes.data, 0, blob.ctypes.data, blob.size) == -2
    assert lib.fa2_varlen_plan_build(cu.ctypes.data, -3, blob.ctypes.data, blob.size) == -2
    assert lib.fa2_varlen_plan_bytes(0, 10) == 0 and lib.fa2_varlen_plan_bytes(2, 0) == 0
    need = HEADER_BYTES + 2 * 3 * 4 * ITEM_INTS          # three blocks in each list
    assert lib.fa2_varlen_plan_bytes(2, 305) >= need
    assert lib.fa2_varlen_plan_build(cu.ctypes.data, 2, blob.ctypes.data, need) == 0
    for short in (0, 8, HEADER_BYTES, need - 1):          # a shape or workspace status, and nothing written past the buffer
        guard = np.full(need + 64, 0xA5, dtype=np.uint8)
        assert lib.fa2_varlen_plan_build(cu.ctypes.data, 2, guard.ctypes.data, short) in (-2, -5)
        assert (guard[short:] == 0xA5).all()
    # the upper bound holds for the worst case of its arguments: every sequence one row past a block boundary
    for lengths in ((257,) * 7, (1,) * 40, (256,) * 3, (1, 0, 0, 0)):
        st, _ = _build(_cu(lengths))
        assert st == 0, lengths


def test_every_block_once_in_the_documented_order():
    cu = _cu(LENGTHS)
    st, blob = _build(cu)
    assert st == 0
    head, rows, keys = _lists(blob)
    assert head[2] == len(LENGTHS) and head[3] == sum(LENGTHS) and head[6] == max(LENGTHS)
    want = {(i, b) for i, n in enumerate(LENGTHS) for b in range((n + 255) // 256)}
    assert head[4] == head[5] == len(want)
    seq_of = {int(cu[i]): i for i, n in enumerate(LENGTHS) if n > 0}          # a non-empty sequence's first row names it
    for items in (rows, keys):
        got = []
        for q0, k0, lq, lk, blk in items.tolist():
            i = seq_of[q0]
            assert k0 == q0 and lq == lk == LENGTHS[i] and lq > 0
            assert 0 <= blk < (lq + 255) // 256
            got.append((i, blk))
        assert len(got) == len(set(got)) and set(got) == want                  # each (sequence, block) exactly once; no empty sequence
    # sequences by descending length, ties by index; a sequence's blocks adjacent, row blocks descending, key blocks ascending
    order = sorted((i for i, n in enumerate(LENGTHS) if n > 0), key=lambda i: (-LENGTHS[i], i))
    assert [(seq_of[r[0]], r[4]) for r in rows.tolist()] == [(i, b) for i in order for b in reversed(range((LENGTHS[i] + 255) // 256))]
    assert [(seq_of[r[0]], r[4]) for r in keys.tolist()] == [(i, b) for i in order for b in range((LENGTHS[i] + 255) // 256)]
    st2, blob2 = _build(cu)
    assert st2 == 0 and blob.tobytes() == blob2.tobytes()                      # deterministic to the byte
    st3, blob3 = _build(_cu((300, 300, 300)))                                  # ties: by index
    assert st3 == 0 and [r[0] for r in _lists(blob3)[1].tolist()] == [0, 0, 300, 300, 600, 600]


def test_python_plan_mirrors_the_blob():
    import cuda_flashattention_amd as fa
    cu = _cu(LENGTHS)
    _, blob = _build(cu)
    _, rows, keys = _lists(blob)
    for arg in (cu.tolist(), cu, cu.astype(np.int64), torch.from_numpy(cu.copy()), torch.from_numpy(cu.astype(np.int64))):
        plan = fa.VarlenPlan(arg)
        assert (plan.n_seqs, plan.total, plan.max_len) == (len(LENGTHS), sum(LENGTHS), max(LENGTHS))
        assert plan.row_items.shape == rows.shape and (plan.row_items == rows).all()
        assert plan.key_items.shape == keys.shape and (plan.key_items == keys).all()
        assert plan.nbytes == HEADER_BYTES + 4 * ITEM_INTS * (len(rows) + len(keys))
    for bad in ([0], 7, [[0, 3]], [0.0, 3.0], torch.tensor([0.0, 4.0])):
        with pytest.raises(ValueError):
            fa.VarlenPlan(bad)


def test_launch_validation_comes_before_any_device_call():
    lib = _lib()
    st, blob = _build(_cu((320, 0, 77, 512)))
    assert st == 0
    head, rows, keys = _lists(blob)
    n = HEADER_BYTES + 4 * ITEM_INTS * (len(rows) + len(keys))          # the blob itself (the buffer is the upper bound)
    assert n <= blob.size and len(rows) == len(keys) == 2 + 1 + 2
    T, one, host = 909, ctypes.c_void_p(16), blob.ctypes.data
    fwd = lambda hq=4, hkv=2, rows=T, d=128, scale=0.125, dtype=0, plan_host=host, plan_dev=one, nbytes=n, q=one: lib.fa2_forward_varlen(
        q, one, one, one, one, hq, hkv, rows, d, scale, dtype, 1, plan_host, plan_dev, nbytes, None)
    assert fwd(q=None) == -1 and fwd(plan_host=None) == -1 and fwd(plan_dev=None) == -1
    assert fwd(d=96) == -3
    assert fwd(dtype=1) == -4 and fwd(dtype=2) == -4
    assert fwd(rows=T + 1) == -2 and fwd(rows=T - 1) == -2 and fwd(rows=0) == -2
    assert fwd(hkv=3) == -2 and fwd(hkv=0) == -2 and fwd(scale=0.0) == -2
    assert fwd(nbytes=n - 1) == -2 and fwd(nbytes=8) == -2
    assert fwd(d=96, dtype=1) == -3 and fwd(d=96, rows=T + 1) == -2          # shape, then head_dim, then dtype
    bad = blob.copy()
    bad[0] ^= 0xFF                                                            # not a plan
    assert fwd(plan_host=bad.ctypes.data) == -2
    bwd = lambda hq=4, hkv=2, rows=T, d=128, dtype=0, ws=one, ws_bytes=1 << 30, plan_host=host: lib.fa2_backward_varlen(
        *([one] * 9), hq, hkv, rows, d, 0.125, dtype, 1, plan_host, one, n, ws, ws_bytes, None)
    assert lib.fa2_backward_varlen(*([None] * 9), 4, 2, T, 128, 0.125, 0, 1, host, one, n, one, 1 << 30, None) == -1
    assert bwd(d=96) == -3 and bwd(dtype=1) == -4 and bwd(rows=T + 1) == -2 and bwd(hkv=3) == -2
    need = lib.fa2_backward_varlen_workspace_bytes(4, 2, T, 128, 0)
    assert need == 3 * ((4 * T * 4 + 255) // 256 * 256)                        # D and the two row-constant planes, nothing else
    assert bwd(ws=None) == -5 and bwd(ws_bytes=need - 1) == -5
    assert bwd(d=96, ws=None) == -3 and bwd(dtype=1, ws=None) == -4           # the workspace comes last
    assert lib.fa2_backward_varlen_workspace_bytes(4, 3, T, 128, 0) == 0


def test_python_wrappers_refuse_what_the_abi_would_take_on_trust():
    import cuda_flashattention_amd as fa
    plan = fa.VarlenPlan([0, 320, 320, 397, 909])
    mk = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    Q, K, V = mk(4, 909, 128), mk(2, 909, 128), mk(2, 909, 128)
    L = torch.zeros(4, 909)
    with pytest.raises(ValueError, match="device tensor"):
        fa.flash_attention_2_varlen_forward(Q, K, V, plan)
    with pytest.raises(ValueError, match="device tensor"):
        fa.flash_attention_2_varlen_backward(Q, K, V, Q, L, Q, plan)
    with pytest.raises(ValueError, match=r"\[H, T, d\]"):
        fa.flash_attention_2_varlen_forward(Q[None], K[None], V[None], plan)
    with pytest.raises(ValueError, match=r"\[H, T, d\]"):
        fa.flash_attention_2_varlen_backward(Q[None], K, V, Q, L, Q, plan)
    with pytest.raises(ValueError, match="T = 909"):
        fa.flash_attention_2_varlen_forward(Q[:, :900], K[:, :900], V[:, :900], plan)
    with pytest.raises(ValueError, match="T = 909"):
        fa.attention_varlen(Q[:, :900], K[:, :900], V[:, :900], plan)
    with pytest.raises(ValueError, match="do not divide"):
        fa.flash_attention_2_varlen_forward(Q, mk(3, 909, 128), mk(3, 909, 128), plan)
    with pytest.raises(ValueError, match="do not divide"):
        fa.flash_attention_2_varlen_backward(Q, mk(3, 909, 128), mk(3, 909, 128), Q, L, Q, plan)
    with pytest.raises(ValueError, match="VarlenPlan"):
        fa.flash_attention_2_varlen_forward(Q, K, V, [0, 909])
    with pytest.raises(ValueError):
        plan.device("cpu")
