"""CPU: the two-sided plan of a packed batch with its own query and key lengths (fa2_varlen_plan_build_qk, VarlenPlan(cu_seqlens,
cu_seqlens_k)), the argument checking of every _qk entry point and of their Python wrappers, and the float64 NumPy reference of
tests/regimes.py (what tests/test_gpu_qk.py and tests/test_gpu_regimes.py judge the kernels by) pinned to the oracle on square
shapes.  No GPU: the plan is host code, and the launch calls are only driven
into the returns that come before any device call (never-dereferenced pointers, the `one = c_void_p(16)` idiom of
test_capi_symbols.py)."""
import ctypes

import numpy as np
import pytest
import torch

from regimes import ref_attention

PAIRS = ((300, 1), (1, 300), (0, 77), (257, 64), (77, 0), (0, 0), (600, 1100), (256, 512), (512, 256), (255, 255), (64, 257))
HEADER_BYTES, ITEM_INTS = 32, 5


def _lib():
    from cuda_flashattention_amd import _capi
    return _capi.lib()


def _cu(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def _build(cq, ck, nbytes=None):
    """(status, blob) of fa2_varlen_plan_build_qk on a buffer of fa2_varlen_plan_bytes_qk (or nbytes) bytes."""
    lib = _lib()
    cq = np.ascontiguousarray(cq, dtype=np.int32)
    ck = None if ck is None else np.ascontiguousarray(ck, dtype=np.int32)
    n = lib.fa2_varlen_plan_bytes_qk(len(cq) - 1, int(cq[-1]), int(cq[-1] if ck is None else ck[-1])) if nbytes is None else nbytes
    blob = np.zeros(max(n, 1), dtype=np.uint8)
    return lib.fa2_varlen_plan_build_qk(cq.ctypes.data, None if ck is None else ck.ctypes.data, len(cq) - 1, blob.ctypes.data, n), blob


def _lists(blob):
    head = blob[:HEADER_BYTES].view(np.int32)
    n_row, n_key = int(head[4]), int(head[5])
    items = blob[HEADER_BYTES:HEADER_BYTES + 4 * ITEM_INTS * (n_row + n_key)].view(np.int32).reshape(-1, ITEM_INTS)
    return head, items[:n_row], items[n_row:]


def test_every_block_once_on_each_side_in_the_documented_order():
    lq, lk = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    cq, ck = _cu(lq), _cu(lk)
    st, blob = _build(cq, ck)
    assert st == 0
    head, rows, keys = _lists(blob)
    blocks = lambda n: (n + 255) // 256
    assert head[2] == len(PAIRS) and head[3] == sum(lq) and head[7] == sum(lk) and head[6] == max(lq)
    assert head[4] == sum(blocks(n) for n in lq) and head[5] == sum(blocks(n) for n in lk) and head[4] != head[5]
    # sequences by descending len_q x len_k, ties by index (every sequence with an empty side ties at 0)
    order = sorted(range(len(PAIRS)), key=lambda i: (-lq[i] * lk[i], i))
    item = lambda i, b: [int(cq[i]), int(ck[i]), lq[i], lk[i], b]
    assert rows.tolist() == [item(i, b) for i in order for b in reversed(range(blocks(lq[i])))]      # len_k == 0 included
    assert keys.tolist() == [item(i, b) for i in order for b in range(blocks(lk[i]))]                # len_q == 0 included
    seqs = lambda items: {(r[0], r[1], r[2], r[3]) for r in items.tolist()}
    assert (int(cq[2]), int(ck[2]), 0, 77) in seqs(keys) and all(r[2] > 0 for r in rows.tolist())    # (0, 77): key list only
    assert (int(cq[4]), int(ck[4]), 77, 0) not in seqs(keys) and all(r[3] > 0 for r in keys.tolist())
    assert (int(cq[4]), int(ck[4]), 77, 0) in seqs(rows)                                             # (77, 0): row list only
    assert not any(r[2] == 0 and r[3] == 0 for r in rows.tolist() + keys.tolist())                   # (0, 0): nowhere
    for items in (rows, keys):
        got = [tuple(r) for r in items.tolist()]
        assert len(got) == len(set(got))                                                             # each (sequence, block) once
    st2, blob2 = _build(cq, ck)
    assert st2 == 0 and blob.tobytes() == blob2.tobytes()                                            # deterministic to the byte
    # 64-bit products: 3000000 x 3000000 does not fit 32 bits and must still sort ahead of 100 x 100
    st3, blob3 = _build(_cu((100, 3000000)), _cu((100, 3000000 - 1)))
    assert st3 == 0 and _lists(blob3)[1][0].tolist()[:4] == [100, 100, 3000000, 3000000 - 1]


def test_no_key_list_or_an_equal_one_is_the_one_sided_plan_byte_for_byte():
    lib = _lib()
    for lengths in ((1, 63, 0, 64, 65, 255, 256, 257, 600, 0), (300, 300, 300), (5,)):
        cu = _cu(lengths)
        n = lib.fa2_varlen_plan_bytes(len(lengths), int(cu[-1]))
        assert lib.fa2_varlen_plan_bytes_qk(len(lengths), int(cu[-1]), int(cu[-1])) == n
        old = np.zeros(n, dtype=np.uint8)
        assert lib.fa2_varlen_plan_build(cu.ctypes.data, len(lengths), old.ctypes.data, n) == 0
        for ck in (None, cu.copy()):
            st, blob = _build(cu, ck)
            assert st == 0 and blob.tobytes() == old.tobytes() and _lists(blob)[0][7] == 0


@pytest.mark.parametrize("cq,ck", [([0, 5, 3], [0, 5, 9]), ([0, 5, 9], [0, 5, 3]), ([0, 0, 0], [0, 4, 8]), ([0, 4, 8], [0, 0, 0]),
                                   ([1, 4], [0, 4]), ([0, 4], [1, 5]), ([0, 4], [0, -1]), ([0, 4], [0, (0x7fffffff // 512) + 1]),
                                   ([0, (0x7fffffff // 512) + 1], [0, 4])])
def test_invalid_lists_are_refused(cq, ck):
    """Per list: [0] != 0, a decreasing entry, a total < 1 or past the row limit -> -2, from the C ABI and from VarlenPlan."""
    st, _ = _build(cq, ck, nbytes=1 << 16)
    assert st == -2
    import cuda_flashattention_amd as fa
    with pytest.raises(ValueError):
        fa.VarlenPlan(cq, ck)


def test_plan_build_null_pointers_sizes_and_n_seqs():
    lib = _lib()
    cq, ck = _cu((5, 300)), _cu((600, 0))
    blob = np.zeros(1 << 12, dtype=np.uint8)
    assert lib.fa2_varlen_plan_build_qk(None, ck.ctypes.data, 2, blob.ctypes.data, blob.size) == -1
    assert lib.fa2_varlen_plan_build_qk(cq.ctypes.data, ck.ctypes.data, 2, None, blob.size) == -1
    assert lib.fa2_varlen_plan_build_qk(cq.ctypes.data, ck.ctypes.data, 0, blob.ctypes.data, blob.size) == -2
    assert lib.fa2_varlen_plan_build_qk(cq.ctypes.data, ck.ctypes.data, -3, blob.ctypes.data, blob.size) == -2
    assert lib.fa2_varlen_plan_bytes_qk(0, 10, 10) == 0 and lib.fa2_varlen_plan_bytes_qk(2, 0, 10) == 0
    assert lib.fa2_varlen_plan_bytes_qk(2, 10, 0) == 0
    need = HEADER_BYTES + (3 + 3) * 4 * ITEM_INTS           # row blocks 1 + 2, key blocks 3 + 0
    assert lib.fa2_varlen_plan_bytes_qk(2, 305, 600) >= need
    assert lib.fa2_varlen_plan_build_qk(cq.ctypes.data, ck.ctypes.data, 2, blob.ctypes.data, need) == 0
    for short in (0, 8, HEADER_BYTES, need - 1):            # too small: -5, and nothing written past the buffer
        guard = np.full(need + 64, 0xA5, dtype=np.uint8)
        assert lib.fa2_varlen_plan_build_qk(cq.ctypes.data, ck.ctypes.data, 2, guard.ctypes.data, short) == -5
        assert (guard[short:] == 0xA5).all()
    # the upper bound holds for the worst case of its arguments on either side
    for lq, lk in (((257,) * 7, (1,) * 7), ((1,) * 40, (0,) * 39 + (9,)), ((256,) * 3, (257, 0, 511)), ((1, 0, 0, 0), (0, 0, 0, 1))):
        st, _ = _build(_cu(lq), _cu(lk))
        assert st == 0, (lq, lk)


def test_python_plan_mirrors_the_blob():
    import cuda_flashattention_amd as fa
    lq, lk = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    cq, ck = _cu(lq), _cu(lk)
    _, blob = _build(cq, ck)
    _, rows, keys = _lists(blob)
    for aq, ak in ((cq.tolist(), ck.tolist()), (cq, ck.astype(np.int64)), (torch.from_numpy(cq.copy()), torch.from_numpy(ck.astype(np.int64)))):
        plan = fa.VarlenPlan(aq, ak)
        assert plan.two_sided and (plan.n_seqs, plan.total, plan.total_k) == (len(PAIRS), sum(lq), sum(lk))
        assert (plan.max_len, plan.max_len_k) == (max(lq), max(lk))
        assert (plan.cu_seqlens == cq).all() and (plan.cu_seqlens_k == ck).all()
        assert plan.row_items.shape == rows.shape and (plan.row_items == rows).all()
        assert plan.key_items.shape == keys.shape and (plan.key_items == keys).all()
        assert plan.nbytes == HEADER_BYTES + 4 * ITEM_INTS * (len(rows) + len(keys))
    one = fa.VarlenPlan(cq)
    assert not one.two_sided and one.total_k == one.total and one.max_len_k == one.max_len and (one.cu_seqlens_k == cq).all()
    same = fa.VarlenPlan(cq, cq.tolist())
    assert not same.two_sided and bytes(same._blob) == bytes(one._blob)
    for bad in ([0], 7, [[0, 3]], [0.0, 3.0], torch.tensor([0.0, 4.0]), ck[:-1]):
        with pytest.raises(ValueError, match="cu_seqlens_k"):
            fa.VarlenPlan(cq, bad)


def test_launch_validation_comes_before_any_device_call():
    lib = _lib()
    cq, ck = _cu((320, 0, 77, 512)), _cu((1000, 40, 0, 512))
    st, blob = _build(cq, ck)
    assert st == 0
    head, rows, keys = _lists(blob)
    n = HEADER_BYTES + 4 * ITEM_INTS * (len(rows) + len(keys))
    assert n <= blob.size and len(rows) == 2 + 1 + 2 and len(keys) == 4 + 1 + 2
    Tq, Tk, one, host = 909, 1552, ctypes.c_void_p(16), blob.ctypes.data
    fwd = lambda hq=4, hkv=2, tq=Tq, tk=Tk, d=128, scale=0.125, dtype=0, plan_host=host, plan_dev=one, nbytes=n, q=one: \
        lib.fa2_forward_varlen_qk(q, one, one, one, one, hq, hkv, tq, tk, d, scale, dtype, 1, plan_host, plan_dev, nbytes, None)
    assert fwd(q=None) == -1 and fwd(plan_host=None) == -1 and fwd(plan_dev=None) == -1
    assert fwd(d=96) == -3
    assert fwd(dtype=1) == -4 and fwd(dtype=2) == -4
    assert fwd(tq=Tq + 1) == -2 and fwd(tk=Tk - 1) == -2 and fwd(tq=0) == -2 and fwd(tk=0) == -2 and fwd(tq=Tk, tk=Tq) == -2
    assert fwd(hkv=3) == -2 and fwd(hkv=0) == -2 and fwd(scale=0.0) == -2
    assert fwd(nbytes=n - 1) == -2 and fwd(nbytes=8) == -2
    assert fwd(q=None, tk=0) == -1 and fwd(d=96, dtype=1) == -3 and fwd(d=96, tk=Tk + 1) == -2      # NULL, shape, head_dim, dtype
    bad = blob.copy()
    bad[0] ^= 0xFF                                                            # not a plan
    assert fwd(plan_host=bad.ctypes.data) == -2
    bwd = lambda hq=4, hkv=2, tq=Tq, tk=Tk, d=128, dtype=0, ws=one, ws_bytes=1 << 30, plan_host=host: lib.fa2_backward_varlen_qk(
        *([one] * 9), hq, hkv, tq, tk, d, 0.125, dtype, 1, plan_host, one, n, ws, ws_bytes, None)
    assert lib.fa2_backward_varlen_qk(*([None] * 9), 4, 2, Tq, Tk, 128, 0.125, 0, 1, host, one, n, one, 1 << 30, None) == -1
    assert bwd(d=96) == -3 and bwd(dtype=1) == -4 and bwd(tq=Tq + 1) == -2 and bwd(tk=Tk + 1) == -2 and bwd(hkv=3) == -2
    need = lib.fa2_backward_varlen_qk_workspace_bytes(4, 2, Tq, Tk, 128, 0)
    assert need == 3 * ((4 * Tq * 4 + 255) // 256 * 256)                      # D and the two row-constant planes over [H_q][T_q]
    assert bwd(ws=None) == -5 and bwd(ws_bytes=need - 1) == -5
    assert bwd(d=96, ws=None) == -3 and bwd(dtype=1, ws=None) == -4 and bwd(tk=Tk + 1, d=96) == -2      # the workspace comes last
    assert lib.fa2_backward_varlen_qk_workspace_bytes(4, 3, Tq, Tk, 128, 0) == 0
    assert lib.fa2_backward_varlen_qk_workspace_bytes(4, 2, Tq, 0, 128, 0) == 0
    # the one-list calls refuse the two-sided blob (they would read K as T_q rows), whichever total they are given
    for t in (Tq, Tk):
        assert lib.fa2_forward_varlen(one, one, one, one, one, 4, 2, t, 128, 0.125, 0, 1, host, one, n, None) == -2
        assert lib.fa2_backward_varlen(*([one] * 9), 4, 2, t, 128, 0.125, 0, 1, host, one, n, one, 1 << 30, None) == -2
    # ... and the _qk calls take a one-list blob, with total_k == total_q only (driven into the next check: head_dim)
    st1, blob1 = _build(cq, None)
    assert st1 == 0
    n1 = HEADER_BYTES + 4 * ITEM_INTS * 2 * 5
    assert fwd(tk=Tq, plan_host=blob1.ctypes.data, nbytes=n1, d=96) == -3 and fwd(plan_host=blob1.ctypes.data, nbytes=n1, d=96) == -2
    assert bwd(tk=Tq, plan_host=blob1.ctypes.data, d=96) == -3 and bwd(plan_host=blob1.ctypes.data, d=96) == -2


def test_dense_entry_points_check_their_arguments():
    lib = _lib()
    one = ctypes.c_void_p(16)
    fwd = lambda hq=4, hkv=2, nq=512, nk=4096, d=128, scale=0.125, dtype=0, q=one, B=2: lib.fa2_forward_qk(
        q, one, one, one, one, B, hq, hkv, nq, nk, d, scale, dtype, 1, None)
    assert fwd(q=None) == -1
    assert fwd(nq=0) == -2 and fwd(nk=0) == -2 and fwd(nk=-4) == -2 and fwd(B=0) == -2 and fwd(scale=-1.0) == -2
    assert fwd(hkv=3) == -2 and fwd(hkv=0) == -2 and fwd(nk=1 << 23) == -2          # a K slab past 2 GiB at 4 bytes per element
    assert fwd(d=96) == -3 and fwd(dtype=1) == -4 and fwd(dtype=2) == -4
    assert fwd(q=None, nk=0) == -1 and fwd(nk=0, d=96) == -2 and fwd(d=96, dtype=1) == -3      # NULL, shape, head_dim, dtype
    bwd = lambda hq=4, hkv=2, nq=512, nk=4096, d=128, dtype=0, ws=one, ws_bytes=1 << 40, phases=7, B=2: lib.fa2_backward_qk(
        *([one] * 9), B, hq, hkv, nq, nk, d, 0.125, dtype, 1, ws, ws_bytes, None, phases)
    assert lib.fa2_backward_qk(*([None] * 9), 2, 4, 2, 512, 4096, 128, 0.125, 0, 1, one, 1 << 40, None, 7) == -1
    assert bwd(nq=0) == -2 and bwd(nk=0) == -2 and bwd(hkv=3) == -2 and bwd(hkv=0) == -2 and bwd(B=0) == -2
    assert bwd(d=96) == -3 and bwd(dtype=1) == -4 and bwd(dtype=2) == -4 and bwd(d=96, dtype=1) == -3 and bwd(nk=0, d=96) == -2
    need = lib.fa2_backward_qk_workspace_bytes(2, 4, 2, 512, 4096, 128, 0)
    assert need == 3 * ((2 * 4 * 512 * 4 + 255) // 256 * 256)                       # D and the two row-constant planes over [B][H_q][q_len]
    assert need == lib.fa2_backward_qk_workspace_bytes(2, 4, 2, 512, 77, 128, 0)    # the key side does not enter
    assert bwd(ws=None) == -5 and bwd(ws_bytes=need - 1) == -5 and bwd(ws=None, d=96) == -3 and bwd(ws=None, dtype=1) == -4
    assert bwd(phases=8) == -6 and bwd(phases=9) == -6 and bwd(phases=8, ws=None) == -5      # the single kernel takes no rectangle
    # equal lengths: the grouped-query call's workspace, whatever it holds at that shape
    for B, hq, hkv, n, d in ((4, 16, 16, 8192, 128), (4, 16, 4, 8192, 128), (2, 8, 2, 300, 128), (2, 6, 3, 4096, 64), (1, 4, 1, 1, 64)):
        assert lib.fa2_backward_qk_workspace_bytes(B, hq, hkv, n, n, d, 0) == lib.fa2_backward_gqa_workspace_bytes(B, hq, hkv, n, d, 0) > 0
    assert bwd(nq=8192, nk=8192, ws_bytes=lib.fa2_backward_gqa_workspace_bytes(2, 4, 2, 8192, 128, 0) - 1) == -5
    for args in ((0, 4, 2, 512, 64, 128, 0), (2, 4, 3, 512, 64, 128, 0), (2, 4, 2, 0, 64, 128, 0), (2, 4, 2, 512, 0, 128, 0), (2, 4, 0, 512, 512, 128, 0)):
        assert lib.fa2_backward_qk_workspace_bytes(*args) == 0, args


def test_python_wrappers_refuse_what_the_abi_would_take_on_trust():
    import cuda_flashattention_amd as fa
    plan = fa.VarlenPlan([0, 320, 320, 397, 909], [0, 1000, 1040, 1040, 1552])
    mk = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    Q, K, V = mk(4, 909, 128), mk(2, 1552, 128), mk(2, 1552, 128)
    L = torch.zeros(4, 909)
    with pytest.raises(ValueError, match="device tensor"):
        fa.flash_attention_2_varlen_forward(Q, K, V, plan)
    with pytest.raises(ValueError, match="device tensor"):
        fa.flash_attention_2_varlen_backward(Q, K, V, Q, L, Q, plan)
    with pytest.raises(ValueError, match="T = 909"):
        fa.flash_attention_2_varlen_forward(K, K, V, plan)
    with pytest.raises(ValueError, match="T_k = 1552"):
        fa.flash_attention_2_varlen_forward(Q, mk(2, 909, 128), mk(2, 909, 128), plan)
    with pytest.raises(ValueError, match="T_k = 1552"):
        fa.attention_varlen(Q, K, mk(2, 909, 128), plan)
    with pytest.raises(ValueError, match="T_k = 1552"):
        fa.flash_attention_2_varlen_backward(Q, K[:, :909], V[:, :909], Q, L, Q, plan)
    with pytest.raises(ValueError, match="do not divide"):
        fa.flash_attention_2_varlen_forward(Q, mk(3, 1552, 128), mk(3, 1552, 128), plan)
    # the dense calls: 4-D bf16 tensors, B and d of K equal to Q's, H_kv dividing H, V like K; then the device
    q, k, v = mk(2, 4, 64, 128), mk(2, 2, 257, 128), mk(2, 2, 257, 128)
    l = torch.zeros(2, 4, 64)
    for f in (lambda K_, V_: fa.flash_attention_2_qk_forward(q, K_, V_), lambda K_, V_: fa.attention_qk(q, K_, V_),
              lambda K_, V_: fa.flash_attention_2_qk_backward(q, K_, V_, q, l, q)):
        with pytest.raises(ValueError, match="device tensor"):
            f(k, v)
        with pytest.raises(ValueError, match="H_kv dividing H = 4"):
            f(mk(2, 3, 257, 128), mk(2, 3, 257, 128))
        with pytest.raises(ValueError, match="does not match"):
            f(mk(1, 2, 257, 128), mk(1, 2, 257, 128))
        with pytest.raises(ValueError, match="does not match"):
            f(mk(2, 2, 257, 64), mk(2, 2, 257, 64))
        with pytest.raises(ValueError, match="V: shape"):
            f(k, mk(2, 2, 256, 128))
        with pytest.raises(ValueError, match=r"\[B, H, N, d\]"):
            f(k[0], v[0])
    with pytest.raises(ValueError, match="bfloat16"):
        fa.flash_attention_2_qk_forward(q.float(), k.float(), v.float())
    # ... and the square-only calls keep refusing a K of another length
    with pytest.raises(ValueError):
        fa.flash_attention_2_forward(q, k, v)


@pytest.mark.parametrize("causal", [False, True])
def test_the_numpy_reference_equals_the_oracle_on_square_shapes(causal):
    """ref_attention of tests/regimes.py against oracle.attention_forward / attention_backward at [1, 3, 300, 64] and a second,
    smaller shape: rel-L2 <= 1e-6 on O, dQ, dK, dV and |dL| <= 1e-5 -- about 40 times the fp32 rounding of the oracle's outputs
    measured at the first shape (2.5e-8 and 2.4e-7), to cover other seeds and shapes."""
    import oracle
    for shape, seed in (((1, 3, 300, 64), 5), ((2, 2, 77, 128), 6)):
        rng = np.random.default_rng(seed)
        q, k, v = (rng.uniform(-0.5, 0.5, shape).astype(np.float32) for _ in range(3))
        g = rng.uniform(-0.2, 0.2, shape).astype(np.float32)
        s = 1.0 / shape[-1] ** 0.5
        O, L = oracle.attention_forward(q, k, v, s, causal=causal)
        want = (O, L) + tuple(oracle.attention_backward(q, k, v, g, s, causal=causal))
        got = ref_attention(q, k, v, g, s, causal)
        for n, a, b in zip(("O", "L", "dQ", "dK", "dV"), got, want):
            err = float(np.abs(a - b).max()) if n == "L" else float(np.linalg.norm(a - b) / np.linalg.norm(a))
            print(shape, causal, n, f"{err:.3e}")
            assert err <= (1e-5 if n == "L" else 1e-6), (shape, n, err)


def test_the_numpy_reference_keeps_the_rules_of_the_rows_without_a_key():
    """Bottom-right alignment and the empty sides, on a problem small enough to check by hand."""
    rng = np.random.default_rng(3)
    q, g = rng.normal(size=(5, 4)), rng.normal(size=(5, 4))
    k, v = rng.normal(size=(2, 4)), rng.normal(size=(2, 4))
    O, L, dQ, dK, dV = ref_attention(q, k, v, g, 0.5, True)              # shift -3: rows 0..2 see nothing, row 3 key 0, row 4 both
    assert np.isneginf(L[:3]).all() and np.isfinite(L[3:]).all() and (O[:3] == 0).all() and (dQ[:3] == 0).all()
    assert np.allclose(O[3], v[0]) and np.allclose(L[3], 0.5 * q[3] @ k[0]) and np.allclose(dV[1], g[4] * np.exp(0.5 * q[4] @ k[1] - L[4]))
    O2, L2, *_ = ref_attention(q[3:], k, v, g[3:], 0.5, True)            # the square problem of the last two rows is the same
    assert np.allclose(O2, O[3:]) and np.allclose(L2, L[3:])
    O, L, dQ, dK, dV = ref_attention(q, k[:0], v[:0], g, 0.5, False)     # no keys
    assert (O == 0).all() and np.isneginf(L).all() and (dQ == 0).all() and dK.shape == (0, 4)
    O, L, dQ, dK, dV = ref_attention(q[:0], k, v, g[:0], 0.5, True)      # no queries
    assert O.shape == (0, 4) and (dK == 0).all() and (dV == 0).all() and dK.shape == (2, 4)
