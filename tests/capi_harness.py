"""The C ABI against stub launchers: what tests/test_capi_launches.py drives.

fa2_capi.cpp is compiled host-only and linked with tests/capi_stubs.cpp, whose launchers write what they are handed into a text
log instead of enqueuing a kernel.  The grid is calls through _capi.SIGNATURES -- valid ones (valid_calls) over every attention entry point
and every branch of the routing, and invalid ones (invalid_combos: one field, then every pair of fields of a valid baseline set to a
value no entry point accepts) -- and run() turns them into (status, launch records).  No call of the grid reaches the HIP runtime, so
nothing here can touch a GPU.  Tensors are distinct fake addresses; plans, cu_seqlens and the merge pointer arrays are real
host memory, because the library reads those on the host.

    python tests/capi_harness.py build  SRC OUT_DIR      # -> OUT_DIR/libfa2_capi_stub.so from the fa2_capi.cpp at SRC
    python tests/capi_harness.py run    LIB [SECTION]    # the grid's lines on stdout (in a process of its own: the library
                                                         # reads FA2_BACKWARD_PATH once)
    python tests/capi_harness.py record SRC              # tests/golden/capi_launches.txt.gz from the fa2_capi.cpp at SRC
"""
import ctypes
import gzip
import importlib.util
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_launches.txt.gz")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
VALIDATION_CODES = (-1, -2, -3, -4, -5, -6)      # what argument checking may answer (include/fa2_mi355x.h)


def _signatures():
    """_capi.SIGNATURES without importing the package (which imports torch)."""
    spec = importlib.util.spec_from_file_location("_fa2_capi_table", os.path.join(ROOT, "cuda_flashattention_amd", "_capi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SIGNATURES


def build(src, out_dir):
    """-Bsymbolic: the library's calls bind to ITS OWN stubs even where the product library is loaded RTLD_GLOBAL."""
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libfa2_capi_stub.so")
    host = [HIPCC, "-O1", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-host-only", "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "cuda_flashattention_amd", "csrc")]
    objs = []
    for name, path in (("capi", src), ("stubs", os.path.join(ROOT, "tests", "capi_stubs.cpp"))):
        objs.append(os.path.join(out_dir, name + ".o"))
        subprocess.check_call(host + ["-c", os.path.abspath(path), "-o", objs[-1]])
    subprocess.check_call([HIPCC, "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", lib] + objs)
    return lib


# ---- the calls ------------------------------------------------------------------------------------------------------------
# argument names of every entry point the grid calls, in the order of the C declaration (checked against SIGNATURES by count)
_T9 = "Q K V O L dO dQ dK dV"
_WS = "ws ws_bytes stream"
_PLAN = "plan_host plan_dev plan_bytes"
NAMES = {k: v.split() for k, v in {
    "fa2_forward": "Q K V O L B H seq_len head_dim scale dtype causal stream",
    "fa2_forward_gqa": "Q K V O L B H H_kv seq_len head_dim scale dtype causal stream",
    "fa2_forward_qk": "Q K V O L B H H_kv q_len kv_len head_dim scale dtype causal stream",
    "fa2_forward_sink": "Q K V sink O L B H H_kv q_len kv_len head_dim scale dtype causal stream",
    "fa2_forward_varlen": f"Q K V O L H H_kv total_q head_dim scale dtype causal {_PLAN} stream",
    "fa2_forward_varlen_qk": f"Q K V O L H H_kv total_q total_k head_dim scale dtype causal {_PLAN} stream",
    "fa2_forward_varlen_sink": f"Q K V sink O L H H_kv total_q total_k head_dim scale dtype causal {_PLAN} stream",
    "fa2_forward_fp8": f"Q K V O L B H seq_len head_dim scale causal {_WS}",
    "fa2_forward_fp8_scaled": f"Q K V O L B H seq_len head_dim scale q_descale k_descale v_descale causal {_WS}",
    "fa2_forward_step": "Q K V O L Oacc M B H q_len kv_len head_dim scale dtype first last stream",
    "fa2_forward_step_strided": "Q K V O L Oacc M B H q_len kv_len head_dim scale dtype first last q_hs k_hs causal shift stream",
    "fa2_forward_state_finalize": "O L Oacc M rows head_dim dtype stream",
    "fa2_forward_decode": f"Q K V seqlens sink O L B H H_kv q_len kv_capacity head_dim scale dtype causal n_splits {_WS}",
    "fa2_backward": f"{_T9} B H seq_len head_dim scale dtype causal {_WS}",
    "fa2_backward_phases": f"{_T9} B H seq_len head_dim scale dtype causal {_WS} phases",
    "fa2_backward_gqa": f"{_T9} B H H_kv seq_len head_dim scale dtype causal {_WS} phases",
    "fa2_backward_qk": f"{_T9} B H H_kv q_len kv_len head_dim scale dtype causal {_WS} phases",
    "fa2_backward_sink": f"Q K V sink O L dO dQ dK dV dsink B H H_kv q_len kv_len head_dim scale dtype causal {_WS} phases",
    "fa2_backward_lse": f"Q K V sink O L dO dL dQ dK dV dsink B H H_kv q_len kv_len head_dim scale dtype causal {_WS} phases",
    "fa2_backward_block": f"{_T9} B H q_len kv_len head_dim scale dtype q_hs k_hs q_row0 causal shift {_WS} phases",
    "fa2_backward_fused": f"{_T9} B H seq_len head_dim scale mode {_WS}",
    "fa2_backward_varlen": f"{_T9} H H_kv total_q head_dim scale dtype causal {_PLAN} {_WS}",
    "fa2_backward_varlen_qk": f"{_T9} H H_kv total_q total_k head_dim scale dtype causal {_PLAN} {_WS}",
    "fa2_backward_varlen_sink": f"Q K V sink O L dO dQ dK dV dsink H H_kv total_q total_k head_dim scale dtype causal {_PLAN} {_WS}",
    "fa2_backward_varlen_lse": f"Q K V sink O L dO dL dQ dK dV dsink H H_kv total_q total_k head_dim scale dtype causal {_PLAN} {_WS}",
    "fa2_backward_plan": "B H seq_len head_dim dtype causal reason",
    "fa2_backward_gqa_plan": "B H H_kv seq_len head_dim dtype causal reason",
    "fa2_merge_states": "O_parts L_parts n_parts O L rows head_dim dtype stream",
    "fa2_merge_states_backward": "O_parts L_parts O L dO dL dO_parts dL_parts n_parts rows head_dim dtype stream",
    "fa2_backward_workspace_bytes": "B H seq_len head_dim dtype",
    "fa2_backward_fused_workspace_bytes": "B H seq_len head_dim",
    "fa2_backward_gqa_workspace_bytes": "B H H_kv seq_len head_dim dtype",
    "fa2_backward_qk_workspace_bytes": "B H H_kv q_len kv_len head_dim dtype",
    "fa2_backward_sink_workspace_bytes": "B H H_kv q_len kv_len head_dim dtype",
    "fa2_backward_varlen_workspace_bytes": "H H_kv total_q head_dim dtype",
    "fa2_backward_varlen_qk_workspace_bytes": "H H_kv total_q total_k head_dim dtype",
    "fa2_backward_varlen_sink_workspace_bytes": "H H_kv total_q total_k head_dim dtype",
    "fa2_varlen_plan_bytes": "n_seqs total_q",
    "fa2_varlen_plan_bytes_qk": "n_seqs total_q total_k",
}.items()}

# distinct fake base addresses, far enough apart for any tensor of the grid; the workspace is as large as anyone asks
_TENSORS = "Q K V O L dO dQ dK dV sink dsink dL Oacc M seqlens plan_dev ws".split()
ADDR = {n: (i + 1) << 40 for i, n in enumerate(_TENSORS)}
PART_ADDR = {n: [((20 + 10 * j + i) << 40) for i in range(8)] for j, n in enumerate(("O_parts", "L_parts", "dO_parts", "dL_parts"))}
STREAM = 0x5ead0
BIG = 1 << 44
BF16, F32 = 0, 1
B, H = 2, 8

# what no entry point accepts.  Pointers an entry point takes as optional (sink / dsink / dL of the _lse calls, seqlens and sink
# of decode, reason of the plans) are not in this set for that entry point: OPTIONAL
INVALID = {"B": [0], "H": [0], "seq_len": [0], "q_len": [0], "kv_len": [0], "total_q": [0], "total_k": [0], "rows": [0],
           "H_kv": [0, -2], "head_dim": [96], "dtype": [7], "scale": [-1.0], "ws": [None], "plan_bytes": [0], "n_parts": [0, 9],
           "n_splits": [-1, 257], "kv_capacity": [0]}
POINTERS = set(_TENSORS) - {"ws"} | {"plan_host", "O_parts", "L_parts", "dO_parts", "dL_parts"}
OPTIONAL = {"fa2_backward_lse": {"sink", "dsink", "dL"}, "fa2_backward_varlen_lse": {"sink", "dsink", "dL"},
            "fa2_forward_decode": {"seqlens", "sink"}, "fa2_merge_states_backward": {"dL"}}


class Plans:
    """Real host memory the library reads: two packed plans (one-sided and two-sided, an empty sequence on each side) built by
    the library under test, and the part-pointer arrays of a merge."""

    def __init__(self, lib):
        self.cq = np.array([0, 300, 300, 812, 1000], dtype=np.int32)
        self.ck = np.array([0, 0, 513, 600, 1100], dtype=np.int32)      # sequence 0 without keys, sequence 1 without queries
        n = self.cq.size - 1
        self.one = np.zeros(lib.fa2_varlen_plan_bytes(n, 1000), dtype=np.uint8)
        assert lib.fa2_varlen_plan_build(self.cq.ctypes.data, n, self.one.ctypes.data, self.one.size) == 0
        self.two = np.zeros(lib.fa2_varlen_plan_bytes_qk(n, 1000, 1100), dtype=np.uint8)
        assert lib.fa2_varlen_plan_build_qk(self.cq.ctypes.data, self.ck.ctypes.data, n, self.two.ctypes.data, self.two.size) == 0
        self.arrays = {k: (ctypes.c_void_p * 8)(*v) for k, v in PART_ADDR.items()}


def _dense(fn, d, N, causal, g=1, Nk=None, dtype=BF16, phases=7, **over):
    """A dense call of `fn` with every tensor present: what its names ask for, from this one description."""
    v = dict(ADDR, B=B, H=H, H_kv=H // g, seq_len=N, q_len=N, kv_len=Nk or N, head_dim=d, scale=0.125, dtype=dtype, causal=causal,
             stream=STREAM, ws_bytes=BIG, phases=phases, mode=1, q_hs=0, k_hs=0, q_row0=0, shift=0, first=0, last=1,
             q_descale=0.5, k_descale=2.0, v_descale=0.25, rows=B * H * N, kv_capacity=Nk or 4096, n_splits=4, reason=None)
    v.update(over)
    return fn, v


def _packed(fn, plans, two_sided, d, causal, g=1, **over):
    plan = plans.two if two_sided else plans.one
    v = dict(ADDR, H=H, H_kv=H // g, total_q=1000, total_k=1100 if two_sided else 1000, head_dim=d, scale=0.125, dtype=BF16,
             causal=causal, plan_host=plan.ctypes.data, plan_bytes=plan.size, stream=STREAM, ws_bytes=BIG)
    v.update(over)
    return fn, v


def _merge(fn, plans, n, d, **over):
    v = dict(ADDR, n_parts=n, rows=B * H * 300, head_dim=d, dtype=BF16, stream=STREAM,
             **{k: ctypes.addressof(a) for k, a in plans.arrays.items()})
    v.update(over)
    return fn, v


LSE = [dict(), dict(dL=None), dict(sink=None, dsink=None), dict(sink=None, dsink=None, dL=None), dict(sink=None), dict(dsink=None)]
DENSE_N = (256, 300, 1024, 8000)
LEAVE = lambda n: 16 | ((n & 0xff) << 8)      # FA2_PHASE_LEAVE_CUS


def valid_calls(plans, section):
    """(device_ok, fn, values) of every valid call.  `section`: "main", or "two_kernel" -- the backward rows alone, for the
    process that runs with FA2_BACKWARD_PATH=two_kernel."""
    calls = []
    add = lambda ok, call: calls.append((ok,) + call)
    if section == "main":
        for d, N, c in itertools.product((64, 128), DENSE_N, (0, 1)):
            add(1, _dense("fa2_forward", d, N, c))
            for g in (1, 4):
                for fn in ("fa2_forward_gqa", "fa2_forward_qk", "fa2_forward_sink"):
                    add(1, _dense(fn, d, N, c, g))
        for d, g, c, (Nq, Nk) in itertools.product((64, 128), (1, 4), (0, 1), ((160, 288), (288, 160))):
            add(1, _dense("fa2_forward_qk", d, Nq, c, g, Nk))
            add(1, _dense("fa2_forward_sink", d, Nq, c, g, Nk))
        for c in (0, 1):
            add(1, _dense("fa2_forward", 72, 300, c, dtype=F32))
            add(1, _dense("fa2_forward_fp8", 128, 300, c))
            add(1, _dense("fa2_forward_fp8_scaled", 128, 1024, c))
        for dtype, d in ((BF16, 64), (BF16, 128), (F32, 72)):
            for first, last in itertools.product((0, 1), (0, 1)):
                add(1, _dense("fa2_forward_step", d, 300, 0, Nk=512, dtype=dtype, first=first, last=last))
        for d, c, (qs, ks, sh) in itertools.product((64, 128), (0, 1), ((0, 0, 0), (600, 1024, 212))):
            add(1, _dense("fa2_forward_step_strided", d, 300, c, Nk=512, first=1, last=1, q_hs=qs, k_hs=ks, shift=sh))
            add(1, _dense("fa2_forward_step_strided", d, 300, c, Nk=512, first=0, last=0, q_hs=qs, k_hs=ks, shift=sh, O=None))
        for d in (64, 128):
            add(1, _dense("fa2_forward_state_finalize", d, 300, 0))
        # packed forward: either plan through every entry point that takes it (a two-sided plan through the one-list call: refused)
        for d, g, c in itertools.product((64, 128), (1, 4), (0, 1)):
            add(1, _packed("fa2_forward_varlen", plans, False, d, c, g))
            for two in (False, True):
                add(1, _packed("fa2_forward_varlen_qk", plans, two, d, c, g))
                add(1, _packed("fa2_forward_varlen_sink", plans, two, d, c, g))
        add(1, _packed("fa2_forward_varlen", plans, True, 128, 0, total_q=1000))
        # decode: 1, 4 and default splits, with and without lengths and sinks
        for d, g, ns, c in itertools.product((64, 128), (1, 4), (1, 4, 0), (0, 1)):
            add(1, _dense("fa2_forward_decode", d, 2, c, g, n_splits=ns))
            add(1, _dense("fa2_forward_decode", d, 1, c, g, n_splits=ns, seqlens=None, sink=None, kv_capacity=1000))
        add(1, _dense("fa2_forward_decode", 128, 1, 1, 4, n_splits=1, ws=None, ws_bytes=0))
        add(1, _dense("fa2_forward_decode", 128, 16, 1, 4))      # 64 rows: more than a tile
        for d, n in itertools.product((64, 128), (1, 8)):
            add(1, _merge("fa2_merge_states", plans, n, d))
            add(1, _merge("fa2_merge_states_backward", plans, n, d))
            add(1, _merge("fa2_merge_states_backward", plans, n, d, dL=None))
        # the sizes the callers allocate by
        for d, N, g in itertools.product((64, 128), DENSE_N, (1, 4)):
            for fn in ("fa2_backward_workspace_bytes", "fa2_backward_fused_workspace_bytes", "fa2_backward_gqa_workspace_bytes",
                       "fa2_backward_qk_workspace_bytes", "fa2_backward_sink_workspace_bytes"):
                if g == 1 or "H_kv" in NAMES[fn]:
                    add(1, _dense(fn, d, N, 0, g))
            add(1, _dense("fa2_backward_qk_workspace_bytes", d, N, 0, g, Nk=N + 32))
        for fn in ("fa2_backward_varlen_workspace_bytes", "fa2_backward_varlen_qk_workspace_bytes", "fa2_backward_varlen_sink_workspace_bytes"):
            add(1, _packed(fn, plans, True, 128, 0, 4))
        add(1, ("fa2_varlen_plan_bytes", dict(n_seqs=4, total_q=1000)))
        add(1, ("fa2_varlen_plan_bytes_qk", dict(n_seqs=4, total_q=1000, total_k=1100)))
    # ---- the backward, with device_ok true and false
    # (in full with device_ok true in the main section; a causal subset with device_ok false and under FA2_BACKWARD_PATH)
    for ok in (1, 0):
        full = ok == 1 and section == "main"
        Ns, cs = (DENSE_N, (0, 1)) if full else ((256, 8000), (1,))
        for d, N, c in itertools.product((64, 128), Ns, cs):
            add(ok, _dense("fa2_backward", d, N, c))
            add(ok, _dense("fa2_backward_phases", d, N, c))
            for g in (1, 4):
                for fn in ("fa2_backward_gqa", "fa2_backward_qk", "fa2_backward_sink"):
                    add(ok, _dense(fn, d, N, c, g))
                for lse in LSE[:4] if N in (300, 8000) and c else LSE[:1]:
                    add(ok, _dense("fa2_backward_lse", d, N, c, g, **lse))
            for mode in (0, 1, 2):
                add(ok, _dense("fa2_backward_fused", d, N, c, mode=mode))
        for d, N, g in itertools.product((64, 128), (256, 300), (1, 4)):
            for ph in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 7 | 16) if full else (6, 8, 9, 7 | 16):
                add(ok, _dense("fa2_backward_gqa", d, N, 1, g, phases=ph))
                add(ok, _dense("fa2_backward_qk", d, N, 1, g, phases=ph))
                if g == 1:
                    add(ok, _dense("fa2_backward_phases", d, N, 1, phases=ph))
        # the rectangle: the two kernels, whatever is asked
        for d, g, c, (Nq, Nk) in itertools.product((64, 128), (1, 4), cs, ((160, 288), (288, 160))):
            add(ok, _dense("fa2_backward_qk", d, Nq, c, g, Nk))
            add(ok, _dense("fa2_backward_sink", d, Nq, c, g, Nk))
            for lse in LSE if full else LSE[:1]:
                add(ok, _dense("fa2_backward_lse", d, Nq, c, g, Nk, **lse))
        for ph in (1, 2, 4, 6, 8, 9, 7 | 16):
            add(ok, _dense("fa2_backward_qk", 128, 160, 1, 4, 288, phases=ph))
        for N, c, ph in itertools.product((300, 1024), cs, (7, 1, 6, 8)):
            add(ok, _dense("fa2_backward", 72, N, c, dtype=F32) if ph == 7 else _dense("fa2_backward_phases", 72, N, c, dtype=F32, phases=ph))
        # fa2_backward_block: square, rect and strided; with room for a control block and without
        blocks = (dict(N=1024), dict(N=1024, shift=0), dict(N=1024, shift=256), dict(N=512, Nk=256, q_hs=1024, k_hs=256, q_row0=512),
                  dict(N=512, Nk=1024, q_hs=1024, q_row0=0), dict(N=300, Nk=300, q_hs=2048, k_hs=2048, q_row0=256, shift=-44),
                  dict(N=500, Nk=256, q_hs=1000, q_row0=500))
        for d, c, blk, ph in itertools.product((64, 128), (0, 1), blocks, (7, 6, 3, 7 | 16, 6 | LEAVE(8), 7 | LEAVE(0)) if full else (7, 6 | LEAVE(8))):
            blk = dict(blk)
            N = blk.pop("N")
            add(ok, _dense("fa2_backward_block", d, N, c, phases=ph, **blk))
            if ph == 7:
                add(ok, _dense("fa2_backward_block", d, N, c, phases=ph, ws_bytes=3 * 4 * B * H * (blk.get("q_hs") or N) + 3 * 256, **blk))
        # the packed backward: both plans through every entry point that takes them
        for d, g, c in itertools.product((64, 128), (1, 4), cs):
            add(ok, _packed("fa2_backward_varlen", plans, False, d, c, g))
            for two in (False, True):
                add(ok, _packed("fa2_backward_varlen_qk", plans, two, d, c, g))
                add(ok, _packed("fa2_backward_varlen_sink", plans, two, d, c, g))
                for lse in LSE if full else LSE[:1]:
                    add(ok, _packed("fa2_backward_varlen_lse", plans, two, d, c, g, **lse))
        add(ok, _packed("fa2_backward_varlen", plans, True, 128, 0, total_q=1000))
        for d, N, dtype, g in itertools.product((64, 128), DENSE_N, (BF16, F32), (1, 4)):
            add(ok, _dense("fa2_backward_gqa_plan" if g > 1 else "fa2_backward_plan", d, N, 1, g, dtype=dtype, reason="why"))
    return calls


def baselines(plans):
    """One valid call per entry point that validates: what the invalid rows start from.  Every pointer present, a workspace
    that is needed (decode: 4 splits), an interior head_dim / N."""
    dense = ("fa2_forward fa2_forward_gqa fa2_forward_qk fa2_forward_sink fa2_forward_fp8 fa2_forward_fp8_scaled fa2_forward_step "
             "fa2_forward_step_strided fa2_forward_decode fa2_backward fa2_backward_phases fa2_backward_gqa fa2_backward_qk "
             "fa2_backward_sink fa2_backward_lse fa2_backward_block fa2_backward_fused fa2_backward_plan fa2_backward_gqa_plan").split()
    out = [_dense(fn, 128, 1024 if "decode" not in fn else 2, 1 if fn != "fa2_backward_fused" else 0, 4, reason="why") for fn in dense]
    out += [_packed(fn, plans, fn != "fa2_forward_varlen" and fn != "fa2_backward_varlen", 128, 1, 4)
            for fn in ("fa2_forward_varlen", "fa2_forward_varlen_qk", "fa2_forward_varlen_sink", "fa2_backward_varlen",
                       "fa2_backward_varlen_qk", "fa2_backward_varlen_sink", "fa2_backward_varlen_lse")]
    out += [_merge(fn, plans, 8, 128) for fn in ("fa2_merge_states", "fa2_merge_states_backward")]
    return out


def invalid_combos(fn):
    """Every invalid row of one entry point as ((field, value), ...): each field, then each pair of fields."""
    fields = []
    for name in NAMES[fn]:
        if name in POINTERS and name not in OPTIONAL.get(fn, ()):
            fields.append((name, [None]))
        elif name in INVALID:
            fields.append((name, INVALID[name]))
    single = [((n, x),) for n, xs in fields for x in xs]
    return single + [a + b for a, b in itertools.combinations(single, 2) if a[0][0] != b[0][0]]


def invalid_rows(fn, values):
    for combo in invalid_combos(fn):
        v = dict(values)
        for n, x in combo:
            v[n] = x
            if n == "ws":
                v["ws_bytes"] = 0
        yield v


# ---- running them ---------------------------------------------------------------------------------------------------------
class Lib:
    def __init__(self, path):
        self.h = ctypes.CDLL(path)
        self.sig = _signatures()
        for name, (res, args) in self.sig.items():
            f = getattr(self.h, name)
            f.restype, f.argtypes = res, args
        self.h.fa2_stub_log.restype = ctypes.c_char_p
        for fn, names in NAMES.items():
            assert len(names) == len(self.sig[fn][1]), fn

    def call(self, ok, fn, values):
        """(label, status, records) of one call."""
        self.h.fa2_stub_reset()
        self.h.fa2_stub_set_device_ok(ok)
        why = ctypes.c_char_p()
        args = [ctypes.byref(why) if n == "reason" and values[n] else values[n] for n in NAMES[fn]]
        status = getattr(self.h, fn)(*args)
        records = self.h.fa2_stub_log().decode()
        if why.value is not None:
            records += "why=" + why.value.decode()
        shown = []
        for n in NAMES[fn]:      # the numbers, and which pointers are NULL
            pointer = n in ADDR or n in POINTERS or n == "reason"
            if n != "stream" and (values[n] is None or not pointer):
                shown.append(f"{n}={0 if pointer else values[n]}")
        shown = " ".join(shown)
        return f"{fn} ok={ok} {shown}", status, records


def run(path, section="main"):
    """The fixture's lines for one process: 'V <call> | <status> | <records>' per valid call and, in the main section,
    'I <entry point> | <one digit per invalid row: -status>'."""
    lib = Lib(path)
    plans = Plans(lib.h)
    lines = []
    for ok, fn, values in valid_calls(plans, section):
        label, status, records = lib.call(ok, fn, values)
        lines.append(f"V {label} | {status} | {records}")
    if section == "main":
        for fn, values in baselines(plans):
            label, status, records = lib.call(1, fn, values)
            assert status in (0, 1, 2) and (records or "plan" in fn), (label, status)      # the baseline itself is valid
            digits = []
            for v in invalid_rows(fn, values):
                _, status, records = lib.call(1, fn, v)
                assert not records.replace("why=", ""), (fn, v)
                digits.append(str(-status) if -9 <= status <= 0 else "?")
            lines.append(f"I {fn} | {''.join(digits)}")
    return [f"{section[0].upper()}{line}" for line in lines]


def run_child(path, section):
    """run() in a process of its own, with FA2_BACKWARD_PATH as the section asks."""
    env = {k: v for k, v in os.environ.items() if k != "FA2_BACKWARD_PATH"}
    if section == "two_kernel":
        env["FA2_BACKWARD_PATH"] = "two_kernel"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "run", path, section], env=env, check=True, capture_output=True, text=True)
    return out.stdout.splitlines()


def record_all(path):
    return run_child(path, "main") + run_child(path, "two_kernel")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "build":
        print(build(sys.argv[2], sys.argv[3]))
    elif cmd == "run":
        print("\n".join(run(sys.argv[2], *sys.argv[3:4])))
    elif cmd == "record":
        with tempfile.TemporaryDirectory() as tmp:
            lines = record_all(build(sys.argv[2], tmp))
        with gzip.GzipFile(FIXTURE, "wb", mtime=0) as f:
            f.write(("\n".join(lines) + "\n").encode())
        print(f"{FIXTURE}: {len(lines)} lines")
