"""Extend attention: the two-row-tile body against the grid-only form, in ONE process on one device (dev aid; the method and
time_variants of tools/gpu_decode_time.py, the shapes of tools/gpu_extend_time.py).

    python tools/gpu_extend_ab.py VARIANT.so [--out profiles/extend_rows_ab.json] [--min-launches 40] [--min-seconds 0.25]

VARIANT.so: a build of the library with -DFA2_EXTEND_ROWS=32 (one 32-row tile per wave, a workgroup per 32 rows: twice the
workgroups, every K/V byte streamed once per 32 rows), linked -Bsymbolic so that it binds its own kernels.  The product library
(64 rows per workgroup, two tiles per wave) is the other arm.  Both are called through fa2_forward_extend / _paged with
n_splits = 0 (each build's own default) on the same tensors; every arm twice, |x - x2| is the spread.  The outputs of the two
builds are compared bit for bit where their default split counts agree (a row's arithmetic does not depend on its tile)."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from cuda_flashattention_amd import _capi  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402
from gpu_extend_time import D, LENS, PAGE, SHAPES, caches, paged  # noqa: E402


def load(path):
    h = ctypes.CDLL(os.path.abspath(path), mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in _capi.EXTEND_SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    return h


def call(lib, Q, K, V, table, lens, fp8):
    B, hq, nq, _ = Q.shape
    hkv = K.shape[1]
    cap = K.shape[2] if table is None else table.shape[1] * PAGE
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device=Q.device)
    ws = torch.empty(max(lib.fa2_extend_workspace_bytes(B, hq, hkv, nq, cap, D, 0, -1), 16), dtype=torch.uint8, device=Q.device)
    kd = torch.full((hkv,), 1 / 64, device=Q.device) if fp8 else None
    ptr = lambda t: None if t is None else t.data_ptr()
    kv = 2 if fp8 else 0
    tail = (ctypes.c_float(1.0 / D ** 0.5), 0, kv, 1, 0, ws.data_ptr(), ws.numel(), None, -1)

    def run():
        if table is None:
            st = lib.fa2_forward_extend(Q.data_ptr(), K.data_ptr(), V.data_ptr(), lens.data_ptr(), None, ptr(kd), ptr(kd), O.data_ptr(), L.data_ptr(),
                                        B, hq, hkv, nq, cap, D, *tail)
        else:
            st = lib.fa2_forward_extend_paged(Q.data_ptr(), K.data_ptr(), V.data_ptr(), table.data_ptr(), lens.data_ptr(), None, ptr(kd), ptr(kd),
                                              O.data_ptr(), L.data_ptr(), B, hq, hkv, nq, K.shape[0], PAGE, table.shape[1], D, *tail)
        assert st == 0, st
    return run, (O, L, kd, ws), lib.fa2_extend_num_splits(B, hq, hkv, nq, cap, D, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "extend_rows_ab.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    two, one = _capi.lib(), load(a.variant)
    g = torch.Generator(device="cuda").manual_seed(8642)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"two": "the product library: 64 rows per workgroup, two row tiles per wave",
                    "one": "-DFA2_EXTEND_ROWS=32: 32 rows per workgroup, one row tile per wave (the grid-only form)"},
           "cases": []}
    for name, B, hq, hkv, nq in SHAPES:
        for n in LENS:
            for is_paged in (False, True):
                for fp8 in (False, True):
                    dev = torch.device("cuda")
                    Q = (torch.rand(B, hq, nq, D, device=dev, generator=g) - 0.5).bfloat16()
                    K, V = caches(B, hkv, n, fp8, g)
                    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                    table = None
                    if is_paged:
                        K, V, table = paged(K, V, g)
                    f2, out2, s2 = call(two, Q, K, V, table, lens, fp8)
                    f1, out1, s1 = call(one, Q, K, V, table, lens, fp8)
                    f2(), f1()
                    torch.cuda.synchronize()
                    same = bool(torch.equal(out2[0].view(torch.int16), out1[0].view(torch.int16)) and
                                torch.equal(out2[1].view(torch.int32), out1[1].view(torch.int32)))
                    t = time_variants({"two": f2, "one": f1, "two2": f2, "one2": f1}, a.min_launches, a.min_seconds)
                    spread = {k: abs(t[k] - t[k + "2"]) for k in ("two", "one")}
                    r = {"shape": name, "B": B, "H_q": hq, "H_kv": hkv, "q_len": nq, "len": n, "kv": "e4m3" if fp8 else "bf16",
                         "layout": "paged" if is_paged else "contiguous", "n_splits": {"two": s2, "one": s1},
                         "same_bits": same if s1 == s2 else None,
                         "ms": {k: round(v, 5) for k, v in t.items()}, "spread_ms": {k: round(v, 5) for k, v in spread.items()},
                         "two_over_one": round(t["two"] / t["one"], 4),
                         "two_slower_beyond_spread": bool(min(t["two"], t["two2"]) > max(t["one"], t["one2"]) + max(spread.values()))}
                    res["cases"].append(r)
                    print(json.dumps(r), flush=True)
                    del K, V, Q, out1, out2
                    torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
