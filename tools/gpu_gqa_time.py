"""Grouped-query attention against the workaround, timed in ONE process on one device (dev aid; bench.py is untouched).

    python tools/gpu_gqa_time.py [--out profiles/gqa_times.json] [--min-launches 40] [--min-seconds 1.0]

Shapes (B, H_q -> H_kv, N, d): (4, 16 -> 4, 8192, 128) and (2, 32 -> 8, 8192, 128), causal and not.  For the forward and the
backward separately:
    a   the grouped call (K, V, dK, dV with H_kv heads)
    b   the multi-head call on PRE-EXPANDED K, V -- the kernels alone, the expansion untimed
    b2  a second copy of b: b against b2 is the spread of the method on this box
    c   what a caller had to do before: repeat_interleave of K and V + the multi-head forward; the multi-head backward +
        the sum of dK / dV over each group in torch
Variants alternate in blocks of a few launches (order reversed every other round) after a warm-up; every variant gets at
least --min-launches timed launches and --min-seconds of timed work; medians of the per-launch block times are reported.
Expectations, each against the SAME run's baseline: forward a <= b + |b - b2|; forward + backward a <= c.  backward a / b is
information (the price of the reduction pass or of the group loop).  Writes the JSON and prints a four-line summary."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402

SHAPES = ((4, 16, 4, 8192, 128), (2, 32, 8, 8192, 128))
BLOCK = 5          # launches between two events


def time_variants(calls, min_launches, min_seconds):
    """calls: name -> callable.  Returns name -> (median ms per launch, launches, timed seconds)."""
    names = list(calls)
    for n in names:                    # code-object load, clock ramp
        for _ in range(3):
            calls[n]()
    torch.cuda.synchronize()
    blocks = {n: [] for n in names}
    rnd = 0
    while any(len(blocks[n]) * BLOCK < min_launches or sum(blocks[n]) * BLOCK < min_seconds * 1e3 for n in names):
        for n in (names if rnd % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                calls[n]()
            e1.record()
            e1.synchronize()
            blocks[n].append(e0.elapsed_time(e1) / BLOCK)
        rnd += 1
    return {n: (statistics.median(blocks[n]), len(blocks[n]) * BLOCK, sum(blocks[n]) * BLOCK / 1e3) for n in names}


def one_shape(B, Hq, Hkv, N, d, causal, min_launches, min_seconds):
    dev = torch.device("cuda")
    G = Hq // Hkv
    g = torch.Generator(device=dev).manual_seed(4321)
    mk = lambda h, s: ((torch.rand(B, h, N, d, device=dev, generator=g) - 0.5) * s).bfloat16()
    Q, K, V, dO = mk(Hq, 1.0), mk(Hkv, 1.0), mk(Hkv, 1.0), mk(Hq, 0.4)
    Ke, Ve = K.repeat_interleave(G, dim=1).contiguous(), V.repeat_interleave(G, dim=1).contiguous()
    s = 1.0 / d ** 0.5
    lib = fa._capi.lib()
    O, L = torch.empty_like(Q), torch.empty(B, Hq, N, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.fa2_backward_gqa_workspace_bytes(B, Hq, Hkv, N, d, 0), dtype=torch.uint8, device=dev)
    dQ, dKg, dVg, dKe, dVe = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V), torch.empty_like(Ke), torch.empty_like(Ve)
    fwd = lambda k, v: fa.flash_attention_2_forward(Q, k, v, s, causal=causal, O=O, L=L)
    bwd = lambda k, v, dk, dv: fa.flash_attention_2_backward(Q, k, v, O, L, dO, s, causal=causal, dQ=dQ, dK=dk, dV=dv, workspace=ws)

    def fwd_c():
        fwd(K.repeat_interleave(G, dim=1), V.repeat_interleave(G, dim=1))

    def bwd_c():
        bwd(Ke, Ve, dKe, dVe)
        return dKe.view(B, Hkv, G, N, d).sum(dim=2), dVe.view(B, Hkv, G, N, d).sum(dim=2)

    fwd(K, V)
    tf = time_variants({"a": lambda: fwd(K, V), "b": lambda: fwd(Ke, Ve), "b2": lambda: fwd(Ke, Ve), "c": fwd_c}, min_launches, min_seconds)
    tb = time_variants({"a": lambda: bwd(K, V, dKg, dVg), "b": lambda: bwd(Ke, Ve, dKe, dVe), "b2": lambda: bwd(Ke, Ve, dKe, dVe), "c": bwd_c},
                       min_launches, min_seconds)
    torch.cuda.synchronize()
    ms = lambda t: {k: round(v[0], 4) for k, v in t.items()}
    f, b = ms(tf), ms(tb)
    spread_f = abs(f["b"] - f["b2"])
    return {"shape": [B, Hq, Hkv, N, d], "causal": bool(causal),
            "backward_plan": lib.fa2_backward_gqa_plan(B, Hq, Hkv, N, d, 0, int(causal), None),
            "forward_ms": f, "backward_ms": b,
            "launches": {"forward": {k: v[1] for k, v in tf.items()}, "backward": {k: v[1] for k, v in tb.items()}},
            "timed_seconds": {"forward": {k: round(v[2], 2) for k, v in tf.items()}, "backward": {k: round(v[2], 2) for k, v in tb.items()}},
            "forward_spread_ms": round(spread_f, 4), "backward_spread_ms": round(abs(b["b"] - b["b2"]), 4),
            "forward_a_le_b_plus_spread": f["a"] <= f["b"] + spread_f,
            "fwd_bwd_a_le_c": f["a"] + b["a"] <= f["c"] + b["c"],
            "backward_a_over_b": round(b["a"] / b["b"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gqa_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms)",
           "cases": []}
    for B, Hq, Hkv, N, d in SHAPES:
        for causal in (False, True):
            r = one_shape(B, Hq, Hkv, N, d, causal, a.min_launches, a.min_seconds)
            res["cases"].append(r)
            f, b = r["forward_ms"], r["backward_ms"]
            print(f"({B},{Hq}->{Hkv},{N},{d}) causal={int(causal)}: fwd a {f['a']} b {f['b']} b2 {f['b2']} c {f['c']} | bwd a {b['a']} b {b['b']} "
                  f"b2 {b['b2']} c {b['c']} | fwd a<=b+spread {r['forward_a_le_b_plus_spread']}  fwd+bwd a<=c {r['fwd_bwd_a_le_c']}  "
                  f"bwd a/b {r['backward_a_over_b']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
