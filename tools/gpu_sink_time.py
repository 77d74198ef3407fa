"""What attention sinks cost, timed in ONE process on one device (dev aid; bench.py is untouched; the method of
tools/gpu_qk_time.py).

    python tools/gpu_sink_time.py [--out profiles/sink_times.json] [--min-launches 40] [--min-seconds 1.0]

Shapes (B, H, N, d) = (4, 16, 8192, 128) and (4, 16, 4096, 64), multi-head, plain and causal.  Sinks: finite on every head
(log N + {-1, 0, 1, 3}, cycled), so every row block takes the sink's branch of the epilogue.  For the forward and the backward
(phases 7: what the routing rule picks) separately:
    plain    the _qk call without a sink
    plain2   a second copy of it: plain against plain2 is the spread of the method on this box
    sink     the same call with sink= (and dsink=)
and for the sinks' gradient kernel alone:
    d        the backward with phases = 1 (the D kernel), without a sink
    d_sink   the same with the sinks: the D kernel and fa2_bwd_dsink_kernel behind it; d_sink - d is the kernel's own time
Variants alternate in blocks of a few launches (order reversed every other round) after a warm-up; every variant gets at least
--min-launches timed launches and --min-seconds of timed work; medians of the per-launch block times are reported.
Expectations, each against the SAME run: forward sink - plain within the spread; backward sink - plain within the spread plus the
dsink kernel's own time.  Nothing is fixed in advance: the medians and the verdicts go into the JSON, whatever they are."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402

SHAPES = ((4, 16, 8192, 128), (4, 16, 4096, 64))
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


def one_case(shape, causal, min_launches, min_seconds):
    B, H, N, D = shape
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(2468)
    s = 1.0 / D ** 0.5
    mk = lambda sc: ((torch.rand(B, H, N, D, device=dev, generator=g) - 0.5) * sc).bfloat16()
    Q, K, V, dO = mk(1.0), mk(1.0), mk(1.0), mk(0.4)
    sink = torch.tensor([math.log(N) + (-1.0, 0.0, 1.0, 3.0)[h % 4] for h in range(H)], dtype=torch.float32, device=dev)
    lib = fa._capi.lib()
    need = lib.fa2_backward_sink_workspace_bytes(B, H, H, N, N, D, 0)

    def variant(sk):
        """(forward, backward(phases)) on tensors, outputs and a workspace of the variant's own."""
        O, L = torch.empty_like(Q), torch.empty(B, H, N, dtype=torch.float32, device=dev)
        dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        kw = {} if sk is None else {"sink": sk, "dsink": torch.empty(H, dtype=torch.float32, device=dev)}
        f = lambda: fa.flash_attention_2_qk_forward(Q, K, V, s, causal=causal, O=O, L=L, **({} if sk is None else {"sink": sk}))
        b = lambda ph: fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=ph, **kw)
        return f, b

    (fp, bp), (fs, bs) = variant(None), variant(sink)
    fwd = {"plain": fp, "plain2": fp, "sink": fs}
    bwd = {"plain": lambda: bp(7), "plain2": lambda: bp(7), "sink": lambda: bs(7)}
    dk = {"d": lambda: bp(1), "d2": lambda: bp(1), "d_sink": lambda: bs(1)}
    for f in fwd.values():             # O, L of every variant exist before a backward is timed
        f()
    tf, tb, td = (time_variants(c, min_launches, min_seconds) for c in (fwd, bwd, dk))
    torch.cuda.synchronize()
    ms = lambda t: {k: round(v[0], 4) for k, v in t.items()}
    f, b, d = ms(tf), ms(tb), ms(td)
    dsink_ms = round(d["d_sink"] - d["d"], 4)
    res = {"shape": list(shape), "causal": causal, "backward_plan": lib.fa2_backward_plan(B, H, N, D, 0, int(causal), None),
           "forward_ms": f, "backward_ms": b, "d_kernel_ms": d,
           "launches": {"forward": {k: v[1] for k, v in tf.items()}, "backward": {k: v[1] for k, v in tb.items()},
                        "d_kernel": {k: v[1] for k, v in td.items()}},
           "forward_spread_ms": round(abs(f["plain"] - f["plain2"]), 4), "backward_spread_ms": round(abs(b["plain"] - b["plain2"]), 4),
           "d_kernel_spread_ms": round(abs(d["d"] - d["d2"]), 4), "dsink_kernel_ms": dsink_ms,
           "forward_sink_minus_plain_ms": round(f["sink"] - f["plain"], 4), "backward_sink_minus_plain_ms": round(b["sink"] - b["plain"], 4)}
    res["expect_forward_within_spread"] = res["forward_sink_minus_plain_ms"] <= res["forward_spread_ms"]
    res["expect_backward_within_spread_plus_dsink"] = res["backward_sink_minus_plain_ms"] <= res["backward_spread_ms"] + max(dsink_ms, 0.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sink_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); plain2 / d2 are second copies of plain / d (the spread)",
           "cases": []}
    for shape in SHAPES:
        for causal in (False, True):
            r = one_case(shape, causal, a.min_launches, a.min_seconds)
            res["cases"].append(r)
            print(f"{shape} causal={causal}: fwd {r['forward_ms']} | bwd {r['backward_ms']} | D {r['d_kernel_ms']} | "
                  f"{ {k: v for k, v in r.items() if k.startswith('expect_')} }", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
