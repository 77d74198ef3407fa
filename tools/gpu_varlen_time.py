"""Packed variable-length attention against the workarounds, timed in ONE process on one device (dev aid; bench.py is untouched).

    python tools/gpu_varlen_time.py [--out profiles/varlen_times.json] [--min-launches 40] [--min-seconds 1.0]

H = 16 heads (multi-head), d = 128, T = 16384 rows per head, causal and not, two length sets:
    uniform  8 x 2048
    skewed   8192, 4096, 2048, 1024, 512, 256, 128, 128
For the forward and the backward separately:
    a       the packed call (one launch sequence over the whole batch; the backward is D + the dQ and dK/dV kernels)
    b       what a caller had to do before: a loop of dense calls, one per sequence on its own [1, H, len, d] tensors (made
            beforehand, untimed); the backward with phases 1, then 6 -- the same two kernels, so the comparison is kernel for kernel
    b2      a second copy of b: b against b2 is the spread of the method on this box
    c       uniform only: the dense [8, H, 2048, d] call; the backward with phases 1, then 6
    c_rule  uniform only, backward only, information: the dense backward under the routing rule (the single five-product
            kernel at this shape) -- what the packed backward leaves on the table until that kernel takes ragged units
Variants alternate in blocks of a few launches (order reversed every other round) after a warm-up; every variant gets at
least --min-launches timed launches and --min-seconds of timed work; medians of the per-launch block times are reported.
Expectations, each against the SAME run's baseline: skewed, forward and backward: a <= b; uniform non-causal forward:
a <= c + |b - b2| (the same workgroups do the same work after one table lookup).  Uniform causal is information (the packed
forward runs one row block per workgroup, the dense causal launch pairs them).  Writes the JSON and prints a summary."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402

H, D = 16, 128
SETS = {"uniform": (2048,) * 8, "skewed": (8192, 4096, 2048, 1024, 512, 256, 128, 128)}
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


def one_case(name, causal, min_launches, min_seconds):
    dev = torch.device("cuda")
    lengths = SETS[name]
    T = sum(lengths)
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    g = torch.Generator(device=dev).manual_seed(4321)
    mk = lambda s: ((torch.rand(H, T, D, device=dev, generator=g) - 0.5) * s).bfloat16()
    Q, K, V, dO = mk(1.0), mk(1.0), mk(1.0), mk(0.4)
    s = 1.0 / D ** 0.5
    lib = fa._capi.lib()
    plan = fa.VarlenPlan(cu)

    # a: the packed tensors
    O, L = torch.empty_like(Q), torch.empty(H, T, dtype=torch.float32, device=dev)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    ws = torch.empty(lib.fa2_backward_varlen_workspace_bytes(H, H, T, D, 0), dtype=torch.uint8, device=dev)
    fwd_a = lambda: fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal, O=O, L=L)
    bwd_a = lambda: fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws)

    # b: every sequence as a dense problem of its own
    def dense(B, N, src):
        """Tensors, outputs and workspace of a dense [B, H, N, d] problem cut from rows src of the packed tensors, and its calls."""
        cut = lambda t: torch.stack([t[:, r0:r0 + N] for r0 in src]).contiguous()
        q, k, v, go = cut(Q), cut(K), cut(V), cut(dO)
        o, l = torch.empty_like(q), torch.empty(B, H, N, dtype=torch.float32, device=dev)
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        w = torch.empty(lib.fa2_backward_workspace_bytes(B, H, N, D, 0), dtype=torch.uint8, device=dev)
        f = lambda: fa.flash_attention_2_forward(q, k, v, s, causal=causal, O=o, L=l)
        b = lambda ph: fa.flash_attention_2_backward(q, k, v, o, l, go, s, causal=causal, dQ=gq, dK=gk, dV=gv, workspace=w, phases=ph)
        return f, b

    per_seq = [dense(1, n, (r0,)) for r0, n in zip(cu, lengths)]

    def fwd_b():
        for f, _ in per_seq:
            f()

    def bwd_b():
        for _, b in per_seq:
            b(1)
            b(6)

    fwd_calls = {"a": fwd_a, "b": fwd_b, "b2": fwd_b}
    bwd_calls = {"a": bwd_a, "b": bwd_b, "b2": bwd_b}
    if name == "uniform":
        fc, bc = dense(len(lengths), lengths[0], cu[:-1])
        fwd_calls["c"] = fc
        bwd_calls["c"] = lambda: (bc(1), bc(6))
        bwd_calls["c_rule"] = lambda: bc(7)
        fc()
    fwd_a()
    fwd_b()                            # O, L of every variant exist before a backward is timed
    tf = time_variants(fwd_calls, min_launches, min_seconds)
    tb = time_variants(bwd_calls, min_launches, min_seconds)
    torch.cuda.synchronize()
    ms = lambda t: {k: round(v[0], 4) for k, v in t.items()}
    f, b = ms(tf), ms(tb)
    res = {"lengths": name, "lengths_list": list(lengths), "shape": [H, T, D], "causal": bool(causal),
           "row_items": int(plan.row_items.shape[0]), "key_items": int(plan.key_items.shape[0]),
           "forward_ms": f, "backward_ms": b,
           "launches": {"forward": {k: v[1] for k, v in tf.items()}, "backward": {k: v[1] for k, v in tb.items()}},
           "timed_seconds": {"forward": {k: round(v[2], 2) for k, v in tf.items()}, "backward": {k: round(v[2], 2) for k, v in tb.items()}},
           "forward_spread_ms": round(abs(f["b"] - f["b2"]), 4), "backward_spread_ms": round(abs(b["b"] - b["b2"]), 4),
           "forward_a_over_b": round(f["a"] / f["b"], 4), "backward_a_over_b": round(b["a"] / b["b"], 4)}
    if name == "skewed":
        res["expect_forward_a_le_b"] = f["a"] <= f["b"]
        res["expect_backward_a_le_b"] = b["a"] <= b["b"]
    else:
        res["forward_a_over_c"] = round(f["a"] / f["c"], 4)
        res["backward_a_over_c"] = round(b["a"] / b["c"], 4)
        res["backward_a_over_c_rule"] = round(b["a"] / b["c_rule"], 4)
        if not causal:
            res["expect_forward_a_le_c_plus_spread"] = f["a"] <= f["c"] + abs(f["b"] - f["b2"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "varlen_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms)",
           "cases": []}
    for name in SETS:
        for causal in (False, True):
            r = one_case(name, causal, a.min_launches, a.min_seconds)
            res["cases"].append(r)
            verdicts = {k: v for k, v in r.items() if k.startswith("expect_")}
            print(f"{name} causal={int(causal)}: fwd {r['forward_ms']} | bwd {r['backward_ms']} | a/b fwd {r['forward_a_over_b']} "
                  f"bwd {r['backward_a_over_b']} | {verdicts if verdicts else 'information'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
