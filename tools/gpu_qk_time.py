"""Attention over different query and key lengths against the workarounds, timed in ONE process on one device (dev aid; bench.py
is untouched; the method of tools/gpu_varlen_time.py).

    python tools/gpu_qk_time.py [--out profiles/qk_times.json] [--min-launches 40] [--min-seconds 1.0]

H = 16 heads (multi-head), d = 128.  Two workloads:
    prefill  causal, a prompt chunk against a longer contiguous KV cache: 8 sequences of (len_q, len_k) = (512, 4096); and a
             skewed set, chunks of 512 rows at different depths of their sequences and two short ones
    cross    non-causal cross-attention: 8 sequences of (2048, 512); and a skewed set
For the forward and the backward separately:
    a       the packed two-sided call on the uniform set (one launch sequence over the whole batch)
    a'      the same on the skewed set, with its own b' / b2' (a loop over ITS sequences)
    b       a loop of dense _qk calls, one per sequence on its own [1, H, len, d] tensors (made beforehand, untimed); the backward
            with phases 1, then 6 -- the same two kernels
    b2      a second copy of b: b against b2 is the spread of the method on this box
    c       the dense _qk call [8, H, len_q | len_k, d]; the backward with phases 1, then 6
    p       what a caller had to do before this entry point existed: the SQUARE call on Q (and dO) padded with zero rows to
            max(len_q, len_k) per sequence -- for the prefill, in FRONT of the chunk, so that the square causal mask is the chunk's;
            for the cross-attention K and V padded behind instead, where a padded key still gets weight: p then computes something
            else and is timed as the cost of the square only.  Backward p: phases 1, then 6 (the same two kernels as c)
Variants alternate in blocks of a few launches (order reversed every other round) after a warm-up; every variant gets at least
--min-launches timed launches and --min-seconds of timed work; medians of the per-launch block times are reported.
Expectations, each against the SAME run's baseline: a <= b and c <= p, forward and backward, both workloads.  Nothing is fixed in
advance: the medians and the verdicts go into the JSON, whatever they are."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402

H, D = 16, 128
WORKLOADS = {
    "prefill": {"causal": True, "uniform": ((512, 4096),) * 8,
                "skewed": ((512, 8192), (512, 6144), (512, 4096), (512, 2048), (512, 1024), (512, 512), (128, 4096), (64, 640))},
    "cross": {"causal": False, "uniform": ((2048, 512),) * 8,
              "skewed": ((4096, 512), (4096, 77), (2048, 512), (2048, 1024), (1024, 512), (512, 512), (256, 2048), (128, 77))},
}
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


def packed_and_loop(pairs, causal, g):
    """(forward, backward) of the packed two-sided call on `pairs` and of the loop of dense _qk calls over its sequences."""
    dev = torch.device("cuda")
    s = 1.0 / D ** 0.5
    cq, ck = [0], [0]
    for lq, lk in pairs:
        cq.append(cq[-1] + lq)
        ck.append(ck[-1] + lk)
    mk = lambda t, sc: ((torch.rand(H, t, D, device=dev, generator=g) - 0.5) * sc).bfloat16()
    Q, K, V, dO = mk(cq[-1], 1.0), mk(ck[-1], 1.0), mk(ck[-1], 1.0), mk(cq[-1], 0.4)
    plan = fa.VarlenPlan(cq, ck)
    lib = fa._capi.lib()
    O, L = torch.empty_like(Q), torch.empty(H, cq[-1], dtype=torch.float32, device=dev)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    ws = torch.empty(lib.fa2_backward_varlen_qk_workspace_bytes(H, H, cq[-1], ck[-1], D, 0), dtype=torch.uint8, device=dev)
    fwd_a = lambda: fa.flash_attention_2_varlen_forward(Q, K, V, plan, s, causal=causal, O=O, L=L)
    bwd_a = lambda: fa.flash_attention_2_varlen_backward(Q, K, V, O, L, dO, plan, s, causal=causal, dQ=dQ, dK=dK, dV=dV, workspace=ws)
    per_seq = []
    for i, (lq, lk) in enumerate(pairs):
        cut_q, cut_k = (lambda t, i=i: t[None, :, cq[i]:cq[i + 1]].contiguous()), (lambda t, i=i: t[None, :, ck[i]:ck[i + 1]].contiguous())
        per_seq.append(dense_calls(cut_q(Q), cut_k(K), cut_k(V), cut_q(dO), causal))

    def fwd_b():
        for f, _ in per_seq:
            f()

    def bwd_b():
        for _, b in per_seq:
            b(1)
            b(6)

    return (fwd_a, bwd_a), (fwd_b, bwd_b), plan


def dense_calls(q, k, v, go, causal, square=False):
    """(forward, backward(phases)) of a dense problem on its own tensors, outputs and workspace: the _qk calls, or (square) the calls
    a caller had before them."""
    s = 1.0 / D ** 0.5
    B, _, nq, _ = q.shape
    nk = k.shape[2]
    lib = fa._capi.lib()
    o, l = torch.empty_like(q), torch.empty(B, H, nq, dtype=torch.float32, device=q.device)
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if square:
        w = torch.empty(lib.fa2_backward_workspace_bytes(B, H, nq, D, 0), dtype=torch.uint8, device=q.device)
        f = lambda: fa.flash_attention_2_forward(q, k, v, s, causal=causal, O=o, L=l)
        b = lambda ph: fa.flash_attention_2_backward(q, k, v, o, l, go, s, causal=causal, dQ=gq, dK=gk, dV=gv, workspace=w, phases=ph)
    else:
        w = torch.empty(lib.fa2_backward_qk_workspace_bytes(B, H, H, nq, nk, D, 0), dtype=torch.uint8, device=q.device)
        f = lambda: fa.flash_attention_2_qk_forward(q, k, v, s, causal=causal, O=o, L=l)
        b = lambda ph: fa.flash_attention_2_qk_backward(q, k, v, o, l, go, s, causal=causal, dQ=gq, dK=gk, dV=gv, workspace=w, phases=ph)
    return f, b


def one_workload(name, min_launches, min_seconds):
    dev = torch.device("cuda")
    w = WORKLOADS[name]
    causal = w["causal"]
    g = torch.Generator(device=dev).manual_seed(4321)
    (fa_u, ba_u), (fb_u, bb_u), plan_u = packed_and_loop(w["uniform"], causal, g)
    (fa_s, ba_s), (fb_s, bb_s), plan_s = packed_and_loop(w["skewed"], causal, g)
    lq, lk = w["uniform"][0]
    B, n = len(w["uniform"]), max(lq, lk)
    mk = lambda rows, sc: ((torch.rand(B, H, rows, D, device=dev, generator=g) - 0.5) * sc).bfloat16()
    q, k, v, go = mk(lq, 1.0), mk(lk, 1.0), mk(lk, 1.0), mk(lq, 0.4)
    fc, bc = dense_calls(q, k, v, go, causal)
    # p: the square of max(len_q, len_k) rows per sequence; zero rows in front of the chunk (prefill) or behind the keys (cross)
    pad_front = lambda t: torch.cat([torch.zeros(B, H, n - t.shape[2], D, dtype=t.dtype, device=dev), t], dim=2).contiguous()
    pad_back = lambda t: torch.cat([t, torch.zeros(B, H, n - t.shape[2], D, dtype=t.dtype, device=dev)], dim=2).contiguous()
    fp, bp = dense_calls(pad_front(q), pad_back(k), pad_back(v), pad_front(go), causal, square=True)
    fwd_calls = {"a": fa_u, "b": fb_u, "b2": fb_u, "c": fc, "p": fp, "a'": fa_s, "b'": fb_s, "b2'": fb_s}
    two = lambda b: (lambda: (b(1), b(6)))
    bwd_calls = {"a": ba_u, "b": bb_u, "b2": bb_u, "c": two(bc), "p": two(bp), "a'": ba_s, "b'": bb_s, "b2'": bb_s}
    for f in fwd_calls.values():       # O, L of every variant exist before a backward is timed
        f()
    tf = time_variants(fwd_calls, min_launches, min_seconds)
    tb = time_variants(bwd_calls, min_launches, min_seconds)
    torch.cuda.synchronize()
    ms = lambda t: {k_: round(v_[0], 4) for k_, v_ in t.items()}
    f, b = ms(tf), ms(tb)
    res = {"workload": name, "causal": causal, "heads": H, "head_dim": D,
           "uniform": list(map(list, w["uniform"])), "skewed": list(map(list, w["skewed"])), "dense_c": [B, H, lq, lk, D], "square_p": [B, H, n, D],
           "items": {"uniform": [int(plan_u.row_items.shape[0]), int(plan_u.key_items.shape[0])],
                     "skewed": [int(plan_s.row_items.shape[0]), int(plan_s.key_items.shape[0])]},
           "forward_ms": f, "backward_ms": b,
           "launches": {"forward": {k_: v_[1] for k_, v_ in tf.items()}, "backward": {k_: v_[1] for k_, v_ in tb.items()}},
           "timed_seconds": {"forward": {k_: round(v_[2], 2) for k_, v_ in tf.items()}, "backward": {k_: round(v_[2], 2) for k_, v_ in tb.items()}}}
    for side, t in (("forward", f), ("backward", b)):
        res[f"{side}_spread_ms"] = round(abs(t["b"] - t["b2"]), 4)
        res[f"{side}_spread_skewed_ms"] = round(abs(t["b'"] - t["b2'"]), 4)
        res[f"{side}_a_over_b"] = round(t["a"] / t["b"], 4)
        res[f"{side}_a_over_b_skewed"] = round(t["a'"] / t["b'"], 4)
        res[f"{side}_a_over_c"] = round(t["a"] / t["c"], 4)
        res[f"{side}_c_over_p"] = round(t["c"] / t["p"], 4)
        res[f"expect_{side}_a_le_b"] = t["a"] <= t["b"]
        res[f"expect_{side}_a_le_b_skewed"] = t["a'"] <= t["b'"]
        res[f"expect_{side}_c_le_p"] = t["c"] <= t["p"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "qk_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms)",
           "cases": []}
    for name in WORKLOADS:
        r = one_workload(name, a.min_launches, a.min_seconds)
        res["cases"].append(r)
        verdicts = {k: v for k, v in r.items() if k.startswith("expect_")}
        print(f"{name}: fwd {r['forward_ms']} | bwd {r['backward_ms']} | {verdicts}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
