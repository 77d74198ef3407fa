"""Split-KV decode attention against the only way the library had before it and against a copy of the bytes it must read, timed
in ONE process on one device (dev aid; bench.py is untouched; the method of tools/gpu_qk_time.py).

    python tools/gpu_decode_time.py [--out profiles/decode_times.json] [--min-launches 40] [--min-seconds 0.25]

d = 128, N_q = 1 (one line with N_q = 4), (H_q, H_kv) in {(64, 8), (32, 8), (16, 16)}, (B, len) in {(1, 4096), (1, 32768), (1, 131072),
(8, 8192), (64, 2048)}; every sequence at the full length of its cache (seqlens_k is passed, holding N_cap), so that arm b can run.
    a, a2   flash_attention_2_decode with n_splits = 0 (the default rule), caller workspace
    b, b2   flash_attention_2_qk_forward on the same tensors: one workgroup per query head, 256-row tiles for N_q rows
    c, c2   a device-to-device copy of exactly the K and V bytes the call must read (two copy_ calls): the bandwidth yardstick
Every arm is timed twice; |x - x2| is the spread of the method, per arm and shape, and goes into the file.
    sweep   at three shapes, the decode call with n_splits = 1, 2, 4, ... up to 256 (twice each): what the default rule rests on
Variants alternate in blocks of a few launches (order reversed every other round) after a warm-up; every variant gets at least
--min-launches timed launches and --min-seconds of timed work; medians of the per-launch block times are reported.  Nothing is
fixed in advance: the medians and the verdicts go into the JSON, whatever they are."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402

D = 128
HEADS = ((64, 8), (32, 8), (16, 16))
BATCHES = ((1, 4096), (1, 32768), (1, 131072), (8, 8192), (64, 2048))
SHAPES = [(hq, hkv, 1, B, n) for hq, hkv in HEADS for B, n in BATCHES] + [(64, 8, 4, 8, 8192)]
SWEEPS = [(64, 8, 1, 1, 4096), (64, 8, 1, 1, 32768), (64, 8, 1, 8, 8192)]
BLOCK = 5          # launches between two events


def time_variants(calls, min_launches, min_seconds):
    """calls: name -> callable.  Returns name -> median ms per launch."""
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
    return {n: statistics.median(blocks[n]) for n in names}


def tensors(hq, hkv, nq, B, n, g):
    dev = torch.device("cuda")
    mk = lambda h, rows: (torch.rand(B, h, rows, D, device=dev, generator=g) - 0.5).bfloat16()
    Q, K, V = mk(hq, nq), mk(hkv, n), mk(hkv, n)
    return Q, K, V, torch.full((B,), n, dtype=torch.int32, device=dev)


def decode_call(Q, K, V, lens, n_splits):
    B, hq, nq, _ = Q.shape
    hkv, n = K.shape[1], K.shape[2]
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device=Q.device)
    ws = fa.decode_workspace(B, hq, hkv, nq, n, D, n_splits, device=Q.device)
    s = 1.0 / D ** 0.5
    return lambda: fa.flash_attention_2_decode(Q, K, V, lens, s, causal=True, n_splits=n_splits, O=O, L=L, workspace=ws)


def one_shape(shape, min_launches, min_seconds, g):
    hq, hkv, nq, B, n = shape
    Q, K, V, lens = tensors(hq, hkv, nq, B, n, g)
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device=Q.device)
    Kc, Vc = torch.empty_like(K), torch.empty_like(V)
    s = 1.0 / D ** 0.5
    a = decode_call(Q, K, V, lens, 0)
    b = lambda: fa.flash_attention_2_qk_forward(Q, K, V, s, causal=True, O=O, L=L)
    c = lambda: (Kc.copy_(K), Vc.copy_(V))
    t = time_variants({"a": a, "b": b, "c": c, "a2": a, "b2": b, "c2": c}, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b", "c")}
    kv_bytes = 2 * K.numel() * 2
    res = {"H_q": hq, "H_kv": hkv, "N_q": nq, "B": B, "len": n, "head_dim": D, "n_splits": fa.decode_num_splits(B, hkv, n, D),
           "ms": ms, "spread_ms": spread, "kv_bytes": kv_bytes, "a_kv_TBps": round(kv_bytes / (t["a"] * 1e-3) / 1e12, 3),
           "a_over_b": round(t["a"] / t["b"], 4), "a_over_c": round(t["a"] / t["c"], 4)}
    if B * hq <= 256:      # the requirement: faster than the parent's only way by more than the spread of the method
        res["expect_a_faster_than_b_beyond_spread"] = bool(max(t["a"], t["a2"]) + max(spread.values()) < min(t["b"], t["b2"]))
    return res


def one_sweep(shape, min_launches, min_seconds, g):
    hq, hkv, nq, B, n = shape
    Q, K, V, lens = tensors(hq, hkv, nq, B, n, g)
    counts = [c for c in (1, 2, 4, 8, 16, 32, 64, 128, 256) if c * 128 <= n]
    calls = {}
    for c in counts:
        calls[f"{c}"] = decode_call(Q, K, V, lens, c)
    for c in counts:
        calls[f"{c}'"] = calls[f"{c}"]
    t = time_variants(calls, min_launches, min_seconds)
    return {"H_q": hq, "H_kv": hkv, "N_q": nq, "B": B, "len": n, "head_dim": D, "default_n_splits": fa.decode_num_splits(B, hkv, n, D),
            "ms_by_n_splits": {str(c): round(t[f"{c}"], 5) for c in counts},
            "spread_ms_by_n_splits": {str(c): round(abs(t[f"{c}"] - t[f"{c}'"]), 5) for c in counts}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decode_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(2468)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "flash_attention_2_decode, n_splits = 0", "b": "flash_attention_2_qk_forward on the same tensors",
                    "c": "device-to-device copy of the K and V bytes"},
           "cases": [], "sweeps": []}
    for shape in SHAPES:
        r = one_shape(shape, a.min_launches, a.min_seconds, g)
        res["cases"].append(r)
        print(json.dumps(r), flush=True)
    for shape in SWEEPS:
        r = one_sweep(shape, a.min_launches, a.min_seconds, g)
        res["sweeps"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
