"""MLA decode attention against the framework route and against a copy of the bytes it must read, timed in ONE process on one
device (dev aid; bench.py is untouched; the method of tools/gpu_decode_time.py, whose time_variants this uses).

    python tools/gpu_mla_decode_time.py [--out profiles/mla_decode_times.json] [--min-launches 40] [--min-seconds 0.25]

H in {16, 128}, N_q = 1, (B, len) in {(1, 4096), (1, 32768), (8, 8192), (64, 2048)}; every sequence at the full length of its cache.
    a, a2   flash_attention_2_mla_decode with n_splits = 0 (the default rule), caller workspace, O and L
    b, b2   the framework route on the same tensors: bf16 torch.matmul, softmax, matmul against the cache's first 512 columns
    c, c2   a device-to-device copy of exactly the cache bytes the call must read: the bandwidth yardstick
Every arm is timed twice; |x - x2| is the spread of the method, per arm and shape, and goes into the file.  Nothing is fixed in
advance: the medians go into the JSON, whatever they are, with the largest |O_a - O_b| of the shape beside them."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

SHAPES = [(H, B, n) for H in (16, 128) for B, n in ((1, 4096), (1, 32768), (8, 8192), (64, 2048))]
SCALE = 0.1147      # DeepSeek-V3's: (128 + 64) ** -0.5 times its YaRN factor squared


def one_shape(H, B, n, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    Q = ((torch.rand(B, H, 1, 576, device=dev, generator=g) - 0.5) * 8).bfloat16()
    C = (torch.rand(B, n, 576, device=dev, generator=g) - 0.5).bfloat16()
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    O, L = torch.empty(B, H, 1, 512, dtype=torch.bfloat16, device=dev), torch.empty(B, H, 1, dtype=torch.float32, device=dev)
    ws = fa.mla_decode_workspace(B, H, 1, n, 0, device=dev)
    Cc, Q3, Ct, V = torch.empty_like(C), Q.view(B, H, 576), C.transpose(1, 2), C[:, :, :512]
    a = lambda: fa.flash_attention_2_mla_decode(Q, C, lens, softmax_scale=SCALE, n_splits=0, O=O, L=L, workspace=ws)
    b = lambda: torch.matmul(torch.softmax(torch.matmul(Q3, Ct) * SCALE, dim=-1), V)
    c = lambda: Cc.copy_(C)
    t = time_variants({"a": a, "b": b, "c": c, "a2": a, "b2": b, "c2": c}, min_launches, min_seconds)
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b", "c")}
    a()
    diff = float((O.view(B, H, 512).float() - b().float()).abs().max())
    return {"H": H, "N_q": 1, "B": B, "len": n, "n_splits": fa.mla_decode_num_splits(B, H, 1, n), "ms": {k: round(v, 5) for k, v in t.items()},
            "spread_ms": spread, "cache_bytes": C.numel() * 2, "a_cache_TBps": round(C.numel() * 2 / (t["a"] * 1e-3) / 1e12, 3),
            "a_over_b": round(t["a"] / t["b"], 4), "a_over_c": round(t["a"] / t["c"], 4), "max_abs_diff_a_b": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mla_decode_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(576)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "flash_attention_2_mla_decode, n_splits = 0", "b": "bf16 torch.matmul / softmax / matmul on the same tensors",
                    "c": "device-to-device copy of the cache bytes"},
           "cases": []}
    for H, B, n in SHAPES:
        r = one_shape(H, B, n, a.min_launches, a.min_seconds, g)
        res["cases"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
