"""The sparse MLA decode against the dense decode at equal bytes and against select-then-decode, timed in ONE process on one
device (dev aid; bench.py is untouched; the method of tools/gpu_decode_time.py, whose time_variants this uses).

    python tools/gpu_mla_sparse_time.py [--out profiles/mla_sparse_times.json] [--min-launches 40] [--min-seconds 0.25]

H in {16, 128}, N_q = 1, topk = 2048, (B, len) in {(1, 32768), (32, 8192)}; every sequence at the full length of its cache.
    a, a2   flash_attention_2_mla_decode_sparse, random sorted indices (topk distinct positions of [0, len)), n_splits = 0
    i, i2   the same call with identity indices arange(topk)
    d, d2   flash_attention_2_mla_decode over a cache of exactly topk rows: the same bytes streamed in order (what a gather could
            approach)
    s, s2   index_select of the topk rows into that cache, then d: what a user does without the sparse call (what it must beat)
Every arm is timed twice; |x - x2| is the spread of the method, per arm and shape, and goes into the file.  Nothing is fixed in
advance: the medians go into the JSON, whatever they are, with the largest |O_a - O_s| of the shape beside them."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

TOPK = 2048
SHAPES = [(H, B, n) for H in (16, 128) for B, n in ((1, 32768), (32, 8192))]
SCALE = 0.1147      # DeepSeek-V3's: (128 + 64) ** -0.5 times its YaRN factor squared


def one_shape(H, B, n, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    Q = ((torch.rand(B, H, 1, 576, device=dev, generator=g) - 0.5) * 8).bfloat16()
    C = (torch.rand(B, n, 576, device=dev, generator=g) - 0.5).bfloat16()
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    rand = torch.rand(B, n, device=dev, generator=g).argsort(dim=1)[:, :TOPK].sort(dim=1).values.to(torch.int32).view(B, 1, TOPK).contiguous()
    ident = torch.arange(TOPK, dtype=torch.int32, device=dev).repeat(B, 1, 1)
    O, L = torch.empty(B, H, 1, 512, dtype=torch.bfloat16, device=dev), torch.empty(B, H, 1, dtype=torch.float32, device=dev)
    Od, Ld = torch.empty_like(O), torch.empty_like(L)
    ws, wsd = fa.mla_sparse_workspace(B, H, 1, TOPK, 0, device=dev), fa.mla_decode_workspace(B, H, 1, TOPK, 0, device=dev)
    Cd, lens_d = C[:, :TOPK].clone(), torch.full((B,), TOPK, dtype=torch.int32, device=dev)
    flat, rows = C.view(B * n, 576), (rand.view(B, TOPK).long() + torch.arange(B, device=dev)[:, None] * n).view(-1)
    sparse = lambda idx: fa.flash_attention_2_mla_decode_sparse(Q, C, idx, lens, softmax_scale=SCALE, n_splits=0, O=O, L=L, workspace=ws)
    dense = lambda: fa.flash_attention_2_mla_decode(Q, Cd, lens_d, softmax_scale=SCALE, n_splits=0, O=Od, L=Ld, workspace=wsd)

    def select():
        torch.index_select(flat, 0, rows, out=Cd.view(B * TOPK, 576))
        return dense()

    a, i = (lambda: sparse(rand)), (lambda: sparse(ident))
    t = time_variants({"a": a, "i": i, "d": dense, "s": select, "a2": a, "i2": i, "d2": dense, "s2": select}, min_launches, min_seconds)
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "i", "d", "s")}
    a(), select()
    diff = float((O.float() - Od.float()).abs().max())
    return {"H": H, "N_q": 1, "B": B, "len": n, "topk": TOPK, "n_splits": fa.mla_sparse_num_splits(B, H, 1, TOPK),
            "ms": {k: round(v, 5) for k, v in t.items()}, "spread_ms": spread, "gathered_bytes": B * TOPK * 1152,
            "a_gather_TBps": round(B * TOPK * 1152 / (t["a"] * 1e-3) / 1e12, 3), "a_over_d": round(t["a"] / t["d"], 4),
            "i_over_d": round(t["i"] / t["d"], 4), "a_over_s": round(t["a"] / t["s"], 4), "max_abs_diff_a_s": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mla_sparse_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(2048)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "flash_attention_2_mla_decode_sparse, random sorted indices, n_splits = 0", "i": "the same, identity indices",
                    "d": "flash_attention_2_mla_decode over a cache of topk rows", "s": "index_select of the rows, then d"},
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
