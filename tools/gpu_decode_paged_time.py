"""Paged decode attention against the contiguous kernel and against what a caller with a page pool had to do before it -- gather
the pages into a contiguous cache, then decode -- timed in ONE process on one device (dev aid; bench.py is untouched; the method
of tools/gpu_decode_time.py, whose time_variants this uses).

    python tools/gpu_decode_paged_time.py [--out profiles/decode_paged_times.json] [--min-launches 40] [--min-seconds 0.25]

d = 128, N_q = 1, (H_q, H_kv) = (64, 8), (B, len) in {(1, 4096), (1, 32768), (8, 8192), (64, 2048)}, page sizes 32, 128, 256; every
sequence at the full length of its pages (seqlens_k is passed, holding the capacity).
    a, a2     flash_attention_2_decode_paged, identity table (sequence b's pages are b max_pages ..+max_pages, in order)
    a', a'2   flash_attention_2_decode_paged, a shuffled table over the same pool
    b, b2     flash_attention_2_decode on the gathered contiguous cache
    g, g2     index_select of the pages through the shuffled table into a preallocated contiguous cache (K and V), then b: what
              a caller with a page pool had to do for every step (the permute back to [B, H_kv, N, d] is part of the gather)
All with n_splits = 0 and a caller workspace.  Every arm is timed twice; |x - x2| is the spread of the method, per arm and shape.
CONDITION: a and a' faster than g beyond the spread at every shape and page size (g moves the K/V bytes three times).
REPORTED: a / b and a' / b; a ratio above 1 by more than twice the larger spread of its two arms is flagged `explain`.  Nothing
is fixed in advance: the medians and the verdicts go into the JSON, whatever they are."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_decode_time import time_variants, BLOCK  # noqa: E402  (puts the repository root on sys.path)
import cuda_flashattention_amd as fa  # noqa: E402

D = 128
HQ, HKV, NQ = 64, 8, 1
BATCHES = ((1, 4096), (1, 32768), (8, 8192), (64, 2048))
PAGE_SIZES = (32, 128, 256)


def one_shape(B, n, P, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    max_pages = n // P
    n_pages = B * max_pages
    mk = lambda *s: (torch.rand(*s, device=dev, generator=g) - 0.5).bfloat16()
    Q, Kp, Vp = mk(B, HQ, NQ, D), mk(n_pages, HKV, P, D), mk(n_pages, HKV, P, D)
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    ident = torch.arange(n_pages, dtype=torch.int32, device=dev).view(B, max_pages)
    shuf = torch.randperm(n_pages, device=dev, generator=g).to(torch.int32).view(B, max_pages)
    flat = shuf.view(-1).long()
    # the contiguous cache of the shuffled table: [B, max_pages, hkv, P, d] -> [B, hkv, max_pages P, d]
    gathered = lambda pool, out: torch.index_select(pool, 0, flat, out=out)
    stage_k, stage_v = torch.empty_like(Kp), torch.empty_like(Vp)
    Kc, Vc = torch.empty(B, HKV, n, D, dtype=torch.bfloat16, device=dev), torch.empty(B, HKV, n, D, dtype=torch.bfloat16, device=dev)

    def gather():
        for pool, stage, out in ((Kp, stage_k, Kc), (Vp, stage_v, Vc)):
            gathered(pool, stage)
            out.view(B, HKV, max_pages, P, D).copy_(stage.view(B, max_pages, HKV, P, D).permute(0, 2, 1, 3, 4))

    gather()
    s = 1.0 / D ** 0.5
    ws = fa.decode_workspace(B, HQ, HKV, NQ, n, D, 0, device=dev)
    outs = [(torch.empty_like(Q), torch.empty(B, HQ, NQ, dtype=torch.float32, device=dev)) for _ in range(3)]
    paged = lambda table, o: (lambda: fa.flash_attention_2_decode_paged(Q, Kp, Vp, table, lens, s, causal=True, n_splits=0, O=o[0], L=o[1],
                                                                      workspace=ws))
    a, a1 = paged(ident, outs[0]), paged(shuf, outs[1])
    b = lambda: fa.flash_attention_2_decode(Q, Kc, Vc, lens, s, causal=True, n_splits=0, O=outs[2][0], L=outs[2][1], workspace=ws)
    gb = lambda: (gather(), b())
    a1(), b()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[1][0].view(torch.int16), outs[2][0].view(torch.int16))
                and torch.equal(outs[1][1].view(torch.int32), outs[2][1].view(torch.int32)))
    t = time_variants({"a": a, "a'": a1, "b": b, "g": gb, "a2": a, "a'2": a1, "b2": b, "g2": gb}, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "a'", "b", "g")}
    kv_bytes = 2 * Kp.numel() * 2
    res = {"H_q": HQ, "H_kv": HKV, "N_q": NQ, "B": B, "len": n, "head_dim": D, "page_size": P, "n_splits": fa.decode_num_splits(B, HKV, n, D),
           "ms": ms, "spread_ms": spread, "kv_bytes": kv_bytes, "a_kv_TBps": round(kv_bytes / (t["a"] * 1e-3) / 1e12, 3),
           "shuffled_equals_contiguous_bits": same}
    for k in ("a", "a'"):
        res[f"{k}_over_b"] = round(t[k] / t["b"], 4)
        res[f"{k}_over_b_explain"] = bool(t[k] - t["b"] > 2 * max(spread[k], spread["b"]))
        res[f"{k}_faster_than_g_beyond_spread"] = bool(max(t[k], t[k + "2"]) + max(spread.values()) < min(t["g"], t["g2"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decode_paged_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1357)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "flash_attention_2_decode_paged, identity table", "a'": "flash_attention_2_decode_paged, shuffled table",
                    "b": "flash_attention_2_decode on the gathered contiguous cache",
                    "g": "index_select of the pages + permute into a contiguous cache, then b"},
           "cases": []}
    for B, n in BATCHES:
        for P in PAGE_SIZES:
            r = one_shape(B, n, P, a.min_launches, a.min_seconds, g)
            res["cases"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
