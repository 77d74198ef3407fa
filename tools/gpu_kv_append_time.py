"""The KV-cache append (kv_cache_append, kv_cache_append_paged) against the framework path it replaces and against a copy of the
bytes it writes, timed in ONE process on one device (dev aid; bench.py is untouched; the method of tools/gpu_decode_time.py).

    python tools/gpu_kv_append_time.py [--out profiles/kv_append_times.json] [--min-launches 40] [--min-seconds 0.25]

(B, H_kv, n_new, d): the decode steps (1, 8, 1, 128), (64, 8, 1, 128), (64, 8, 4, 128) and the prompt chunks (1, 8, 8192, 128),
(8, 8, 8192, 128); all four cache kinds: contiguous and paged (pages of 64 keys assigned by a seeded permutation), bf16 and e4m3
with per-head descales.  The capacity is max(4096, 2 n_new) and every sequence's new tokens fill the rows just below
3/4 of it.  The source is the K and V slices of one fused [B, n_new, 64 + 2 H_kv, d] projection output, passed as views.
    a, a2   this call: one launch for K and V
    b, b2   the framework path it replaces, on the same views: the index computation (positions from the device lengths; pages
            and rows through the table when paged), for e4m3 (x.float() / descale).clamp(-448, 448).to(float8_e4m3fn), and two
            index_put_ scatters, one each for K and V; no host synchronisation in it either
    c, c2   a device-to-device copy of exactly the bytes the bf16 append writes (two copy_ calls of [B, H_kv, n_new, d] bf16)
Every arm is timed twice; |x - x2| is the spread of the method.  Nothing is fixed in advance: the medians and the verdicts go
into the JSON, whatever they are.  `faster_than_framework_beyond_spread`: max(a, a2) + the larger spread of a and b < min(b, b2).
At the chunk shapes a / c is recorded too."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

SHAPES = [(1, 8, 1, 128), (64, 8, 1, 128), (64, 8, 4, 128), (1, 8, 8192, 128), (8, 8, 8192, 128)]
KINDS = [("contiguous", "bf16"), ("contiguous", "e4m3"), ("paged", "bf16"), ("paged", "e4m3")]
HQ, PAGE = 64, 64
CHUNK = 1024      # n_new from which a shape counts as a prompt chunk
E4M3 = torch.float8_e4m3fn


def framework_append(kn, vn, K, V, lens, table, kd, vd):
    """The path a caller writes today, on the same views: positions from the device lengths, then one scatter per tensor."""
    B, H, n_new, d = kn.shape
    fp8 = K.dtype == E4M3
    steps = torch.arange(n_new, device=kn.device)
    batch = torch.arange(B, device=kn.device)[:, None]

    def call():
        pos = lens.long()[:, None] - n_new + steps[None, :]
        if table is None:
            first, rows = batch, pos
        else:
            first, rows = table.gather(1, pos // PAGE).long(), pos % PAGE
        for new, cache, ds in ((kn, K, kd), (vn, V, vd)):
            x = new.permute(0, 2, 1, 3)
            if fp8:
                x = (x.float() / ds[None, None, :, None]).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
                cache.view(torch.uint8)[first, :, rows] = x
            else:
                cache[first, :, rows] = x
    return call


def one_case(shape, kind, min_launches, min_seconds, g):
    B, H, n_new, d = shape
    layout, cache_dtype = kind
    dev = torch.device("cuda")
    cap = max(4096, 2 * n_new)
    fused = (torch.rand(B, n_new, HQ + 2 * H, d, device=dev, generator=g) - 0.5).bfloat16()
    kn, vn = fused[:, :, HQ:HQ + H].permute(0, 2, 1, 3), fused[:, :, HQ + H:].permute(0, 2, 1, 3)
    lens = torch.full((B,), cap * 3 // 4, dtype=torch.int32, device=dev)
    fp8 = cache_dtype == "e4m3"
    dtype = E4M3 if fp8 else torch.bfloat16
    table = None
    if layout == "paged":
        n_pages = B * cap // PAGE
        table = torch.randperm(n_pages, device=dev, generator=g).view(B, cap // PAGE).int().contiguous()
        cache_shape = (n_pages, H, PAGE, d)
    else:
        cache_shape = (B, H, cap, d)
    mk = lambda: torch.zeros(cache_shape, dtype=torch.uint8 if fp8 else dtype, device=dev).view(dtype)
    Ka, Va, Kb, Vb = mk(), mk(), mk(), mk()
    kd = torch.tensor([0.004 + 0.0005 * h for h in range(H)], device=dev) if fp8 else None
    vd = torch.tensor([0.006 - 0.0003 * h for h in range(H)], device=dev) if fp8 else None
    if table is None:
        a = lambda: fa.kv_cache_append(kn, vn, Ka, Va, lens, kd, vd)
    else:
        a = lambda: fa.kv_cache_append_paged(kn, vn, Ka, Va, table, lens, kd, vd)
    b = framework_append(kn, vn, Kb, Vb, lens, table, kd, vd)
    src = [torch.empty(B, H, n_new, d, dtype=torch.bfloat16, device=dev).copy_(t) for t in (kn, vn)]
    dst = [torch.empty_like(t) for t in src]
    c = lambda: (dst[0].copy_(src[0]), dst[1].copy_(src[1]))
    a(), b()
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in ((Ka, Kb), (Va, Vb)))
    t = time_variants({"a": a, "b": b, "c": c, "a2": a, "b2": b, "c2": c}, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b", "c")}
    written = 2 * B * H * n_new * d * (1 if fp8 else 2)
    read = 2 * B * H * n_new * d * 2
    res = {"B": B, "H_kv": H, "n_new": n_new, "head_dim": d, "layout": layout, "cache": cache_dtype, "kv_capacity": cap,
           "page_size": PAGE if table is not None else None, "ms": ms, "spread_ms": spread, "bytes_read": read, "bytes_written": written,
           "a_TBps": round((read + written) / (t["a"] * 1e-3) / 1e12, 3), "a_over_b": round(t["a"] / t["b"], 4),
           "same_bytes_as_framework": bool(same),
           "faster_than_framework_beyond_spread": bool(max(t["a"], t["a2"]) + max(spread["a"], spread["b"]) < min(t["b"], t["b2"]))}
    if n_new >= CHUNK:
        res["a_over_c"] = round(t["a"] / t["c"], 4)
        if not fp8:
            res["slower_than_copy_beyond_spread"] = bool(min(t["a"], t["a2"]) > max(t["c"], t["c2"]) + max(spread["a"], spread["c"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kv_append_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(2468)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "kv_cache_append / kv_cache_append_paged: one launch for K and V",
                    "b": "the framework path: index computation (through the table when paged), for e4m3 divide, clamp and cast, "
                         "two index_put_ scatters",
                    "c": "device-to-device copy of the bytes the bf16 append writes (two copy_ calls)"},
           "cases": []}
    for shape in SHAPES:
        for kind in KINDS:
            r = one_case(shape, kind, a.min_launches, a.min_seconds, g)
            res["cases"].append(r)
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
