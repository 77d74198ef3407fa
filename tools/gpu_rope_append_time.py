"""The rotary-embedding KV-cache append (rope_kv_cache_append, rope_kv_cache_append_paged) against the framework path it replaces
and against the plain append, timed in ONE process on one device (dev aid; bench.py is untouched; the method of
tools/gpu_kv_append_time.py and tools/gpu_decode_time.py).

    python tools/gpu_rope_append_time.py [--out profiles/rope_append_times.json] [--min-launches 40] [--min-seconds 0.25]

(B, n_new): the decode steps (1, 1), (64, 1), (64, 4) and the prompt chunks (1, 8192), (8, 8192); H_q = 64, H_kv = 8, d = 128,
rot_dim = d, the rotate-half form, real cos/sin tables (base 10000); all four cache kinds: contiguous and paged (pages of 64 keys
assigned by a seeded permutation), bf16 and e4m3 with per-head descales.  The capacity is max(4096, 2 n_new) and every
sequence's new tokens fill the rows just below 3/4 of it.  The source is one fused [B, n_new, H_q + 2 H_kv, d] projection output
whose Q, K and V slices are passed as views.
    a, a2   this call: one launch for Q, K and V
    b, b2   what it replaces today, on the same views: positions from the device lengths, a cos/sin gather, the rotation of K
            and of Q in torch with the contract's expression (fp32 products and sums, one op each, then .bfloat16()),
            .contiguous() on Q, K and V (the append takes K_new and V_new under ONE stride triple, so a contiguous rotated K
            needs a contiguous V), then kv_cache_append / kv_cache_append_paged; no host synchronisation in it either
    c, c2   kv_cache_append / kv_cache_append_paged alone on the unrotated views: the floor -- the same K/V bytes, no Q, no rotation
Every arm is timed twice; |x - x2| is the spread of the method.  Nothing is fixed in advance: the medians and the verdicts go
into the JSON, whatever they are.  `faster_than_framework_beyond_spread`: max(a, a2) + the larger spread of a and b < min(b, b2).
At the chunk shapes the bytes the call must move per second are recorded too."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

SHAPES = [(1, 1), (64, 1), (64, 4), (1, 8192), (8, 8192)]
KINDS = [("contiguous", "bf16"), ("contiguous", "e4m3"), ("paged", "bf16"), ("paged", "e4m3")]
HQ, HKV, D, PAGE = 64, 8, 128, 64
CHUNK = 1024      # n_new from which a shape counts as a prompt chunk
E4M3 = torch.float8_e4m3fn


def framework_rope_append(q, kn, vn, K, V, cos, sin, lens, table, kd, vd):
    """The path a caller writes today: everything the fused call does, in framework ops, ending in the existing append."""
    B, _, n_new, d = kn.shape
    half = cos.shape[1]
    steps = torch.arange(n_new, device=kn.device)
    out = {}

    def dense(x):      # .contiguous(); a size-1 dimension keeps any stride through it, and the append compares strides
        x = x.contiguous()
        return x if x.stride() == torch.empty(0).new_empty(x.shape).stride() else x.clone(memory_format=torch.contiguous_format)

    def rotate(x, c, s):
        xf = x.float()
        x1, x2 = xf[..., :half], xf[..., half:2 * half]
        return dense(torch.cat([x1 * c - x2 * s, x2 * c + x1 * s, xf[..., 2 * half:]], dim=-1).bfloat16())

    def call():
        pos = lens.long()[:, None] - n_new + steps[None, :]
        c, s = cos[pos][:, None], sin[pos][:, None]
        out["Q"] = rotate(q, c, s)
        k_rot, v = rotate(kn, c, s), dense(vn)
        if table is None:
            fa.kv_cache_append(k_rot, v, K, V, lens, kd, vd)
        else:
            fa.kv_cache_append_paged(k_rot, v, K, V, table, lens, kd, vd)
    return call, out


def one_case(shape, kind, min_launches, min_seconds, g):
    B, n_new = shape
    layout, cache_dtype = kind
    dev = torch.device("cuda")
    cap = max(4096, 2 * n_new)
    fused = (torch.rand(B, n_new, HQ + 2 * HKV, D, device=dev, generator=g) - 0.5).bfloat16()
    q, kn, vn = (t.permute(0, 2, 1, 3) for t in (fused[:, :, :HQ], fused[:, :, HQ:HQ + HKV], fused[:, :, HQ + HKV:]))
    lens = torch.full((B,), cap * 3 // 4, dtype=torch.int32, device=dev)
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(cap, dtype=torch.float64)[:, None] * inv[None, :]
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    fp8 = cache_dtype == "e4m3"
    dtype = E4M3 if fp8 else torch.bfloat16
    table = None
    if layout == "paged":
        n_pages = B * cap // PAGE
        table = torch.randperm(n_pages, device=dev, generator=g).view(B, cap // PAGE).int().contiguous()
        cache_shape = (n_pages, HKV, PAGE, D)
    else:
        cache_shape = (B, HKV, cap, D)
    mk = lambda: torch.zeros(cache_shape, dtype=torch.uint8 if fp8 else dtype, device=dev).view(dtype)
    Ka, Va, Kb, Vb, Kc, Vc = mk(), mk(), mk(), mk(), mk(), mk()
    kd = torch.tensor([0.004 + 0.0005 * h for h in range(HKV)], device=dev) if fp8 else None
    vd = torch.tensor([0.006 - 0.0003 * h for h in range(HKV)], device=dev) if fp8 else None
    Qa = torch.empty(B, HQ, n_new, D, dtype=torch.bfloat16, device=dev)
    if table is None:
        a = lambda: fa.rope_kv_cache_append(q, kn, vn, Ka, Va, cos, sin, lens, k_descale=kd, v_descale=vd, Q_out=Qa)
        c = lambda: fa.kv_cache_append(kn, vn, Kc, Vc, lens, kd, vd)
    else:
        a = lambda: fa.rope_kv_cache_append_paged(q, kn, vn, Ka, Va, table, cos, sin, lens, k_descale=kd, v_descale=vd, Q_out=Qa)
        c = lambda: fa.kv_cache_append_paged(kn, vn, Kc, Vc, table, lens, kd, vd)
    b, b_out = framework_rope_append(q, kn, vn, Kb, Vb, cos, sin, lens, table, kd, vd)
    a(), b()
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in ((Ka, Kb), (Va, Vb))) and \
        torch.equal(Qa.view(torch.int16), b_out["Q"].view(torch.int16))
    t = time_variants({"a": a, "b": b, "c": c, "a2": a, "b2": b, "c2": c}, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b", "c")}
    read = B * (HQ + 2 * HKV) * n_new * D * 2 + 2 * B * n_new * (D // 2) * 4      # the three sources; a table row pair per (sequence, token)
    written = B * HQ * n_new * D * 2 + 2 * B * HKV * n_new * D * (1 if fp8 else 2)
    res = {"B": B, "H_q": HQ, "H_kv": HKV, "n_new": n_new, "head_dim": D, "rot_dim": D, "layout": layout, "cache": cache_dtype,
           "kv_capacity": cap, "page_size": PAGE if table is not None else None, "ms": ms, "spread_ms": spread,
           "bytes_read": read, "bytes_written": written,
           "a_over_b": round(t["a"] / t["b"], 4), "a_over_c": round(t["a"] / t["c"], 4),
           "same_bytes_as_framework": bool(same),
           "faster_than_framework_beyond_spread": bool(max(t["a"], t["a2"]) + max(spread["a"], spread["b"]) < min(t["b"], t["b2"]))}
    if n_new >= CHUNK:
        res["a_TBps"] = round((read + written) / (t["a"] * 1e-3) / 1e12, 3)
    del b_out["Q"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rope_append_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1357)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "rope_kv_cache_append / rope_kv_cache_append_paged: one launch for Q, K and V",
                    "b": "the framework path: positions from the device lengths, cos/sin gather, fp32 rotation of K and Q in torch, "
                         ".contiguous() on Q, K and V, then kv_cache_append / kv_cache_append_paged",
                    "c": "kv_cache_append / kv_cache_append_paged alone: the same K/V bytes, no Q, no rotation"},
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
