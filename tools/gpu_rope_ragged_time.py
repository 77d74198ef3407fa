"""The ragged rotary-embedding KV-cache append (rope_kv_cache_append_ragged_paged) against the only device route there was before
it -- one uniform rope_kv_cache_append_paged per sequence -- and, at a uniform q_b, against the single uniform call; timed in ONE
process on one device (dev aid; bench.py is untouched; the method of tools/gpu_rope_append_time.py and tools/gpu_decode_time.py).

    python tools/gpu_rope_ragged_time.py [--out profiles/rope_ragged_times.json] [--min-launches 40] [--min-seconds 0.25]

H_q = 64, H_kv = 8, d = 128, rot_dim = d, the rotate-half form, real cos/sin tables (base 10000); paged caches (pages of 64 keys
assigned by a seeded permutation), bf16 and e4m3 with per-head descales.  The capacity is max(4096, 2 max q_b) and every
sequence's new tokens fill the rows just below 3/4 of it.  The source is one fused [T, H_q + 2 H_kv, d] projection output whose
Q, K and V slices are passed as views.  Workloads:
    decode_mix    64 sequences: 56 with q = 1, 8 with q = 8 (every eighth), T = 120
    chunk_mix     64 sequences: one 2048-token prompt chunk among 63 decodes, T = 2111
    chunk         one sequence, q = 8192
    uniform4      64 sequences with q = 4 each, T = 256: a uniform mix small enough that per-launch overhead shows
Arms:
    a, a2   this call, driven by a plan built ONCE outside the timed region (a step builds it once for all layers)
    b, b2   one uniform rope_kv_cache_append_paged per non-empty sequence on [1, H, q_b, d] views of the same tokens, with the
            slices of the table and of the lengths made outside the timed region: B launches, and a host that knows cu
    c, c2   (uniform q_b only) the single uniform rope_kv_cache_append_paged on [B, H, q, d] views of the same tokens
Every arm is timed twice; |x - x2| is the spread of the method.  Nothing is fixed in advance: the medians, the ratios and the
achieved bytes per second go into the JSON, whatever they are."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

HQ, HKV, D, PAGE = 64, 8, 128, 64
E4M3 = torch.float8_e4m3fn
WORKLOADS = [
    ("decode_mix", [8 if b % 8 == 7 else 1 for b in range(64)]),
    ("chunk_mix", [2048 if b == 31 else 1 for b in range(64)]),
    ("chunk", [8192]),
    ("uniform4", [4] * 64),
]


def one_case(name, qs, cache_dtype, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    B, T = len(qs), sum(qs)
    cap = max(4096, 2 * max(qs))
    cu = [0]
    for q in qs:
        cu.append(cu[-1] + q)
    fused = (torch.rand(T, HQ + 2 * HKV, D, device=dev, generator=g) - 0.5).bfloat16()
    q, kn, vn = fused[:, :HQ], fused[:, HQ:HQ + HKV], fused[:, HQ + HKV:]
    lens = torch.full((B,), cap * 3 // 4, dtype=torch.int32, device=dev)
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(cap, dtype=torch.float64)[:, None] * inv[None, :]
    cos, sin = ang.cos().float().to(dev), ang.sin().float().to(dev)
    fp8 = cache_dtype == "e4m3"
    dtype = E4M3 if fp8 else torch.bfloat16
    n_pages = B * cap // PAGE
    table = torch.randperm(n_pages, device=dev, generator=g).view(B, cap // PAGE).int().contiguous()
    mk = lambda: torch.zeros((n_pages, HKV, PAGE, D), dtype=torch.uint8 if fp8 else dtype, device=dev).view(dtype)
    Ka, Va, Kb, Vb, Kc, Vc = mk(), mk(), mk(), mk(), mk(), mk()
    kd = torch.tensor([0.004 + 0.0005 * h for h in range(HKV)], device=dev) if fp8 else None
    vd = torch.tensor([0.006 - 0.0003 * h for h in range(HKV)], device=dev) if fp8 else None
    kw = dict(k_descale=kd, v_descale=vd)
    plan = fa.extend_ragged_plan(torch.tensor(cu, dtype=torch.int32, device=dev), HQ, HKV, T)
    Qa = torch.empty(T, HQ, D, dtype=torch.bfloat16, device=dev)
    a = lambda: fa.rope_kv_cache_append_ragged_paged(q, kn, vn, Ka, Va, table, cos, sin, plan, lens, Q_out=Qa, **kw)
    # (b) the views, table rows, lengths and outputs of every sequence, made once
    one = lambda t, s, n: t[s:s + n].permute(1, 0, 2)[None]
    per = [(one(q, cu[b], qs[b]), one(kn, cu[b], qs[b]), one(vn, cu[b], qs[b]), table[b:b + 1].contiguous(), lens[b:b + 1].contiguous(),
            torch.empty(1, HQ, qs[b], D, dtype=torch.bfloat16, device=dev)) for b in range(B) if qs[b]]

    def b_route():
        for qb, kb, vb, tb, lb, ob in per:
            fa.rope_kv_cache_append_paged(qb, kb, vb, Kb, Vb, tb, cos, sin, lb, Q_out=ob, **kw)

    calls = {"a": a, "b": b_route}
    uniform = len(set(qs)) == 1
    if uniform:
        n = qs[0]
        u = lambda t: t.view(B, n, -1, D).permute(0, 2, 1, 3)
        Qc = torch.empty(B, HQ, n, D, dtype=torch.bfloat16, device=dev)
        calls["c"] = lambda: fa.rope_kv_cache_append_paged(u(q), u(kn), u(vn), Kc, Vc, table, cos, sin, lens, Q_out=Qc, **kw)
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in ((Ka, Kb), (Va, Vb))) and \
        all(torch.equal(ob[0].permute(1, 0, 2), Qa[cu[b]:cu[b] + qs[b]]) for b, (*_, ob) in zip([b for b in range(B) if qs[b]], per))
    if uniform:
        same = same and torch.equal(Ka.view(torch.uint8), Kc.view(torch.uint8)) and torch.equal(Qc.permute(0, 2, 1, 3).reshape(T, HQ, D), Qa)
    calls.update({k + "2": v for k, v in list(calls.items())})
    t = time_variants(calls, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    arms = [k for k in ("a", "b", "c") if k in t]
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in arms}
    read = T * (HQ + 2 * HKV) * D * 2 + (HQ + HKV) * 2 * T * (D // 2) * 4      # the three sources; a table row pair per (head, token)
    written = T * HQ * D * 2 + 2 * T * HKV * D * (1 if fp8 else 2)
    res = {"workload": name, "B": B, "total_q": T, "launches_b": len(per), "H_q": HQ, "H_kv": HKV, "head_dim": D, "rot_dim": D,
           "cache": cache_dtype, "kv_capacity": cap, "page_size": PAGE, "ms": ms, "spread_ms": spread,
           "bytes_read": read, "bytes_written": written, "a_over_b": round(t["a"] / t["b"], 4),
           "a_TBps": round((read + written) / (t["a"] * 1e-3) / 1e12, 4), "same_bytes_as_per_sequence_route": bool(same)}
    if uniform:
        res["a_over_c"] = round(t["a"] / t["c"], 4)
        res["c_TBps"] = round((read + written) / (t["c"] * 1e-3) / 1e12, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rope_ragged_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(2468)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "rope_kv_cache_append_ragged_paged with a prebuilt plan: one launch for the packed Q, K and V",
                    "b": "one uniform rope_kv_cache_append_paged per non-empty sequence (B = 1, n_new = q_b) on views of the same tokens",
                    "c": "uniform q_b only: the single uniform rope_kv_cache_append_paged"},
           "cases": []}
    for name, qs in WORKLOADS:
        for cache in ("bf16", "e4m3"):
            r = one_case(name, qs, cache, a.min_launches, a.min_seconds, g)
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
