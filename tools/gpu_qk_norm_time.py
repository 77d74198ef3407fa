"""The ragged rotary append with a per-head QK RMSNorm (norm_rope_kv_cache_append_ragged_paged) against the same append without a
norm and against the route a framework takes today -- two RMSNorms written in torch over the Q and K slices of the projection
output, then the existing call on the normalised copies; timed in ONE process on one device (dev aid; bench.py is untouched; the
method of tools/gpu_rope_ragged_time.py and tools/gpu_decode_time.py).

    python tools/gpu_qk_norm_time.py [--out profiles/qk_norm_times.json] [--min-launches 40] [--min-seconds 0.25]

tools/gpu_rope_ragged_time.py's shapes: H_q = 64, H_kv = 8, d = 128, rot_dim = d, the rotate-half form, real cos/sin tables (base
10000); paged caches (pages of 64 keys assigned by a seeded permutation), bf16 and e4m3 with per-head descales; the source one
fused [T, H_q + 2 H_kv, d] projection output whose Q, K and V slices are passed as views; eps = 1e-6.  Workloads:
    decode_mix    64 sequences: 56 with q = 1, 8 with q = 8 (every eighth), T = 120
    chunk_mix     64 sequences: one 2048-token prompt chunk among 63 decodes, T = 2111
    chunk         one sequence, q = 8192
Arms, all driven by a plan built ONCE outside the timed region:
    a, a2   norm_rope_kv_cache_append_ragged_paged: one launch
    b, b2   rope_kv_cache_append_ragged_paged on the raw source: the same launch without a norm (it computes something else: the
            floor of what the fused call can cost)
    c, c2   the framework route: torch_rmsnorm(Q slice, q_weight) and torch_rmsnorm(K slice, k_weight) -- x.float(), pow(2),
            mean(-1), rsqrt, the weight, one cast to bf16; each a chain of eager kernels that materialises a normalised contiguous
            copy -- then V_new.contiguous() (K_new and V_new share one stride pair, and the normalised K is contiguous) and
            rope_kv_cache_append_ragged_paged on the three copies
Every arm is timed twice; |x - x2| is the spread of the method.  Nothing is fixed in advance: the medians and the ratios a / b and
a / c go into the JSON, whatever they are.  (a) and (c) need not agree in every bit -- torch's mean sums in another order and
rsqrt is not 1 / sqrt -- so the JSON records the share of bf16 elements of Q_out on which they differ, not an equality."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402
from gpu_rope_ragged_time import D, E4M3, HKV, HQ, PAGE, WORKLOADS  # noqa: E402

EPS = 1e-6
NAMES = ("decode_mix", "chunk_mix", "chunk")


def torch_rmsnorm(x, w, eps):
    """What a framework runs today on a strided [T, H, d] slice: fp32 inside, one rounding to bf16, a contiguous result."""
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w).to(torch.bfloat16)


def one_case(name, qs, cache_dtype, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    B, T = len(qs), sum(qs)
    cap = max(4096, 2 * max(qs))
    cu = [0]
    for q in qs:
        cu.append(cu[-1] + q)
    fused = (torch.rand(T, HQ + 2 * HKV, D, device=dev, generator=g) - 0.5).bfloat16()
    q, kn, vn = fused[:, :HQ], fused[:, HQ:HQ + HKV], fused[:, HQ + HKV:]
    qw = (torch.rand(D, device=dev, generator=g) + 0.5).contiguous()
    kw_ = (torch.rand(D, device=dev, generator=g) + 0.5).contiguous()
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
    Qa, Qb, Qc = (torch.empty(T, HQ, D, dtype=torch.bfloat16, device=dev) for _ in range(3))
    a = lambda: fa.norm_rope_kv_cache_append_ragged_paged(q, kn, vn, Ka, Va, table, cos, sin, qw, kw_, EPS, plan, lens, Q_out=Qa, **kw)
    b = lambda: fa.rope_kv_cache_append_ragged_paged(q, kn, vn, Kb, Vb, table, cos, sin, plan, lens, Q_out=Qb, **kw)

    def c():
        qn, knn = torch_rmsnorm(q, qw, EPS), torch_rmsnorm(kn, kw_, EPS)
        fa.rope_kv_cache_append_ragged_paged(qn, knn, vn.contiguous(), Kc, Vc, table, cos, sin, plan, lens, Q_out=Qc, **kw)

    calls = {"a": a, "b": b, "c": c}
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    differ = float((Qa.view(torch.int16) != Qc.view(torch.int16)).float().mean())
    close = bool(torch.allclose(Qa.float(), Qc.float(), rtol=2.0 ** -6, atol=2.0 ** -6))
    same_v = bool(torch.equal(Va.view(torch.uint8), Vb.view(torch.uint8)) and torch.equal(Va.view(torch.uint8), Vc.view(torch.uint8)))
    calls.update({k + "2": v for k, v in list(calls.items())})
    t = time_variants(calls, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b", "c")}
    read = T * (HQ + 2 * HKV) * D * 2 + (HQ + HKV) * 2 * T * (D // 2) * 4      # the three sources; a table row pair per (head, token)
    written = T * HQ * D * 2 + 2 * T * HKV * D * (1 if fp8 else 2)
    return {"workload": name, "B": B, "total_q": T, "H_q": HQ, "H_kv": HKV, "head_dim": D, "rot_dim": D, "eps": EPS,
            "cache": cache_dtype, "kv_capacity": cap, "page_size": PAGE, "ms": ms, "spread_ms": spread,
            "bytes_read": read, "bytes_written": written, "a_over_b": round(t["a"] / t["b"], 4), "a_over_c": round(t["a"] / t["c"], 4),
            "a_TBps": round((read + written) / (t["a"] * 1e-3) / 1e12, 4), "b_TBps": round((read + written) / (t["b"] * 1e-3) / 1e12, 4),
            "q_out_share_differing_from_framework_route": round(differ, 6), "q_out_close_to_framework_route": close,
            "v_same_bytes_in_all_arms": same_v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "qk_norm_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1357)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "norm_rope_kv_cache_append_ragged_paged with a prebuilt plan: one launch",
                    "b": "rope_kv_cache_append_ragged_paged on the raw source: the same launch without a norm",
                    "c": "two RMSNorms written in torch (fp32 inside, contiguous bf16 copies of Q and K), V_new.contiguous(), then "
                         "rope_kv_cache_append_ragged_paged"},
           "cases": []}
    for name, qs in WORKLOADS:
        if name not in NAMES:
            continue
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
