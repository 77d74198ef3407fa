"""Ragged extend attention against the cheapest route a caller had before it, timed in ONE process on one device (dev aid; bench.py
is untouched; the method of tools/gpu_extend_time.py).

    python tools/gpu_extend_ragged_time.py [--out profiles/extend_ragged_times.json] [--min-launches 40] [--min-seconds 0.25]

d = 128, the causal mask, 32 heads on 8, paged bf16 and paged e4m3 caches (pages of 64 keys behind a shuffled table), every sequence
at 8192 and at 32768 keys, n_splits = 0 everywhere (each call's own default):
    mixed-first, mixed-last   one 512-token chunk plus 63 decodes, the chunk first / last in the batch: the pair measures the order
                              of the work items
    verify-mix                32 sequences at q_b = 8 plus 32 at q_b = 1
    uniform                   8 sequences at q_b = 8
    x, x2   the ragged call (flash_attention_2_extend_ragged_paged) on a plan built before, the plan excluded
    p, p2   the plan launch alone (extend_ragged_plan into a caller's buffer)
    a, a2   the cheapest route without it: one flash_attention_2_extend_paged call per distinct q_len, on table rows and lengths
            gathered outside the timed region, Q already in each call's [B, H_q, q_len, d] layout, outputs preallocated -- which
            favours a: the gathers, the transposes and the scatter of O are not timed
    u, u2   uniform only: the uniform call (flash_attention_2_extend_paged)
Every arm is timed twice; |x - x2| is the spread of the method and goes into the file.  Nothing is fixed in advance: the medians
and the verdicts go into the JSON, whatever they are.  The condition on record: x is not above a on any mixed row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402
from gpu_extend_time import D, caches, descales, paged  # noqa: E402

HQ, HKV = 32, 8
LENS = (8192, 32768)
SHAPES = (("mixed-first", (512,) + (1,) * 63), ("mixed-last", (1,) * 63 + (512,)), ("verify-mix", (8,) * 32 + (1,) * 32), ("uniform", (8,) * 8))
SCALE = 1.0 / D ** 0.5


def ragged_arms(Q, Kp, Vp, table, lens, qs, fp8, cap):
    dev = Q.device
    B, T = len(qs), Q.shape[0]
    cu = torch.tensor([sum(qs[:b]) for b in range(B + 1)], dtype=torch.int32, device=dev)
    plan = fa.extend_ragged_plan(cu, HQ, HKV, T)
    buf = torch.empty_like(plan.tensor)
    O, L = torch.empty_like(Q), torch.empty(T, HQ, dtype=torch.float32, device=dev)
    ws = fa.extend_ragged_workspace(B, HQ, HKV, T, cap, D, 0, device=dev)
    kw = dict(causal=True, n_splits=0, O=O, L=L, workspace=ws, **descales(HKV, fp8, dev))
    x = lambda: fa.flash_attention_2_extend_ragged_paged(Q, Kp, Vp, table, plan, lens, SCALE, **kw)
    p = lambda: fa.extend_ragged_plan(cu, HQ, HKV, T, plan=buf)
    return x, p, (O, L)


def grouped_arm(Q, Kp, Vp, table, lens, qs, fp8, cap):
    """One uniform call per distinct q_len; everything a caller would gather or transpose is prepared here, outside the timing."""
    dev = Q.device
    cu = [sum(qs[:b]) for b in range(len(qs) + 1)]
    calls, outs = [], []
    for q in sorted(set(qs)):
        idx = [b for b, v in enumerate(qs) if v == q]
        Qg = torch.stack([Q[cu[b]:cu[b] + q].transpose(0, 1) for b in idx]).contiguous()      # [B_q, H_q, q, d]
        tg, lg = table[idx].contiguous(), lens[idx].contiguous()
        O, L = torch.empty_like(Qg), torch.empty(len(idx), HQ, q, dtype=torch.float32, device=dev)
        ws = fa.extend_workspace(len(idx), HQ, HKV, q, cap, D, 0, device=dev)
        kw = dict(causal=True, n_splits=0, O=O, L=L, workspace=ws, **descales(HKV, fp8, dev))
        calls.append(lambda Qg=Qg, tg=tg, lg=lg, kw=kw: fa.flash_attention_2_extend_paged(Qg, Kp, Vp, tg, lg, SCALE, **kw))
        outs.append((idx, q, O))

    def run():
        for c in calls:
            c()
    return run, len(calls), outs


def one_case(name, qs, n, fp8, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    B, T = len(qs), sum(qs)
    Q = (torch.rand(T, HQ, D, device=dev, generator=g) - 0.5).bfloat16()
    Kc, Vc = caches(B, HKV, n, fp8, g)
    Kp, Vp, table = paged(Kc, Vc, g)
    del Kc, Vc
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    x, p, (Ox, _) = ragged_arms(Q, Kp, Vp, table, lens, qs, fp8, n)
    a, n_calls, outs = grouped_arm(Q, Kp, Vp, table, lens, qs, fp8, n)
    variants = {"x": x, "a": a, "p": p}
    if name == "uniform":
        variants["u"] = a      # one distinct q_len: the grouped route IS the uniform call
    x(), a()
    torch.cuda.synchronize()
    cu = [sum(qs[:b]) for b in range(B + 1)]
    same = all(torch.equal(Ox[cu[b]:cu[b] + q].transpose(0, 1).contiguous().view(torch.int16), O[j].view(torch.int16))
               for idx, q, O in outs for j, b in enumerate(idx))
    variants.update({k + "2": v for k, v in list(variants.items())})
    t = time_variants(variants, min_launches, min_seconds)
    arms = [k for k in variants if not k.endswith("2")]
    spread = {k: abs(t[k] - t[k + "2"]) for k in arms}
    res = {"shape": name, "B": B, "H_q": HQ, "H_kv": HKV, "total_q": T, "q_lens": sorted(set(qs), reverse=True), "len": n, "head_dim": D,
           "kv": "e4m3" if fp8 else "bf16", "layout": "paged",
           "n_splits": {"x": fa.extend_ragged_num_splits(B, HQ, HKV, T, n, D),
                        "a": [fa.extend_num_splits(sum(v == q for v in qs), HQ, HKV, q, n, D) for q in sorted(set(qs))]},
           "a_calls": n_calls, "x_rows_equal_a_rows_bitwise": bool(same),
           "ms": {k: round(v, 5) for k, v in t.items()}, "spread_ms": {k: round(v, 5) for k, v in spread.items()},
           "x_over_a": round(t["x"] / t["a"], 4), "p_over_x": round(t["p"] / t["x"], 4),
           "x_not_above_a": bool(min(t["x"], t["x2"]) <= max(t["a"], t["a2"]))}
    if "u" in t:
        res["x_over_u"] = round(t["x"] / t["u"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "extend_ragged_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1357)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"x": "the ragged call on a plan built before, n_splits = 0", "p": "the plan launch alone",
                    "a": "one flash_attention_2_extend_paged call per distinct q_len, gathers and transposes outside the timing",
                    "u": "uniform only: the uniform call (the same closure as a)"},
           "cases": []}
    for name, qs in SHAPES:
        for n in LENS:
            for fp8 in (False, True):
                r = one_case(name, qs, n, fp8, a.min_launches, a.min_seconds, g)
                res["cases"].append(r)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
    mixed = [r for r in res["cases"] if r["shape"].startswith("mixed")]
    res["x_not_above_a_on_every_mixed_row"] = all(r["x_not_above_a"] for r in mixed)
    first = {(r["len"], r["kv"]): r["ms"]["x"] for r in mixed if r["shape"] == "mixed-first"}
    res["x_last_over_first"] = {f"{n}-{kv}": round(r["ms"]["x"] / first[(n, kv)], 4) for r in mixed if r["shape"] == "mixed-last"
                                for n, kv in [(r["len"], r["kv"])]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
