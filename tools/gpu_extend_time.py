"""Extend attention against the only route a caller had before it, timed in ONE process on one device (dev aid; bench.py is
untouched; the method of tools/gpu_decode_window_time.py and tools/gpu_decode_time.py).

    python tools/gpu_extend_time.py [--out profiles/extend_times.json] [--min-launches 40] [--min-seconds 0.25]

d = 128, every sequence at the full length of its cache, bf16 and e4m3 caches, contiguous and paged (pages of 64 keys behind a
shuffled table), the causal mask, no window, n_splits = 0 everywhere (each call's own default):
    verify   B = 8, (H_q, H_kv) = (64, 8), q_len = 8 (M = 64) against 8192 and 32768 keys: speculative-decoding verification
    mqa      B = 8, (H_q, H_kv) = (64, 1), q_len = 1 (M = 64) against 8192 and 32768 keys
    chunk    B = 1, (H_q, H_kv) = (32, 8), q_len = 512 (M = 2048) against 8192 and 32768 keys: a prefill chunk
    x, x2   the extend call (flash_attention_2_extend / _paged)
    a, a2   what the shipped decode kernels can do for the same rows, summed: one flash_attention_2_decode / _paged call per group
            member g on Q[:, g::G] (pre-sliced, outputs preallocated); for the chunk, whose q_len exceeds 32, per group member AND
            per slice of 32 tokens, each slice with the lengths its last token sees (len - q_len + 32 (t + 1)): the slices' rows
            are disjoint, so nothing is left to merge -- the cheapest form of that route
    b, b2   contiguous bf16 only: flash_attention_2_qk_forward on the cache (all sequences have the full length), for information
Every arm is timed twice; |x - x2| is the spread of the method and goes into the file.  Nothing is fixed in advance: the medians
and the verdicts go into the JSON, whatever they are.  The condition on record: x is not above a on any row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402
from gpu_decode_window_time import E4M3, PAGE  # noqa: E402

D = 128
SHAPES = (("verify", 8, 64, 8, 8), ("mqa", 8, 64, 1, 1), ("chunk", 1, 32, 8, 512))      # (name, B, H_q, H_kv, q_len)
LENS = (8192, 32768)
SLICE = 32


def caches(B, hkv, n, fp8, g):
    dev = torch.device("cuda")
    mk = lambda: (torch.rand(B, hkv, n, D, device=dev, generator=g) - 0.5).bfloat16()
    K, V = mk(), mk()
    if fp8:
        K, V = (K.float() * 64).to(E4M3), (V.float() * 64).to(E4M3)
    return K, V


def paged(K, V, g):
    """The pools and a shuffled table that hold the contiguous caches K, V [B, H_kv, n, D] (n a multiple of the page size)."""
    B, hkv, n, _ = K.shape
    mp = n // PAGE
    perm = torch.randperm(B * mp, device=K.device, generator=g)
    table = perm.view(B, mp).to(torch.int32)
    pools = []
    for t in (K, V):
        pages = t.view(torch.uint8 if t.dtype == E4M3 else t.dtype).view(B, hkv, mp, PAGE, D).permute(0, 2, 1, 3, 4).reshape(B * mp, hkv, PAGE, D)
        pool = torch.empty(pages.shape, dtype=pages.dtype, device=pages.device)
        pool[perm.long()] = pages
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], table


def descales(hkv, fp8, dev):
    return dict(k_descale=torch.full((hkv,), 1 / 64, device=dev), v_descale=torch.full((hkv,), 1 / 64, device=dev)) if fp8 else {}


def extend_call(Q, K, V, table, lens, fp8, cap):
    B, hq, nq, _ = Q.shape
    hkv = K.shape[1]
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device=Q.device)
    ws = fa.extend_workspace(B, hq, hkv, nq, cap, D, 0, device=Q.device)
    kw = dict(causal=True, n_splits=0, O=O, L=L, workspace=ws, **descales(hkv, fp8, Q.device))
    s = 1.0 / D ** 0.5
    if table is None:
        return lambda: fa.flash_attention_2_extend(Q, K, V, lens, s, **kw)
    return lambda: fa.flash_attention_2_extend_paged(Q, K, V, table, lens, s, **kw)


def sliced_calls(Q, K, V, table, n, fp8, cap):
    """The shipped kernels' route: per group member (and per 32 tokens of a longer q_len) one decode call, run one after the other."""
    B, hq, nq, _ = Q.shape
    hkv = K.shape[1]
    G = hq // hkv
    s = 1.0 / D ** 0.5
    calls = []
    for g in range(G):
        for t0 in range(0, nq, SLICE):
            t1 = min(t0 + SLICE, nq)
            q = Q[:, g::G, t0:t1].contiguous()
            lens = torch.full((B,), n - nq + t1, dtype=torch.int32, device=Q.device)
            O, L = torch.empty_like(q), torch.empty(B, hkv, t1 - t0, dtype=torch.float32, device=Q.device)
            ws = fa.decode_workspace(B, hkv, hkv, t1 - t0, cap, D, 0, device=Q.device)
            kw = dict(causal=True, n_splits=0, O=O, L=L, workspace=ws, **descales(hkv, fp8, Q.device))
            if table is None:
                calls.append(lambda q=q, lens=lens, kw=kw: fa.flash_attention_2_decode(q, K, V, lens, s, **kw))
            else:
                calls.append(lambda q=q, lens=lens, kw=kw: fa.flash_attention_2_decode_paged(q, K, V, table, lens, s, **kw))

    def run():
        for c in calls:
            c()
    return run, len(calls)


def one_case(name, B, hq, hkv, nq, n, fp8, is_paged, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    Q = (torch.rand(B, hq, nq, D, device=dev, generator=g) - 0.5).bfloat16()
    K, V = caches(B, hkv, n, fp8, g)
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    variants = {}
    if not fp8 and not is_paged:
        Ob, Lb = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device=dev)
        variants["b"] = lambda: fa.flash_attention_2_qk_forward(Q, K, V, 1.0 / D ** 0.5, causal=True, O=Ob, L=Lb)
    table = None
    if is_paged:
        Kc, Vc = K, V
        K, V, table = paged(Kc, Vc, g)
        del Kc, Vc
    x = extend_call(Q, K, V, table, lens, fp8, n)
    a, n_calls = sliced_calls(Q, K, V, table, n, fp8, n)
    variants = {"x": x, "a": a, **variants}
    variants.update({k + "2": v for k, v in list(variants.items())})
    t = time_variants(variants, min_launches, min_seconds)
    arms = [k for k in variants if not k.endswith("2")]
    spread = {k: abs(t[k] - t[k + "2"]) for k in arms}
    res = {"shape": name, "B": B, "H_q": hq, "H_kv": hkv, "q_len": nq, "len": n, "head_dim": D, "kv": "e4m3" if fp8 else "bf16",
           "layout": "paged" if is_paged else "contiguous", "rows_per_kv_head": hq // hkv * nq,
           "n_splits": {"x": fa.extend_num_splits(B, hq, hkv, nq, n, D), "a": fa.decode_num_splits(B, hkv, n, D)}, "a_calls": n_calls,
           "ms": {k: round(v, 5) for k, v in t.items()}, "spread_ms": {k: round(v, 5) for k, v in spread.items()},
           "x_over_a": round(t["x"] / t["a"], 4),
           "x_not_above_a": bool(min(t["x"], t["x2"]) <= max(t["a"], t["a2"]))}
    if "b" in t:
        res["x_over_b"] = round(t["x"] / t["b"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "extend_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(2468)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"x": "the extend call, n_splits = 0", "a": "the shipped decode kernels, one call per group member (and per 32 tokens), summed",
                    "b": "flash_attention_2_qk_forward on the contiguous bf16 cache (information)"},
           "cases": []}
    for name, B, hq, hkv, nq in SHAPES:
        for n in LENS:
            for is_paged in (False, True):
                for fp8 in (False, True):
                    r = one_case(name, B, hq, hkv, nq, n, fp8, is_paged, a.min_launches, a.min_seconds, g)
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
