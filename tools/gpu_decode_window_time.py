"""Windowed split-KV decode against what a caller had before it and against its floor, timed in ONE process on one device (dev
aid; bench.py is untouched; the method of tools/gpu_decode_time.py).

    python tools/gpu_decode_window_time.py [--out profiles/decode_window_times.json] [--min-launches 40] [--min-seconds 0.25]

d = 128, N_q = 1, (H_q, H_kv) = (64, 8), window_left in {127, 4095}, (B, len) in {(1, 4096), (1, 131072), (8, 8192), (64, 2048)}, bf16
and e4m3 caches, contiguous and paged (pages of 64 keys behind a shuffled table); every sequence at the full length of its cache.
    a, a2   the windowed call (window_left=), n_splits = 0 (the window's default rule), caller workspace
    b, b2   the plain call over the whole cache, n_splits = 0: what a caller does today (and numerically another result)
    c, c2   the plain call on a cache that holds only the window's window_left + 1 keys, n_splits = 0: the floor
Every arm is timed twice; |x - x2| is the spread of the method, per arm and case, and goes into the file.  Variants alternate in
blocks of a few launches (order reversed every other round) after a warm-up; every variant gets at least --min-launches timed
launches and --min-seconds of timed work; medians of the per-launch block times are reported.  Nothing is fixed in advance: the
medians and the verdicts go into the JSON, whatever they are.  The expectation on record: a is below b beyond the spread wherever
len > 2 (window_left + 128)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

D, HQ, HKV, PAGE = 128, 64, 8, 64
WINDOWS = (127, 4095)
BATCHES = ((1, 4096), (1, 131072), (8, 8192), (64, 2048))
E4M3 = torch.float8_e4m3fn


def caches(B, n, fp8, g):
    dev = torch.device("cuda")
    mk = lambda: (torch.rand(B, HKV, n, D, device=dev, generator=g) - 0.5).bfloat16()
    K, V = mk(), mk()
    if fp8:
        K, V = (K.float() * 64).to(E4M3), (V.float() * 64).to(E4M3)
    return K, V


def paged(K, V, g):
    """The pools and a shuffled table that hold the contiguous caches K, V [B, HKV, n, D] (n a multiple of the page size)."""
    B, _, n, _ = K.shape
    mp = n // PAGE
    perm = torch.randperm(B * mp, device=K.device, generator=g)
    table = perm.view(B, mp).to(torch.int32)
    pools = []
    for t in (K, V):
        pages = t.view(torch.uint8 if t.dtype == E4M3 else t.dtype).view(B, HKV, mp, PAGE, D).permute(0, 2, 1, 3, 4).reshape(B * mp, HKV, PAGE, D)
        pool = torch.empty(pages.shape, dtype=pages.dtype, device=pages.device)
        pool[perm.long()] = pages
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], table


def call(Q, K, V, table, lens, fp8, wl):
    B = Q.shape[0]
    cap = K.shape[2] if table is None else table.shape[1] * PAGE
    O, L = torch.empty_like(Q), torch.empty(B, HQ, 1, dtype=torch.float32, device=Q.device)
    ws = fa.decode_workspace(B, HQ, HKV, 1, cap, D, 0, device=Q.device, q_len=1, window_left=wl)
    desc = dict(k_descale=torch.full((HKV,), 1 / 64, device=Q.device), v_descale=torch.full((HKV,), 1 / 64, device=Q.device)) if fp8 else {}
    kw = dict(causal=True, n_splits=0, O=O, L=L, workspace=ws, window_left=wl, **desc)
    s = 1.0 / D ** 0.5
    if table is None:
        return lambda: fa.flash_attention_2_decode(Q, K, V, lens, s, **kw)
    return lambda: fa.flash_attention_2_decode_paged(Q, K, V, table, lens, s, **kw)


def one_case(B, n, wl, fp8, is_paged, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    Q = (torch.rand(B, HQ, 1, D, device=dev, generator=g) - 0.5).bfloat16()
    K, V = caches(B, n, fp8, g)
    keys = wl + 1                                             # what one query sees: the floor's whole cache
    Ks, Vs = K[:, :, n - keys:].contiguous(), V[:, :, n - keys:].contiguous()
    lens, lens_s = torch.full((B,), n, dtype=torch.int32, device=dev), torch.full((B,), keys, dtype=torch.int32, device=dev)
    table = table_s = None
    if is_paged:
        K, V, table = paged(K, V, g)
        Ks, Vs, table_s = paged(Ks, Vs, g)
    a = call(Q, K, V, table, lens, fp8, wl)
    b = call(Q, K, V, table, lens, fp8, None)
    c = call(Q, Ks, Vs, table_s, lens_s, fp8, None)
    t = time_variants({"a": a, "b": b, "c": c, "a2": a, "b2": b, "c2": c}, min_launches, min_seconds)
    spread = {k: abs(t[k] - t[k + "2"]) for k in ("a", "b", "c")}
    worst = max(spread.values())
    res = {"B": B, "len": n, "window_left": wl, "kv": "e4m3" if fp8 else "bf16", "layout": "paged" if is_paged else "contiguous",
           "H_q": HQ, "H_kv": HKV, "N_q": 1, "head_dim": D,
           "n_splits": {"a": fa.decode_num_splits(B, HKV, n, D, q_len=1, window_left=wl), "b": fa.decode_num_splits(B, HKV, n, D),
                        "c": fa.decode_num_splits(B, HKV, keys, D)},
           "ms": {k: round(v, 5) for k, v in t.items()}, "spread_ms": {k: round(v, 5) for k, v in spread.items()},
           "a_over_b": round(t["a"] / t["b"], 4), "a_over_c": round(t["a"] / t["c"], 4),
           "a_above_c_beyond_spread": bool(min(t["a"], t["a2"]) > max(t["c"], t["c2"]) + worst)}
    if n > 2 * (wl + 128):
        res["expect_a_below_b_beyond_spread"] = bool(max(t["a"], t["a2"]) + worst < min(t["b"], t["b2"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "decode_window_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1357)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "the windowed call, n_splits = 0", "b": "the plain call over the whole cache, n_splits = 0",
                    "c": "the plain call on a cache of the window's window_left + 1 keys, n_splits = 0"},
           "cases": []}
    for is_paged in (False, True):
        for fp8 in (False, True):
            for wl in WINDOWS:
                for B, n in BATCHES:
                    r = one_case(B, n, wl, fp8, is_paged, a.min_launches, a.min_seconds, g)
                    res["cases"].append(r)
                    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
