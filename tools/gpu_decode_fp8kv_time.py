"""Decode attention over fp8 (e4m3) KV caches against the bf16 call on the same logical cache and against a copy of the fp8 bytes,
timed in ONE process on one device (dev aid; bench.py is untouched; the method and the shapes of tools/gpu_decode_time.py).

    python tools/gpu_decode_fp8kv_time.py [--out profiles/decode_fp8kv_times.json] [--min-launches 40] [--min-seconds 0.25]

d = 128, N_q = 1 (one line with N_q = 4), (H_q, H_kv) in {(64, 8), (32, 8), (16, 16)}, (B, len) in {(1, 4096), (1, 32768), (1, 131072),
(8, 8192), (64, 2048)}, every sequence at the full length of its cache; plus two paged lines (page sizes 64 and 256, pages assigned
by a seeded permutation) at (64, 8), B = 8, len = 8192.
    a, a2   the fp8 call: flash_attention_2_decode (flash_attention_2_decode_paged) on e4m3 caches with per-head descales
    b, b2   the bf16 call on the same logical cache (the dequantised values, rounded to bf16): the existing code, the yardstick
    c, c2   a device-to-device copy of exactly the fp8 K and V bytes (two copy_ calls): the bandwidth yardstick of arm a
n_splits = 0 (the default rule) and a caller workspace in a and b.  Every arm is timed twice; |x - x2| is the spread of the method.
    sweep   at (B, len) = (1, 32768) and (8, 8192), (H_q, H_kv) = (64, 8): the fp8 call with n_splits = 1, 2, 4, ... 256, twice each
The ideal a / b is 0.5, from the bytes; nothing is fixed in advance: the medians and the verdicts go into the JSON, whatever they
are.  `faster_beyond_spread` (shapes whose bf16 K + V is at least 128 MB): max(a, a2) + the largest spread < min(b, b2)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, D, SHAPES, time_variants  # noqa: E402

SWEEPS = [(64, 8, 1, 1, 32768), (64, 8, 1, 8, 8192)]
PAGED = [((64, 8, 1, 8, 8192), 64), ((64, 8, 1, 8, 8192), 256)]
E4M3 = torch.float8_e4m3fn
BIG = 128 << 20      # bf16 K + V bytes from which the call streams the cache


def quantised(X):
    """(X8, descale [H_kv], the dequantised values in bf16) of a device tensor [*, H_kv, *, d], head by head (memory)."""
    X8, Xd = torch.empty(X.shape, dtype=E4M3, device=X.device), torch.empty_like(X)
    descale = torch.empty(X.shape[1], dtype=torch.float32, device=X.device)
    for h in range(X.shape[1]):
        x = X[:, h].float()
        descale[h] = x.abs().amax() / 448.0
        X8[:, h] = (x / descale[h]).clamp(-448.0, 448.0).to(E4M3)
        Xd[:, h] = (X8[:, h].float() * descale[h]).bfloat16()
    return X8, descale, Xd


def tensors(hq, hkv, nq, B, n, g):
    dev = torch.device("cuda")
    mk = lambda h, rows: (torch.rand(B, h, rows, D, device=dev, generator=g) - 0.5).bfloat16()
    Q = mk(hq, nq)
    K8, kd, K = quantised(mk(hkv, n))
    V8, vd, V = quantised(mk(hkv, n))
    return Q, K8, V8, kd, vd, K, V, torch.full((B,), n, dtype=torch.int32, device=dev)


def decode_call(Q, K, V, lens, n_splits, table=None, **descales):
    B, hq, nq, _ = Q.shape
    hkv = K.shape[1]
    cap = K.shape[2] * (table.shape[1] if table is not None else 1)
    O, L = torch.empty_like(Q), torch.empty(B, hq, nq, dtype=torch.float32, device=Q.device)
    ws = fa.decode_workspace(B, hq, hkv, nq, cap, D, n_splits, device=Q.device)
    kw = dict(causal=True, n_splits=n_splits, O=O, L=L, workspace=ws, **descales)
    s = 1.0 / D ** 0.5
    if table is not None:
        return lambda: fa.flash_attention_2_decode_paged(Q, K, V, table, lens, s, **kw)
    return lambda: fa.flash_attention_2_decode(Q, K, V, lens, s, **kw)


def paged(X, P, perm):
    """[B, H_kv, n, d] -> the pool [B n / P, H_kv, P, d] with logical page j of sequence b at perm[b n / P + j]."""
    B, hkv, n, d = X.shape
    pool = torch.empty(B * n // P, hkv, P, d, dtype=X.dtype, device=X.device)
    pool.view(torch.uint8 if X.dtype == E4M3 else X.dtype)[perm] = \
        X.view(B, hkv, n // P, P, d).permute(0, 2, 1, 3, 4).reshape(-1, hkv, P, d).view(torch.uint8 if X.dtype == E4M3 else X.dtype)
    return pool


def one_shape(shape, min_launches, min_seconds, g, P=None):
    hq, hkv, nq, B, n = shape
    Q, K8, V8, kd, vd, K, V, lens = tensors(hq, hkv, nq, B, n, g)
    table = None
    if P:
        perm = torch.randperm(B * n // P, device="cuda", generator=g)
        table = perm.view(B, n // P).int().contiguous()
        K8, V8, K, V = (paged(t, P, perm) for t in (K8, V8, K, V))
    Kc, Vc = torch.empty_like(K8), torch.empty_like(V8)
    a = decode_call(Q, K8, V8, lens, 0, table, k_descale=kd, v_descale=vd)
    b = decode_call(Q, K, V, lens, 0, table)
    c = lambda: (Kc.view(torch.uint8).copy_(K8.view(torch.uint8)), Vc.view(torch.uint8).copy_(V8.view(torch.uint8)))
    t = time_variants({"a": a, "b": b, "c": c, "a2": a, "b2": b, "c2": c}, min_launches, min_seconds)
    ms = {k: round(v, 5) for k, v in t.items()}
    spread = {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b", "c")}
    fp8_bytes = 2 * K8.numel()
    res = {"H_q": hq, "H_kv": hkv, "N_q": nq, "B": B, "len": n, "head_dim": D, "n_splits": fa.decode_num_splits(B, hkv, n, D),
           "ms": ms, "spread_ms": spread, "fp8_kv_bytes": fp8_bytes, "bf16_kv_bytes": 2 * fp8_bytes,
           "a_kv_TBps": round(fp8_bytes / (t["a"] * 1e-3) / 1e12, 3), "b_kv_TBps": round(2 * fp8_bytes / (t["b"] * 1e-3) / 1e12, 3),
           "a_over_b": round(t["a"] / t["b"], 4), "a_over_c": round(t["a"] / t["c"], 4)}
    if P:
        res["page_size"] = P
    if 2 * fp8_bytes >= BIG:
        res["faster_beyond_spread"] = bool(max(t["a"], t["a2"]) + max(spread["a"], spread["b"]) < min(t["b"], t["b2"]))
    return res


def one_sweep(shape, min_launches, min_seconds, g):
    hq, hkv, nq, B, n = shape
    Q, K8, V8, kd, vd, _, _, lens = tensors(hq, hkv, nq, B, n, g)
    counts = [c for c in (1, 2, 4, 8, 16, 32, 64, 128, 256) if c * 128 <= n]
    calls = {f"{c}": decode_call(Q, K8, V8, lens, c, k_descale=kd, v_descale=vd) for c in counts}
    for c in counts:
        calls[f"{c}'"] = calls[f"{c}"]
    t = time_variants(calls, min_launches, min_seconds)
    return {"H_q": hq, "H_kv": hkv, "N_q": nq, "B": B, "len": n, "head_dim": D, "default_n_splits": fa.decode_num_splits(B, hkv, n, D),
            "ms_by_n_splits": {str(c): round(t[f"{c}"], 5) for c in counts},
            "spread_ms_by_n_splits": {str(c): round(abs(t[f"{c}"] - t[f"{c}'"]), 5) for c in counts}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decode_fp8kv_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1357)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "the decode call on e4m3 caches with per-head descales, n_splits = 0",
                    "b": "the decode call on the same logical cache in bf16, n_splits = 0", "c": "device-to-device copy of the fp8 K and V bytes"},
           "cases": [], "paged": [], "sweeps": []}
    for shape in SHAPES:
        r = one_shape(shape, a.min_launches, a.min_seconds, g)
        res["cases"].append(r)
        print(json.dumps(r), flush=True)
    for shape, P in PAGED:
        r = one_shape(shape, a.min_launches, a.min_seconds, g, P)
        res["paged"].append(r)
        print(json.dumps(r), flush=True)
    for shape in SWEEPS:
        r = one_sweep(shape, a.min_launches, a.min_seconds, g)
        res["sweeps"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
