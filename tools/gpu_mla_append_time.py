"""The MLA latent-cache append against the framework composition it replaces, timed in ONE process on one device (dev aid;
bench.py is untouched; the method of tools/gpu_decode_time.py, whose time_variants this uses).

    python tools/gpu_mla_append_time.py [--out profiles/mla_append_times.json] [--min-launches 40] [--min-seconds 0.25]

(B, H, n_new) in {(64, 128, 1), (8, 16, 2), (1, 128, 1), the cache-only fill (1, 0, 4096)}, each contiguous and paged (pages of 64
rows); the sources are the strided views a model has (kv_new a slice of the fused projection output, q_pe the slice at column 128
of [B, n_new, H, 192], q_nope the bmm output [H, B n_new, 512] viewed), every sequence filled to half its cache after the append.
    a, a2   mla_kv_cache_append / _paged with a caller Q_out: one launch
    b, b2   the framework composition on the same inputs: fp32 RMSNorm of the 512 latent columns, a rotate-half rotation of k_pe and
            of q_pe, index_put_ into the cache (paged: through a gather of the table), cat + transpose into Q_out [B, H, n_new, 576]
Every arm is timed twice; |x - x2| is the spread of the method.  Nothing is fixed in advance: the medians go into the JSON,
whatever they are, with the number of elements in which the two arms' cache rows and Q_out differ beside them (the composition
is the same formula in another order of roundings, so a few last bits may differ)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_flashattention_amd as fa  # noqa: E402
from gpu_decode_time import BLOCK, time_variants  # noqa: E402

SHAPES = [(64, 128, 1), (8, 16, 2), (1, 128, 1), (1, 0, 4096)]
PAGE, EPS = 64, 1e-6


def rotate_half(x, c, s):
    """x [..., 64] bf16, c and s broadcastable [..., 32] fp32 -> bf16, the framework way: fp32 arithmetic, one cat."""
    x1, x2 = x[..., :32].float(), x[..., 32:].float()
    return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).bfloat16()


def one_shape(B, H, n_new, paged, min_launches, min_seconds, g):
    dev = torch.device("cuda")
    cap = max(4096, 2 * n_new)
    rnd = lambda *s: ((torch.rand(*s, device=dev, generator=g) - 0.5) * 6).bfloat16()
    kv = rnd(B, n_new, 1536 + 576)[..., 1536:]
    q_nope = rnd(H, B * n_new, 512).view(H, B, n_new, 512).permute(1, 0, 2, 3) if H else None
    q_pe = rnd(B, n_new, H, 192)[..., 128:].permute(0, 2, 1, 3) if H else None
    ang = torch.arange(cap, device=dev, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(0, 64, 2, device=dev, dtype=torch.float64) / 64))
    cos, sin = ang.cos().float().contiguous(), ang.sin().float().contiguous()
    w = (torch.rand(512, device=dev, generator=g) + 0.5).float()
    lens = torch.full((B,), cap // 2, dtype=torch.int32, device=dev)
    mp = cap // PAGE
    table = torch.randperm(B * mp, device=dev, generator=g).to(torch.int32).view(B, mp) if paged else None
    shape = (B * mp, PAGE, 576) if paged else (B, cap, 576)
    Ca, Cb = torch.zeros(shape, dtype=torch.bfloat16, device=dev), torch.zeros(shape, dtype=torch.bfloat16, device=dev)
    Qa = torch.zeros(B, H, n_new, 576, dtype=torch.bfloat16, device=dev) if H else None
    steps = torch.arange(n_new, device=dev)

    if paged:
        a = lambda: fa.mla_kv_cache_append_paged(q_nope, q_pe, kv, Ca, table, cos, sin, w, EPS, lens, Q_out=Qa)
    else:
        a = lambda: fa.mla_kv_cache_append(q_nope, q_pe, kv, Ca, cos, sin, w, EPS, lens, Q_out=Qa)

    def b():
        pos = (lens[:, None] - n_new + steps[None, :]).long()                     # [B, n_new]; no host read of a length
        c, s = cos[pos], sin[pos]                                                  # [B, n_new, 32]
        x = kv[..., :512].float()
        latent = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w).bfloat16()
        row = torch.cat((latent, rotate_half(kv[..., 512:], c, s)), dim=-1)
        if paged:
            page = torch.gather(table.long(), 1, pos // PAGE)
            Cb.index_put_((page, pos % PAGE), row)
        else:
            Cb.index_put_((torch.arange(B, device=dev)[:, None], pos), row)
        if not H:
            return None
        return torch.cat((q_nope, rotate_half(q_pe, c[:, None], s[:, None])), dim=-1)      # [B, H, n_new, 576], contiguous

    t = time_variants({"a": a, "b": b, "a2": a, "b2": b}, min_launches, min_seconds)
    a()
    Qb = b()
    torch.cuda.synchronize()
    differ = int((Ca.view(torch.int16) != Cb.view(torch.int16)).sum()) + (int((Qa.view(torch.int16) != Qb.view(torch.int16)).sum()) if H else 0)
    moved = 2 * 2 * 576 * B * n_new * (H + 1)      # bytes: every 576-wide bf16 row (a cache row, H rows of Q_out) read once and written once
    return {"B": B, "H": H, "n_new": n_new, "paged": paged, "capacity": cap, "ms": {k: round(v, 5) for k, v in t.items()},
            "spread_ms": {k: round(abs(t[k] - t[k + "2"]), 5) for k in ("a", "b")}, "a_over_b": round(t["a"] / t["b"], 4),
            "bytes_moved": moved, "a_GBps": round(moved / (t["a"] * 1e-3) / 1e9, 1), "elements_differing_a_b": differ,
            "elements": Ca.numel() + (Qa.numel() if H else 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mla_append_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=0.25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(576)
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); every arm twice, spread = |x - x2|",
           "arms": {"a": "mla_kv_cache_append / _paged, one launch",
                    "b": "torch: fp32 RMSNorm, two rotations, index_put_ (paged: a gather of the table first), cat into [B, H, n_new, 576]"},
           "cases": []}
    for B, H, n_new in SHAPES:
        for paged in (False, True):
            r = one_shape(B, H, n_new, paged, a.min_launches, a.min_seconds, g)
            res["cases"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
