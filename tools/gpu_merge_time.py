"""What the differentiable log-sum-exp and the merge of partial results cost, timed in ONE process on one device (dev aid; bench.py
is untouched; the alternating-blocks method of tools/gpu_sink_time.py).

    python tools/gpu_merge_time.py [--out profiles/merge_times.json] [--min-launches 40] [--min-seconds 1.0]

(a) fa2_merge_states and fa2_merge_states_backward, n = 2 and n = 4 parts, R = 4 x 16 x 8192 rows at d = 128 and 4 x 16 x 4096 rows at
    d = 64, each beside a device-to-device copy that moves the same number of bytes (read + written: a copy of half of them), and
    a second copy of that copy (the spread).  Both in GB/s; the ratio merge / copy is reported, not gated.
(b) backward phase 1 (the D kernel) plain / plain2 / with dL, at (4, 16, 8192, 128) and (4, 16, 4096, 64).
(c) attention_segments, forward and forward + backward by autograd: a prefix of 4096 keys + a chunk of 512, causal, B = 8, H = 16,
    d = 128, against (i) torch.cat of K and V plus one attention_qk call and (ii) attention_qk on an already concatenated cache
    (twice: the spread).
Nothing is fixed in advance: the medians, the spreads and the verdicts go into the JSON, whatever they are."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cuda_flashattention_amd as fa  # noqa: E402

BLOCK = 5          # launches between two events


def time_variants(calls, min_launches, min_seconds):
    """calls: name -> callable.  Returns name -> median ms per launch (tools/gpu_sink_time.py)."""
    names = list(calls)
    for n in names:
        for _ in range(3):
            calls[n]()
    torch.cuda.synchronize()
    blocks = {n: [] for n in names}
    rnd = 0
    while any(len(blocks[n]) * BLOCK < min_launches or sum(blocks[n]) * BLOCK < min_seconds * 1e3 for n in names):
        for n in (names if rnd % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                calls[n]()
            e1.record()
            e1.synchronize()
            blocks[n].append(e0.elapsed_time(e1) / BLOCK)
        rnd += 1
    return {n: round(statistics.median(blocks[n]), 4) for n in names}


def merge_case(rows, d, a):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1357)
    row_bytes = 2 * d + 4                                  # a bf16 row of O and its fp32 L
    res = {"rows": rows, "head_dim": d, "n": {}}
    for n in (2, 4):
        Os = [(torch.rand(rows, d, device=dev, generator=g) - 0.5).bfloat16() for _ in range(n)]
        Ls = [torch.rand(rows, device=dev, generator=g) * 4 + 5 for _ in range(n)]
        O, L = torch.empty_like(Os[0]), torch.empty_like(Ls[0])
        dO, dL = (torch.rand(rows, d, device=dev, generator=g) - 0.5).bfloat16(), torch.rand(rows, device=dev, generator=g)
        dOs, dLs = [torch.empty_like(O) for _ in range(n)], [torch.empty_like(L) for _ in range(n)]
        fwd_bytes, bwd_bytes = (n + 1) * rows * row_bytes, (2 * n + 2) * rows * row_bytes
        src_f, dst_f = (torch.empty(fwd_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        src_b, dst_b = (torch.empty(bwd_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        fa.merge_states_forward(Os, Ls, O=O, L=L)
        t = time_variants({"merge": lambda: fa.merge_states_forward(Os, Ls, O=O, L=L), "copy": lambda: dst_f.copy_(src_f),
                           "copy2": lambda: dst_f.copy_(src_f),
                           "merge_backward": lambda: fa.merge_states_backward(Os, Ls, O, L, dO, dL, dOs=dOs, dLs=dLs),
                           "copy_backward": lambda: dst_b.copy_(src_b), "copy_backward2": lambda: dst_b.copy_(src_b)},
                          a.min_launches, a.min_seconds)
        gbs = lambda nbytes, ms: round(nbytes / ms / 1e6, 1)
        r = {"ms": t, "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
             "GBps": {"merge": gbs(fwd_bytes, t["merge"]), "copy": gbs(fwd_bytes, t["copy"]), "copy2": gbs(fwd_bytes, t["copy2"]),
                      "merge_backward": gbs(bwd_bytes, t["merge_backward"]), "copy_backward": gbs(bwd_bytes, t["copy_backward"]),
                      "copy_backward2": gbs(bwd_bytes, t["copy_backward2"])}}
        r["forward_time_over_copy"] = round(t["merge"] / t["copy"], 3)
        r["backward_time_over_copy"] = round(t["merge_backward"] / t["copy_backward"], 3)
        res["n"][str(n)] = r
        print(f"merge rows={rows} d={d} n={n}: {r['ms']} GB/s {r['GBps']}", flush=True)
        del Os, Ls, O, L, dO, dL, dOs, dLs, src_f, dst_f, src_b, dst_b
    return res


def dl_case(shape, a):
    B, H, N, D = shape
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(2468)
    s = 1.0 / D ** 0.5
    mk = lambda sc: ((torch.rand(B, H, N, D, device=dev, generator=g) - 0.5) * sc).bfloat16()
    Q, K, V, dO = mk(1.0), mk(1.0), mk(1.0), mk(0.4)
    O, L = fa.flash_attention_2_qk_forward(Q, K, V, s)
    dL = torch.rand(B, H, N, device=dev, generator=g) * 0.01
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    ws = torch.empty(fa._capi.lib().fa2_backward_qk_workspace_bytes(B, H, H, N, N, D, 0), dtype=torch.uint8, device=dev)
    run = lambda gl: fa.flash_attention_2_qk_backward(Q, K, V, O, L, dO, s, dQ=dQ, dK=dK, dV=dV, workspace=ws, phases=1, dL=gl)
    t = time_variants({"plain": lambda: run(None), "plain2": lambda: run(None), "with_dL": lambda: run(dL)}, a.min_launches, a.min_seconds)
    r = {"shape": list(shape), "d_kernel_ms": t, "spread_ms": round(abs(t["plain"] - t["plain2"]), 4),
         "with_dL_minus_plain_ms": round(t["with_dL"] - t["plain"], 4)}
    r["expect_within_spread"] = r["with_dL_minus_plain_ms"] <= r["spread_ms"]
    print(f"phase 1 {shape}: {t} {r['expect_within_spread']}", flush=True)
    return r


def segments_case(a, B=8, H=16, prefix=4096, chunk=512, D=128):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3579)
    mk = lambda n, sc: ((torch.rand(B, H, n, D, device=dev, generator=g) - 0.5) * sc).bfloat16()
    Q, Kp, Vp, Kc, Vc, dO = mk(chunk, 1.0), mk(prefix, 1.0), mk(prefix, 1.0), mk(chunk, 1.0), mk(chunk, 1.0), mk(chunk, 0.4)
    Kall, Vall = torch.cat([Kp, Kc], dim=2), torch.cat([Vp, Vc], dim=2)
    leaves = [t.requires_grad_(True) for t in (Q, Kp, Vp, Kc, Vc, Kall, Vall)]

    def seg():
        return fa.attention_segments(Q, [(Kp, Vp), (Kc, Vc)], causal=True)

    def cat():
        return fa.attention_qk(Q, torch.cat([Kp, Kc], dim=2), torch.cat([Vp, Vc], dim=2), causal=True)

    def pre():
        return fa.attention_qk(Q, Kall, Vall, causal=True)

    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def both(f):
        def run():
            for t in leaves:
                t.grad = None
            f().backward(dO)
        return run

    tf = time_variants({"segments": fwd(seg), "cat_then_qk": fwd(cat), "qk_on_concatenated": fwd(pre), "qk_on_concatenated2": fwd(pre)},
                       a.min_launches, a.min_seconds)
    tb = time_variants({"segments": both(seg), "cat_then_qk": both(cat), "qk_on_concatenated": both(pre), "qk_on_concatenated2": both(pre)},
                       a.min_launches, a.min_seconds)
    r = {"B": B, "H": H, "prefix": prefix, "chunk": chunk, "head_dim": D, "causal": True, "forward_ms": tf, "forward_backward_ms": tb}
    for k, t in (("forward", tf), ("forward_backward", tb)):
        r[k + "_spread_ms"] = round(abs(t["qk_on_concatenated"] - t["qk_on_concatenated2"]), 4)
        r[k + "_segments_over_cat"] = round(t["segments"] / t["cat_then_qk"], 3)
        r[k + "_segments_over_concatenated"] = round(t["segments"] / t["qk_on_concatenated"], 3)
    print(f"segments {prefix}+{chunk}: fwd {tf} | fwd+bwd {tb}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "merge_times.json"))
    ap.add_argument("--min-launches", type=int, default=40)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"device": torch.cuda.get_device_name(0), "library": fa._capi.lib().fa2_version().decode(),
           "method": f"one process, variants alternate in blocks of {BLOCK} launches, >= {a.min_launches} launches and >= {a.min_seconds} s "
                     "timed per variant, medians of per-launch block times (ms); copy2 / plain2 / qk_on_concatenated2 are second copies "
                     "(the spread); a copy moves the merge's bytes, read + written",
           "merge": [merge_case(4 * 16 * 8192, 128, a), merge_case(4 * 16 * 4096, 64, a)],
           "phase1_with_dL": [dl_case((4, 16, 8192, 128), a), dl_case((4, 16, 4096, 64), a)],
           "segments": segments_case(a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
