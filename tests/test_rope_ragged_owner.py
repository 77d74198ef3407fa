"""CPU: the ragged append's ownership rule (cuda_flashattention_amd/csrc/fa2_rope_ragged_owner.h, the ONLY code the kernel takes a
token's owner from) against the model (rope_ragged_ref.owners over extend_ragged_ref.plan_model), over a full enumeration.  The
header is compiled host-only into tests/rope_ragged_owner_main.cpp -- with -fsanitize=address,undefined where the toolchain
links that, so a read outside the 2 B pairs or an overflowing index ends the program; plain otherwise -- and asked about every
t in [-1, T] at T = 28 for the plans of every cu in these classes: all sequences empty, one sequence owning everything, runs of
empty sequences at the front, in the middle and at the end, each at B in 1, 2, 3, 37, 256, 257.
It is also asked about seeded GARBAGE pair arrays.  There only the safety property holds, and it must: the answer is "none", or
(b, i, q) with 0 <= b < B, 0 <= i < q and q the array's q_b."""
import math
import os
import random
import subprocess

import pytest

import extend_ragged_ref as xr
import rope_ragged_ref as gr
from capi_harness import HIPCC, ROOT

T = 28
BS = (1, 2, 3, 37, 256, 257)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rope_ragged_owner") / "rope_ragged_owner")
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "hip", "--cuda-host-only", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "cuda_flashattention_amd", "csrc"), os.path.join(ROOT, "tests", "rope_ragged_owner_main.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        subprocess.check_call(cmd)      # a toolchain without the sanitiser runtimes: the plain program
    return exe


def _cus(B):
    """cu lists of B + 1 entries, by class."""
    out = {"all empty": [5] * (B + 1), "all empty at 0": [0] * (B + 1), "all empty at T": [T] * (B + 1)}
    for b in sorted({0, B // 2, B - 1}):
        out[f"sequence {b} owns all"] = [0] * (b + 1) + [T] * (B - b)
        out[f"sequence {b} owns the middle"] = [3] * (b + 1) + [20] * (B - b)
    def from_q(first, qs):
        cu = [first]
        for q in qs:
            cu.append(min(cu[-1] + q, T))
        return cu

    if B >= 3:
        e = [0] * (B - 3)      # the empty sequences, beside three owners of 2, 7 and 19 tokens
        out["empty runs at the front"] = from_q(0, e + [2, 7, 19])
        out["empty runs at the end"] = from_q(0, [2, 7, 19] + e)
        out["empty runs in the middle"] = from_q(0, [2] + e + [7, 19])
        out["empty runs everywhere"] = from_q(1, e[:len(e) // 3] + [3] + e[:len(e) // 3] + [7] + e[:len(e) - 2 * (len(e) // 3)] + [15])
        out["every other one empty"] = from_q(0, [b % 2 for b in range(B)])      # (past T tokens every q is clamped to 0)
    assert all(len(c) == B + 1 for c in out.values()), {k: len(c) for k, c in out.items()}
    return out


def _ask(program, problems):
    text = "".join(f"{B} {T}\n" + " ".join(map(str, pairs)) + "\n" for B, pairs in problems)
    out = subprocess.run([program], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    answers, at = [], 0
    for B, _ in problems:
        iters = int(lines[at])
        rows = [tuple(map(int, ln.split())) for ln in lines[at + 1:at + 1 + T + 2]]
        assert len(rows) == T + 2
        answers.append((iters, rows))
        at += T + 3
    return answers


def test_header_equals_the_model_on_every_plan(program):
    problems, wants, names = [], [], []
    for B in BS:
        for name, cu in _cus(B).items():
            for G in (1, 4):
                plan = xr.plan_model(cu, G, T)
                assert plan[:3] == [B, G, T]
                problems.append((B, plan[xr.HEADER:xr.HEADER + 2 * B]))
                wants.append(gr.owners(cu, T))
                names.append((B, name, G))
    seen_owned = seen_none = 0
    for (B, _), want, name, (iters, rows) in zip(problems, wants, names, _ask(program, problems)):
        assert iters == (0 if B == 1 else math.ceil(math.log2(B))), name
        assert rows[0] == (-1, 0, 0) and rows[-1] == (-1, 0, 0), name          # t = -1 and t = T
        for t in range(T):
            assert rows[t + 1] == ((-1, 0, 0) if want[t] is None else want[t]), (name, t)
            seen_owned += want[t] is not None
            seen_none += want[t] is None
    assert seen_owned and seen_none


def test_garbage_pairs_keep_the_safety_property(program):
    rng = random.Random(20240)
    pools = ([INT_MIN, INT_MAX, -1, 0, 1, T - 1, T, T + 1], list(range(-2, T + 3)))
    problems = []
    for B in BS:
        for k in range(12):
            pool = pools[k % 2]
            pairs = [rng.choice(pool) if k % 3 else rng.randint(INT_MIN, INT_MAX) for _ in range(2 * B)]
            if k % 4 == 3:      # small values, so that many entries pass the pair test
                pairs = [rng.randint(0, T) for _ in range(2 * B)]
            problems.append((B, pairs))
    owned = 0
    for (B, pairs), (_, rows) in zip(problems, _ask(program, problems)):
        assert rows[0] == (-1, 0, 0) and rows[-1] == (-1, 0, 0)
        for t in range(T):
            b, i, q = rows[t + 1]
            if b == -1:
                continue
            owned += 1
            assert 0 <= b < B and 0 <= i < q and q == pairs[2 * b + 1], (B, t, rows[t + 1])
    assert owned
