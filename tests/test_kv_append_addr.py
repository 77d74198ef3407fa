"""CPU: the append's position and address rule (cuda_flashattention_amd/csrc/fa2_kv_append_addr.h, the ONLY code the kernels form a
destination with) against the reference model of tests/kv_append_ref.py, over a full enumeration.  The header is compiled
host-only into tests/kv_append_addr_main.cpp (as capi_harness.build compiles host code) and asked about every combination of
    n_new in 1, 2, 3, 5; capacity 96; page_size in 32, 96; every token t;
    every length in -3..101 plus INT_MIN, INT_MIN + 1, INT_MAX - 1, INT_MAX;
    table entries -1, 0, n_pages - 1, n_pages, INT_MAX, INT_MIN.
Every answer equals the model's, and every returned offset lies inside the cache (the pool), whole row included, or the token is
reported dropped."""
import os
import subprocess

import pytest

import kv_append_ref as ar
from capi_harness import HIPCC, ROOT

CAP, B, H, D, N_PAGES = 96, 3, 2, 64, 8
LENGTHS = list(range(-3, 102)) + [ar.INT_MIN, ar.INT_MIN + 1, ar.INT_MAX - 1, ar.INT_MAX]
ENTRIES = (-1, 0, N_PAGES - 1, N_PAGES, ar.INT_MAX, ar.INT_MIN)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kv_append_addr") / "kv_append_addr")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "cuda_flashattention_amd", "csrc"),
                           os.path.join(ROOT, "tests", "kv_append_addr_main.cpp"), "-o", exe])
    return exe


def _queries():
    for n_new in (1, 2, 3, 5):
        for P in (32, 96):
            for length in LENGTHS:
                for t in range(n_new):
                    for b, h in ((0, 0), (B - 1, H - 1)):
                        for entry in ENTRIES:
                            yield length, n_new, t, CAP, b, h, H, D, entry, N_PAGES, P


def test_header_equals_the_model_everywhere(program):
    queries = list(_queries())
    out = subprocess.run([program], input="".join(" ".join(map(str, q)) + "\n" for q in queries), capture_output=True, text=True, check=True)
    answers = [tuple(map(int, line.split())) for line in out.stdout.splitlines()]
    assert len(answers) == len(queries)
    written = dropped = 0
    for q, (pos, off, ti, offp) in zip(queries, answers):
        length, n_new, t, cap, b, h, _, d, entry, n_pages, P = q
        want = ar.position(length, n_new, t, cap)
        assert pos == (-1 if want is None else want), q
        row = ar.row_contiguous(length, n_new, t, cap, b, h, H)
        assert off == (-1 if row is None else row * d), q
        assert ti == (-1 if want is None else ar.table_index(want, P)), q
        rowp = ar.row_paged(length, n_new, t, P, cap // P, entry, n_pages, h, H)
        assert offp == (-1 if rowp is None else rowp * d), q
        # inside the cache, whole row included, or dropped -- and a table read stays inside the sequence's row of the table
        assert off == -1 or 0 <= off <= (B * H * cap - 1) * d, q
        assert offp == -1 or 0 <= offp <= (n_pages * H * P - 1) * d, q
        assert ti == -1 or 0 <= ti < cap // P, q
        written += off >= 0
        dropped += off < 0
    assert written and dropped
