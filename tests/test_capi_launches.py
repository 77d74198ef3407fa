"""CPU: every attention entry point of the C ABI, through stub launchers, against what it launched when the fixture was recorded.

tests/capi_harness.py builds fa2_capi.cpp host-only against tests/capi_stubs.cpp and walks a grid of calls; the fixture
tests/golden/capi_launches.txt.gz holds, per valid call, its status and the arguments every launcher saw, and per entry point
the status of each invalid row (one field, then every pair of fields set to a value no entry point accepts: the pairs pin the
ORDER of the checks).  A change of fa2_capi.cpp that alters which kernel runs, with what arguments, or which fault is reported
first shows here without a GPU.  The fixture is re-recorded (python tests/capi_harness.py record SRC) only when behaviour is
meant to change."""
import gzip
import os

import pytest

import capi_harness as ch


@pytest.fixture(scope="module")
def fixture_lines():
    with gzip.open(ch.FIXTURE, "rt") as f:
        return f.read().splitlines()


@pytest.fixture(scope="module")
def stub_lib(tmp_path_factory):
    src = os.path.join(ch.ROOT, "cuda_flashattention_amd", "csrc", "fa2_capi.cpp")
    return ch.build(src, str(tmp_path_factory.mktemp("capi_stub")))


def _compare(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if g == w:
            continue
        if g[1] != "I":
            assert g == w
        fn, digits = g[3:].split(" | ")
        assert w.startswith(f"{g[:3]}{fn} | ")
        want_digits = w.split(" | ")[1]
        rows = ch.invalid_combos(fn)
        assert len(digits) == len(want_digits) == len(rows)
        bad = [(fn, combo, -int(a), -int(b)) for combo, a, b in zip(rows, digits, want_digits) if a != b]
        assert not bad, f"(entry point, invalid fields, status now, status recorded): {bad[:10]}"


def test_fixture_invalid_rows_are_validation_codes(fixture_lines):
    """Every invalid row was refused by argument checking: none ran (0), none reached the HIP runtime (<= -1000)."""
    rows = [line for line in fixture_lines if line[1] == "I"]
    assert len(rows) == 28
    for line in rows:
        fn, digits = line[3:].split(" | ")
        assert len(digits) == len(ch.invalid_combos(fn)) > 10
        assert all(-int(c) in ch.VALIDATION_CODES for c in digits), fn


def test_fixture_covers_every_launcher_and_both_backward_paths(fixture_lines):
    valid = [line for line in fixture_lines if line[1] == "V"]
    assert len(valid) > 2000
    for launcher in ("fwd1_bf16", "fwd1_varlen_bf16", "fwd_f32", "fwd_fp8", "decode", "merge_fwd", "merge_bwd", "bwd_bf16",
                     "bwd_fused_bf16", "bwd_varlen_bf16", "bwd_f32", "clear_error", "finalize_state"):
        assert any(f"| {launcher} " in line or f";{launcher} " in line for line in valid), launcher
    two = [line for line in valid if line[0] == "T"]
    assert two and not any("bwd_fused_bf16" in line for line in two if "fa2_backward_fused" not in line and "phases=8" not in line
                           and "phases=9" not in line)


def test_launches_and_statuses_are_what_was_recorded(stub_lib, fixture_lines):
    _compare(ch.run_child(stub_lib, "main"), [line for line in fixture_lines if line[0] == "M"])


def test_launches_under_the_two_kernel_switch_are_what_was_recorded(stub_lib, fixture_lines):
    _compare(ch.run_child(stub_lib, "two_kernel"), [line for line in fixture_lines if line[0] == "T"])
