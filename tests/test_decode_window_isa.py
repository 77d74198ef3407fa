"""CPU: the windowed decode kernels of fa2_decode.hip as the compiler left them (`make asm`, the shipped flags), from the
metadata alone, as tests/test_decode_isa.py reads it: each of the four exists once per head dim, none uses scratch memory or
spills a VGPR, d = 128 stays at or under 256 VGPRs with no AGPR (two workgroups per CU, like the plain kernel at 244), and each
runs v_mfma_f32_32x32x16_bf16."""
import os
import subprocess

import pytest

from test_isa_guard import CSRC, _kernels

NAMES = ("fa2_decode_win_split_kernel", "fa2_decode_win_paged_split_kernel", "fa2_decode_win_f8_split_kernel",
         "fa2_decode_win_f8_paged_split_kernel")


@pytest.fixture(scope="module")
def kernels():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return _kernels(open(os.path.join(CSRC, "_obj", "fa2_decode.s")).read())


def _window_kernels(kernels):
    return {n: k for n, k in kernels.items() if "fa2_decode_win_" in n}


def test_each_window_kernel_exists_once_per_head_dim(kernels):
    for d in (64, 128):
        for name in NAMES:
            assert sum(f"{name}ILi{d}E" in n for n in kernels) == 1, (name, d, sorted(kernels))
    assert len(_window_kernels(kernels)) == 2 * len(NAMES)


def test_the_names_do_not_collide_with_the_plain_kernels_counts(kernels):
    """tests/test_decode_isa.py and test_decode_fp8kv_isa.py count mangled names by these substrings."""
    for sub in ("fa2_decode_split_kernelILi", "fa2_decode_paged_split_kernelILi", "fa2_decode_f8_split_kernelILi",
                "fa2_decode_f8_paged_split_kernelILi"):
        assert not any(sub in n for n in _window_kernels(kernels)), sub
        assert sum(sub in n for n in kernels) == 2, sub


def test_no_scratch_no_spill(kernels):
    win = _window_kernels(kernels)
    assert win
    for name, k in win.items():
        assert k["meta"]["scratch"] == 0 and k["meta"]["vgpr_spill"] == 0, (name, k["meta"])


def test_head_dim_128_fits_two_workgroups_per_cu(kernels):
    for name, k in _window_kernels(kernels).items():
        print(name, k["meta"])
        assert k["meta"]["agpr"] == 0, (name, k["meta"])
        if "ILi128E" in name:
            assert k["meta"]["total"] <= 256, (name, k["meta"])      # (total: VGPRs and AGPRs together)


def test_window_kernels_use_the_bf16_mfma(kernels):
    for name, k in _window_kernels(kernels).items():
        assert any("v_mfma_f32_32x32x16_bf16" in l for l in k["body"]), name
