"""CPU: the decode kernels of fa2_decode.hip as the compiler left them (`make asm`, the shipped flags): no scratch memory, no
spilled VGPR, and the split kernels do run v_mfma_f32_32x32x16_bf16.  Nothing else of the assembly is inspected: the kernels are
plain compiler code with no hand-named registers (tests/test_isa_guard.py guards the files that have them)."""
import os
import subprocess

import pytest

from test_isa_guard import CSRC, _kernels


@pytest.fixture(scope="module")
def kernels():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return _kernels(open(os.path.join(CSRC, "_obj", "fa2_decode.s")).read())


def test_split_and_combine_kernels_exist_per_head_dim(kernels):
    for d in (64, 128):
        assert sum(f"fa2_decode_split_kernelILi{d}E" in n for n in kernels) == 1, sorted(kernels)
        assert sum(f"fa2_decode_combine_kernelILi{d}E" in n for n in kernels) == 1, sorted(kernels)


def test_no_scratch_no_spill(kernels):
    assert kernels
    for name, k in kernels.items():
        assert k["meta"]["scratch"] == 0 and k["meta"]["vgpr_spill"] == 0, (name, k["meta"])


def test_split_kernels_use_the_bf16_mfma(kernels):
    for name, k in kernels.items():
        if "split_kernel" in name:
            assert any("v_mfma_f32_32x32x16_bf16" in l for l in k["body"]), name
