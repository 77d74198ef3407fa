"""CPU: the fp8-cache decode kernels of fa2_decode.hip as the compiler left them (`make asm`, the shipped flags): one
fa2_decode_f8_split_kernel and one fa2_decode_f8_paged_split_kernel per head dim, no scratch memory, no spilled VGPR, and the bodies
do run v_mfma_f32_32x32x16_bf16 (the caches are widened to bf16 in registers; both products stay the bf16 ones).  Nothing else of
the assembly is inspected, as in tests/test_decode_isa.py."""
import os
import subprocess

import pytest

from test_isa_guard import CSRC, _kernels

NEW = ("fa2_decode_f8_split_kernel", "fa2_decode_f8_paged_split_kernel")


@pytest.fixture(scope="module")
def kernels():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    every = _kernels(open(os.path.join(CSRC, "_obj", "fa2_decode.s")).read())
    return {n: k for n, k in every.items() if any(f"{name}ILi" in n for name in NEW)}


def test_each_kernel_exists_once_per_head_dim(kernels):
    for name in NEW:
        for d in (64, 128):
            assert sum(f"{name}ILi{d}E" in n for n in kernels) == 1, sorted(kernels)
    assert len(kernels) == 4, sorted(kernels)


def test_no_scratch_no_spill(kernels):
    assert kernels
    for name, k in kernels.items():
        assert k["meta"]["scratch"] == 0 and k["meta"]["vgpr_spill"] == 0, (name, k["meta"])


def test_the_bodies_use_the_bf16_mfma(kernels):
    assert kernels
    for name, k in kernels.items():
        assert any("v_mfma_f32_32x32x16_bf16" in l for l in k["body"]), name
