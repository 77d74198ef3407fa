"""CPU: the guard of tests/test_isa_guard.py over the kernels of the packed variable-length calls (`make asm`, the shipped flags).

They are the dense kernels' code behind another front end -- (head, block) and the sequence's view come from a table instead of
blockIdx.x -- so what holds for the dense instances must hold for them: the accumulator file and the bodies' registers are touched
by the asm bodies only, nothing spills, and they hold exactly their dense siblings' MFMAs and vector loads (the table is read
through scalar loads: a vector load of it would show up in the count, and its values would not be wave-uniform for the buffer
resources and the branches around the tile barriers)."""
import os
import re
import subprocess

import pytest

from test_isa_guard import CSRC, _kernels, _split_asm

VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
# (file, the packed kernel, its dense sibling, hipcc's own VGPRs, registers in all) per head_dim and mask
FAMILIES = [
    ("fa2_fwd1_bf16", "fa2_fwd1_varlen_kernelILi128ELb{c}E", "fa2_fwd1_bf16_kernelILi128ELb{c}ELb0E", 64, 512),
    ("fa2_fwd1_bf16", "fa2_fwd1x2_varlen_kernelILi64ELb{c}E", "fa2_fwd1x2_bf16_kernelILi64ELb{c}ELb0E", 40, 256),
    ("fa2_bwd_bf16", "fa2_bwd_dq_varlen_kernelILi128ELb{c}E", "fa2_bwd_dq_kernelILi128ELb{c}E", 64, 512),
    ("fa2_bwd_bf16", "fa2_bwd_dq_varlen_kernelILi64ELb{c}E", "fa2_bwd_dq_kernelILi64ELb{c}E", 64, 512),
    ("fa2_bwd_bf16", "fa2_bwd_dkdv_varlen_kernelILi128ELb{c}E", "fa2_bwd_dkdv_kernelILi128ELb{c}E", 60, 512),
    ("fa2_bwd_bf16", "fa2_bwd_dkdv_varlen_kernelILi64ELb{c}E", "fa2_bwd_dkdv_kernelILi64ELb{c}E", 60, 512),
]


@pytest.fixture(scope="module")
def asm():
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return {f: _kernels(open(os.path.join(CSRC, "_obj", f + ".s")).read()) for f in ("fa2_fwd1_bf16", "fa2_bwd_bf16")}


def _one(ks, pattern):
    hits = [n for n in ks if pattern in n]
    assert len(hits) == 1, (pattern, hits)
    return ks[hits[0]]


def test_each_packed_kernel_exists_once_per_head_dim_and_mask(asm):
    assert sum("varlen_kernel" in n for n in asm["fa2_fwd1_bf16"]) == 4          # d = 128 one wave per SIMD, d = 64 two; x causal
    assert sum("varlen_kernel" in n for n in asm["fa2_bwd_bf16"]) == 8           # dQ and dK/dV x head_dim x causal


@pytest.mark.parametrize("file,packed,dense,own,total", FAMILIES)
@pytest.mark.parametrize("causal", [0, 1])
def test_packed_kernel_is_its_dense_sibling_behind_a_table(asm, file, packed, dense, own, total, causal):
    k, sib = _one(asm[file], packed.format(c=causal)), _one(asm[file], dense.format(c=causal))
    assert k["meta"]["scratch"] == 0 and k["meta"]["vgpr_spill"] == 0, k["meta"]
    assert k["meta"]["total"] == total and k["meta"]["agpr"] == sib["meta"]["agpr"], k["meta"]
    outside, blocks = _split_asm(k["body"])
    hits = [s for s in outside if re.search(r"v_accvgpr|\ba\[\d+|\ba\d+\b", s)]
    assert not hits, hits[:5]
    for s in outside:
        for m in VREG.finditer(s):
            assert int(m.group(1) or m.group(3)) < own, s
    count = lambda kk, what: sum(what in l for l in kk["body"])
    assert count(k, "v_mfma_f32_32x32x16_bf16") == count(sib, "v_mfma_f32_32x32x16_bf16") > 0
    sib_outside = _split_asm(sib["body"])[0]
    for op in ("global_load", "buffer_load", "flat_load"):
        assert sum(s.startswith(op) for s in outside) == sum(s.startswith(op) for s in sib_outside), op
    assert sum(s.startswith("s_load") for s in outside) > sum(s.startswith("s_load") for s in sib_outside)      # the item
