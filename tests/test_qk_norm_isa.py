"""CPU: the kernels of fa2_norm_rope_append_ragged.hip as the compiler left them (`make asm`, the shipped flags): one kernel per
(head_dim, cache dtype, contiguous | paged, pair form), no scratch memory, no spilled register, a group segment of ZERO bytes (the
butterfly's lane permutes go through the LDS crossbar but allocate none); Q, K, V, the partner chunk, the tables and the weights
are read in 16-byte loads -- the only narrower vector loads are the plan's pairs, the lengths and a row's block-table entry --;
the caches are written in 16-byte (bf16) or 8-byte (e4m3) stores and Q_out in 16-byte stores.  A budget check of plain compiler
code, like tests/test_rope_ragged_isa.py; nothing else of the assembly is inspected.  In particular there is no ban on fused
multiply-adds here: the norm's division and square root are built from them in every kernel, and that the products and sums of
the norm and of the rotation are NOT contracted is what the zero tolerance of tests/test_gpu_qk_norm.py shows."""
import os
import re
import subprocess

import pytest

from test_isa_guard import CSRC

NAME = re.compile(r"fa2_norm_rope_append_ragged_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)E")


@pytest.fixture(scope="module")
def kernels():
    """name -> dict(text=the kernel's instructions, meta=its metadata entry) of every kernel of fa2_norm_rope_append_ragged.s."""
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, "_obj", "fa2_norm_rope_append_ragged.s")).read()
    ks = {m.group(1): {"text": m.group(2)} for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)\n\.Lfunc_end", text, flags=re.S | re.M)}
    for m in re.finditer(r"- \.agpr_count:\s+\d+(.*?)\.wavefront_size", text, flags=re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(1)).group(1)
        g = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", m.group(1)).group(1))
        ks[name]["meta"] = dict(scratch=g("private_segment_fixed_size"), vgpr_spill=g("vgpr_spill_count"),
                                sgpr_spill=g("sgpr_spill_count"), lds=g("group_segment_fixed_size"))
    return ks


def _ops(k, prefix):
    return sorted(set(re.findall(r"^\s+(" + prefix + r"\w+)", k["text"], flags=re.M)))


def test_one_kernel_per_variant(kernels):
    assert len(kernels) == 16, sorted(kernels)
    for d in (64, 128):
        for fp8 in (0, 1):
            for paged in (0, 1):
                for pairs in (0, 1):
                    want = f"fa2_norm_rope_append_ragged_kernelILi{d}ELb{fp8}ELb{paged}ELb{pairs}E"
                    assert sum(want in n for n in kernels) == 1, sorted(kernels)


def test_no_scratch_no_spill_no_group_segment(kernels):
    for name, k in kernels.items():
        assert k["meta"] == dict(scratch=0, vgpr_spill=0, sgpr_spill=0, lds=0), (name, k["meta"])
        assert not _ops(k, "scratch_"), name
        # however the compiler moves the butterfly's values between lanes, nothing is read from or written to LDS
        assert not _ops(k, "ds_read") and not _ops(k, "ds_write"), (name, _ops(k, "ds_"))


def test_sixteen_byte_loads_and_whole_stores(kernels):
    for name, k in kernels.items():
        fp8 = NAME.search(name).group(2) == "1"
        loads = _ops(k, "global_load_")
        assert "global_load_dwordx4" in loads and set(loads) <= {"global_load_dword", "global_load_dwordx2", "global_load_dwordx4"}, (name, loads)
        assert _ops(k, "global_store_") == (["global_store_dwordx2", "global_store_dwordx4"] if fp8 else ["global_store_dwordx4"]), name
        assert not _ops(k, "flat_") and not _ops(k, "buffer_"), name
