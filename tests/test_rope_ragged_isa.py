"""CPU: the kernels of fa2_rope_append_ragged.hip as the compiler left them (`make asm`, the shipped flags): one kernel per
(head_dim, cache dtype, contiguous | paged, pair form), no scratch memory, no spilled register, no LDS; Q, K, V, the partner chunk
and the tables are read in 16-byte loads -- the only narrower vector loads are the plan's pairs, the lengths and a row's
block-table entry --; the caches are written in 16-byte (bf16) or 8-byte (e4m3) stores and Q_out in 16-byte stores; and in the
bf16-cache kernels there is NO fused multiply-add at all: those kernels hold no division, so any FMA would be a rotation the
compiler contracted (include/fa2_rope_mi355x.h, ARITHMETIC).  The e4m3 kernels' division is built from FMAs and is exempt.  A
budget check of plain compiler code, like tests/test_rope_isa.py; nothing else of the assembly is inspected."""
import os
import re
import subprocess

import pytest

from test_isa_guard import CSRC

NAME = re.compile(r"fa2_rope_append_ragged_kernelILi(\d+)ELb(\d)ELb(\d)ELb(\d)E")


@pytest.fixture(scope="module")
def kernels():
    """name -> dict(text=the kernel's instructions, meta=its metadata entry) of every kernel of fa2_rope_append_ragged.s."""
    subprocess.check_call(["make", "-s", "-j", "4", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, "_obj", "fa2_rope_append_ragged.s")).read()
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
                    want = f"fa2_rope_append_ragged_kernelILi{d}ELb{fp8}ELb{paged}ELb{pairs}E"
                    assert sum(want in n for n in kernels) == 1, sorted(kernels)


def test_no_scratch_no_spill_no_lds(kernels):
    for name, k in kernels.items():
        assert k["meta"] == dict(scratch=0, vgpr_spill=0, sgpr_spill=0, lds=0), (name, k["meta"])
        assert not _ops(k, "ds_") and not _ops(k, "scratch_"), name


def test_sixteen_byte_loads_and_whole_stores(kernels):
    for name, k in kernels.items():
        fp8 = NAME.search(name).group(2) == "1"
        # Q, K, V, the partner chunk and the tables: 16 bytes a lane; narrower only the plan's pairs (a start, or a start and its
        # q together), a length and a block-table entry
        loads = _ops(k, "global_load_")
        assert "global_load_dwordx4" in loads and set(loads) <= {"global_load_dword", "global_load_dwordx2", "global_load_dwordx4"}, (name, loads)
        # Q_out in 16-byte stores in every kernel; the caches in 16-byte (bf16) or 8-byte (e4m3) stores
        assert _ops(k, "global_store_") == (["global_store_dwordx2", "global_store_dwordx4"] if fp8 else ["global_store_dwordx4"]), name
        assert not _ops(k, "flat_") and not _ops(k, "buffer_"), name


def test_the_rotation_is_not_contracted(kernels):
    seen = 0
    for name, k in kernels.items():
        if NAME.search(name).group(2) == "1":
            continue
        seen += 1
        for op in ("v_fma_f32", "v_pk_fma_f32", "v_fmac_f32", "v_pk_fmac_f32"):
            assert not re.search(r"^\s+" + op + r"\b", k["text"], flags=re.M) and not _ops(k, op), (name, op)
        assert _ops(k, "v_pk_mul_f32") or _ops(k, "v_mul_f32"), name      # (the products are there, as products)
    assert seen == 8
