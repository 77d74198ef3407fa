#!/usr/bin/env python3
"""Are two builds of the kernels the same code?  Compares the device assembly (`make -C cuda_flashattention_amd/csrc asm`
writes _obj/*.s) of two trees after dropping what carries no code: comment-only lines, trailing `; ...` comments, trailing
blanks and empty lines.  Labels, directives and the .amdhsa / metadata blocks are kept, so a changed register count or
descriptor field shows like a changed instruction.  The one symbol hipcc derives from the source file's PATH
(__hip_cuid_<hash>) is reduced to its prefix: it differs between any two checkouts.

    python3 tools/asm_identity.py OLD/_obj NEW/_obj      one line per .s file: equal, or the first differing lines
    python3 tools/asm_identity.py --kernels OLD/_obj/x.s NEW/_obj/x.s      one line per kernel of a file that gained a kernel

The acceptance check of a refactor of the hand-written glue around the generated bodies: a clobber list or an operand type that
differs "harmlessly" moves hipcc's prologue, and in kernels with 32 - 64 compiler registers that can end in a spill."""
import glob
import os
import re
import sys

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def normalised(path):
    out = []
    for line in open(path, errors="replace"):
        if '"' not in line:                    # (strings -- .asciz, metadata -- may hold a ';')
            line = line.split(";", 1)[0]
        line = CUID.sub("__hip_cuid_", line.rstrip())
        if line and not line.lstrip().startswith("//"):
            out.append(line)
    return out


def main(old, new, show=3):
    names = sorted({os.path.basename(p) for d in (old, new) for p in glob.glob(os.path.join(d, "*.s"))})
    differing = 0
    for name in names:
        a, b = os.path.join(old, name), os.path.join(new, name)
        if not (os.path.exists(a) and os.path.exists(b)):
            print(f"{name}: only in {old if os.path.exists(a) else new}")
            differing += 1
            continue
        x, y = normalised(a), normalised(b)
        if x == y:
            print(f"{name}: equal ({len(x)} lines)")
            continue
        differing += 1
        ndiff = sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y))
        first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print(f"{name}: DIFFERS ({len(x)} / {len(y)} lines, {ndiff} differ in place), first at normalised line {first + 1}:")
        for i in range(first, first + show):
            print(f"    - {x[i] if i < len(x) else '<end>'}\n    + {y[i] if i < len(y) else '<end>'}")
    if not names:
        sys.exit("no .s files in either directory")
    return 1 if differing else 0


KERNEL = re.compile(r"^(_Z\w+):")


def kernel_streams(path):
    """{mangled name: (instruction lines from the kernel's label to its .Lfunc_end, its .amdhsa_ lines)} of one .s file."""
    out, name, part = {}, None, None
    for line in normalised(path):
        m = KERNEL.match(line)
        if m:
            name, part = m.group(1), "code"
            out[name] = ([], [])
        elif name and line.startswith(".Lfunc_end"):
            name = None
        elif name and line.lstrip().startswith(".amdhsa_kernel"):
            part = "desc"
        elif name and part == "code" and not line.lstrip().startswith("."):
            out[name][0].append(re.sub(r"\.LBB\d+_", ".LBB_", line))      # (block labels carry the kernel's position in the file)
        elif name and part == "desc" and line.lstrip().startswith(".amdhsa_"):
            out[name][1].append(line.strip())
    return out


def per_kernel(old, new):
    """A file that gained or lost a kernel differs as a whole; this mode compares kernel by kernel: the instruction stream, and
    which descriptor fields (.amdhsa_*) changed."""
    a, b = kernel_streams(old), kernel_streams(new)
    differing = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in {old if name in a else new}" + (f" ({len(b[name][0])} instructions)" if name in b else ""))
            continue
        same = a[name][0] == b[name][0]
        fields = [f"{x} -> {y.split()[-1]}" for x, y in zip(a[name][1], b[name][1]) if x != y]
        print(f"{name}: instructions {'equal' if same else 'DIFFER'} ({len(a[name][0])} / {len(b[name][0])})"
              + (f"; descriptor: {', '.join(fields)}" if fields else "; descriptor equal"))
        differing += not same
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--kernels":      # --kernels OLD/_obj/x.s NEW/_obj/x.s
        sys.exit(per_kernel(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
