#!/usr/bin/env python3
"""Compare the instruction streams of the kernels two builds of one .hip file share.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off \
          --cuda-device-only -S gs_multi.hip -o new.s        # and the same at the parent
    tools/kernel_asm_diff.py parent.s new.s

    tools/kernel_asm_diff.py --resources new.s           # the kernels' resource numbers

Labels, directives and comments are stripped, branch targets are renumbered in order of
first use, and every kernel (a .amdhsa_kernel name) present in both files is compared
instruction by instruction; a kernel that differs lists the instruction index ranges
(of the first file / of the second) that do.  Exit status 1 when one differs.
--resources prints each kernel's register, spill, scratch and LDS numbers from the
code object metadata instead.  Needs no GPU."""
import difflib
import re
import sys

RESOURCES = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
             ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        m = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        if not m:
            continue
        labels, body = {}, []
        for line in m.group(1).splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            line = re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), f"L{len(labels)}"),
                          line)
            body.append(re.sub(r"\s+", " ", line))
        out[name] = body
    return out


def resources(path):
    """{kernel: {field: value}} from the amdhsa.kernels metadata."""
    out = {}
    meta = open(path).read().split("amdhsa.kernels:", 1)[1]
    for block in re.split(r"(?m)^  - ", meta)[1:]:
        name = re.search(r"(?m)^    \.name:\s+(\S+)", block)
        if not name:  # (a list of another metadata key after the kernels')
            continue
        name = name.group(1)
        out[name] = {f: int(re.search(rf"(?m)^\s+\{f}:\s+(\d+)", block).group(1)) for f in RESOURCES}
    return out


def main():
    if sys.argv[1] == "--resources":
        for name, r in sorted(resources(sys.argv[2]).items()):
            print(name, " ".join(f"{f[1:]}={r[f]}" for f in RESOURCES))
        return 0
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) & set(b)):
        same = a[name] == b[name]
        bad += not same
        print(f"{name}: {len(a[name])} / {len(b[name])} instructions, "
              f"{'identical' if same else 'DIFFERENT'}")
        if not same:
            ops = difflib.SequenceMatcher(None, a[name], b[name], autojunk=False).get_opcodes()
            print("   ", " ".join(f"{i1}-{i2}/{j1}-{j2}" for tag, i1, i2, j1, j2 in ops if tag != "equal"))
    for name in sorted(set(b) - set(a)):
        print(f"{name}: new, {len(b[name])} instructions")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
