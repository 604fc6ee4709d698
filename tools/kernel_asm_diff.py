#!/usr/bin/env python3
"""Compare the instruction streams of the kernels two builds of one .hip file share.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off \
          --cuda-device-only -S gs_multi.hip -o new.s        # and the same at the parent
    tools/kernel_asm_diff.py parent.s new.s

Labels, directives and comments are stripped, branch targets are renumbered in order of
first use, and every kernel (a .amdhsa_kernel name) present in both files is compared
instruction by instruction.  Exit status 1 when one differs.  Needs no GPU."""
import re
import sys


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


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) & set(b)):
        same = a[name] == b[name]
        bad += not same
        print(f"{name}: {len(a[name])} / {len(b[name])} instructions, "
              f"{'identical' if same else 'DIFFERENT'}")
    for name in sorted(set(b) - set(a)):
        print(f"{name}: new, {len(b[name])} instructions")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
