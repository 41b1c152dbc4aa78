#!/usr/bin/env python3
"""Compare the kernels of two `hipcc -S` outputs of one unit (make asm-<unit> of two commits): every kernel symbol's
instruction stream after dropping comments, directives and local label numbers. Kernels of the first file are reported
IDENTICAL or DIFFERENT with both instruction counts, kernels only the second file has are listed with theirs.

    python tools/isa_compare.py parent.s new.s > profiles/rNN/isa_parent_vs_new.log

Exits 1 when a kernel of the first file differs or is missing."""
import re
import sys


def kernels(path):
    """{symbol: [instruction, ...]} in file order, for the symbols declared .amdhsa_kernel."""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    out = {}
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.M | re.S)
        body = []
        for line in m.group(1).splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", line))
        out[name] = body
    return out


def main(parent, new):
    a, b = kernels(parent), kernels(new)
    print("# kernel, instructions in the first file, in the second")
    bad = 0
    for name, body in a.items():
        if name not in b:
            print(name, len(body), "MISSING")
            bad += 1
        else:
            same = body == b[name]
            bad += not same
            print(name, len(body), len(b[name]), "IDENTICAL" if same else "DIFFERENT")
    print("# New kernels:")
    for name, body in b.items():
        if name not in a:
            print(name, len(body))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
