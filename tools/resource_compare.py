#!/usr/bin/env python3
"""Compare two -Rpass-analysis=kernel-resource-usage logs (`make -C .../csrc asm 2> log`), kernel by kernel.

    tools/resource_compare.py parent.log this.log [--new-only PATTERN]

Kernel names are demangled (c++filt) and their template arguments normalised (true/false -> 1/0), so
that a flag whose type changed from bool to int still names the same instantiation. Prints every
instantiation both logs hold whose VGPRs, AGPRs, SGPRs, scratch, LDS, spills or occupancy differ, then
the figures of the instantiations only the second log holds. Exit status 1 when a shared one differs.
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for f in FIELDS:
            m = re.search(r"remark: .*\s" + re.escape(f) + r": (\d+)", line)
            if m:
                cur[f] = int(m.group(1))
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"\btrue\b", "1", re.sub(r"\bfalse\b", "0", d))
        d = re.sub(r"\((?:bool|int)\)", "", d)
        res[d] = out[n]
    return res


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for k in sorted(a):
        if k not in b:
            print("only in the first:", k)
            bad += 1
        elif a[k] != b[k]:
            print("differs:", k, a[k], b[k])
            bad += 1
    print(f"{len(a)} kernels in the first log, {len(b)} in the second, {bad} differ or left")
    for k in sorted(b):
        if k not in a:
            print("new:", k.split("(")[0], {f: b[k].get(f) for f in FIELDS})
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
