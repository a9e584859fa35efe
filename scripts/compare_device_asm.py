#!/usr/bin/env python3
"""Do two device-side assembly files of engine.hip hold the same kernels?  The check of a host-only refactor:

    cd meshanything_amd/csrc
    hipcc --offload-arch=gfx950 -O3 -DNDEBUG -std=c++17 -fPIC -fvisibility=hidden -S --cuda-device-only '-DMA_SRC_HASH="x"' [-DMA_EXPERIMENTAL=1] engine.hip -o X.s
    python scripts/compare_device_asm.py before.s after.s

Compared per kernel symbol: the instruction text between `<symbol>:` and its `.Lfunc_end<n>:`, and the `.amdhsa_kernel` descriptor (registers, LDS,
scratch).  Two normalisations, because moving host code reorders the kernel instantiations in the file: assembly comments are dropped, and the
compiler's local labels (.LBB<n>_<m>, .Lfunc_end<n>, .LJTI<n>_<m>) lose the function number n.  Exit status 0 when everything is equal."""
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|LJTI)\d+(_\d+)?")


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    return LABEL.sub(lambda m: "." + m.group(1) + (m.group(2) or ""), line)


def kernels(path):
    lines = open(path).read().split("\n")
    desc, body = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = [norm(x) for x in lines[i + 1:j] if norm(x)]
            i = j
        i += 1
    at = {x.split(":", 1)[0]: n for n, x in enumerate(lines) if x[:1] not in ("", "\t", " ", ".") and ":" in x}      # symbol -> line of `<symbol>:`
    for name in desc:
        start = at[name]
        j = start + 1
        while not lines[j].startswith(".Lfunc_end"):
            j += 1
        body[name] = [norm(x) for x in lines[start + 1:j] if norm(x)]
    return desc, body


def main(a, b):
    (da, ba), (db, bb) = kernels(a), kernels(b)
    only = sorted(set(da) ^ set(db))
    bad_body = sorted(k for k in set(da) & set(db) if ba[k] != bb[k])
    bad_desc = sorted(k for k in set(da) & set(db) if da[k] != db[k])
    for k in only:
        print("only in", a if k in da else b, ":", k)
    for k in bad_body:
        print("body differs:", k)
    for k in bad_desc:
        print("descriptor differs:", k)
    same = not (only or bad_body or bad_desc)
    print(f"{len(da)} vs {len(db)} kernels: {len(set(da) & set(db)) - len(bad_body)} bodies and {len(set(da) & set(db)) - len(bad_desc)} descriptors equal, "
          f"{len(only)} symbols on one side only -> {'SAME device code' if same else 'DIFFERENT'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
