#!/usr/bin/env python3
"""Compare two device assembly files kernel by kernel (text only).

    hipcc $(FLAGS) --cuda-device-only -S -o before.s mfx_wavefront.hip    (at one commit)
    hipcc $(FLAGS) --cuda-device-only -S -o after.s mfx_wavefront.hip     (at another)
    python scripts/device_asm_diff.py before.s after.s

A kernel's text runs from its label to its .end_amdhsa_kernel: the code and the resource directives.
The order of kernels in the files is ignored; a kernel's position shows only in the function number of
its local labels (.LBB12_3, .Lfunc_end12) and in the compiler's comments, which are taken out before
comparing. Exit status 0: the same set of kernels, every one identical."""
import re
import sys


def kernels(path):
    text = open(path).read().split("\n")
    names = [m.group(1) for line in text for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)] if m]
    labels = {m.group(1): i for i, line in enumerate(text) for m in [re.match(r"(\S+):", line)] if m}
    start = {n: labels[n] for n in names}
    out = {}
    for name in names:
        i = start[name]
        j = next(k for k in range(i, len(text)) if text[k].strip() == ".end_amdhsa_kernel")
        body = "\n".join(re.sub(r"\s*;.*$", "", line) for line in text[i:j + 1])  # (comments name the number too)
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", body)
        out[name] = body
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    print(f"{sys.argv[1]}: {len(a)} kernels, {sys.argv[2]}: {len(b)} kernels")
    for what, names in (("only in the first", only_a), ("only in the second", only_b), ("different", differ)):
        for n in names:
            print(f"{what}: {n}")
    if only_a or only_b or differ:
        return 1
    print("all identical")
    return 0


if __name__ == "__main__":
    sys.exit(main())
