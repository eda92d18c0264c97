"""Compare two -Rpass-analysis=kernel-resource-usage logs of mfx_wavefront.hip (two commits' builds):
per kernel instance VGPRs, AGPRs, scratch, LDS, occupancy and SGPRs, the instances that differ and the
ones only one log has. Instances are matched by demangled name; a trailing template argument that a
commit added with the default `false` (k_extend / k_shadow / k_camera LIST) is dropped, and
k_resolve<false / true> is k_resolve<0 / 1> (bool FRAMES became int MODE).

With --strip-false every trailing `false` template argument is dropped on both sides, which matches instances
across commits that added parameters defaulting to false (k_shadow ML and TX, k_resolve ML and TX, k_aov TX,
k_extend / k_camera / k_resolve ENV, k_shadow / k_resolve SKY, k_extend / k_aov LENS).

Usage: python scripts/resource_diff.py OLD.log NEW.log [--markdown] [--strip-false]"""
import re
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "TotalSGPRs"]
NARGS = {"k_extend": 5, "k_shadow": 5, "k_camera": 1}  # template arguments before the added one


def normalise(name):
    name = name.replace("(WfParams)", "").replace("(AovParams)", "").replace("void ", "")
    m = re.match(r"(\w+)<(.*)>$", name)
    if not m:
        return name
    fn, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    if fn == "k_resolve" and "--strip-false" not in sys.argv:
        args = [{"false": "0", "true": "1"}.get(a, a) for a in args]
    if fn in NARGS and len(args) == NARGS[fn] + 1 and args[-1] == "false":
        args = args[:-1]
    if "--strip-false" in sys.argv:  # any number of trailing `false` arguments (parameters added with that default)
        while args and args[-1] == "false":
            args = args[:-1]
    return f"{fn}<{', '.join(args)}>"


def parse(path):
    raw, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = raw.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = sorted(raw)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {normalise(d): raw[n] for n, d in zip(names, dem)}


def main():
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    md = "--markdown" in sys.argv
    shared = sorted(set(old) & set(new))
    same = 0
    for n in shared:
        d = [k for k in KEYS if old[n].get(k) != new[n].get(k)]
        if not d:
            same += 1
        else:
            hard = [k for k in d if k != "TotalSGPRs"]
            print("DIFF " if hard else "sgpr ", n, {k: (old[n].get(k), new[n].get(k)) for k in d})
    for n in sorted(set(new) - set(old)):
        print("new  ", n, [new[n].get(k) for k in KEYS])
    for n in sorted(set(old) - set(new)):
        print("gone ", n)
    print(f"{same} of {len(shared)} shared instances identical in {', '.join(KEYS)}")
    if md:
        print("\n| kernel instance | VGPRs | AGPRs | scratch B/lane | LDS B/block | waves/SIMD | SGPRs |\n|---|---|---|---|---|---|---|")
        for n in shared:
            o, w = old[n], new[n]
            print(f"| `{n}` | " + " | ".join(
                (o.get(k, "?") if o.get(k) == w.get(k) else f"{o.get(k)} -> {w.get(k)}") for k in KEYS) + " |")


if __name__ == "__main__":
    main()
