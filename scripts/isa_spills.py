#!/usr/bin/env python3
"""Register-spill report of the trace kernels' ISA (gfx950), per kernel instance: VGPRs, scratch
bytes per lane, and the spill code inside loops — scratch loads / stores (VGPR spills) and
v_readlane / v_writelane (SGPR spills to VGPR lanes) — listed by basic block with its loop depth.
Round 4 found bounce-1 k_extend's per-lane ray counter spilled this way: a scratch load-add-store
in every refill. Compiles csrc/mfx_wavefront.hip to assembly on the host (no GPU).
Usage: scripts/isa_spills.py [--all-blocks] [--loops] [--asm FILE] [kernel-name-substring ...]
(default: the flat trace kernels)
--all-blocks lists every labelled loop block (depth, instructions, lane ops, scratch ops), not only
  those with scratch ops or 8 or more lane ops.
--loops lists every loop instead: its header, depth, the instructions of the blocks that belong to it
  directly (not to a loop nested in it), their spill lane ops and scratch ops, and what marks it: `push`
  for the per-lane node step (lds_push3's v_cmpx stores), `packet-step` for the packet node step (its
  v_readlane of the representative lane's distances, the lane in a scalar register; loops of 100
  instructions or more). A labelled block runs on through the unlabelled blocks (`; %bb.N:`) after it,
  which may belong to another loop — a leaf loop's first block is listed under the label before it by the
  block modes — so the loop a line belongs to is read from the compiler's own `in Loop: Header=` notes
  on every block, labelled or not. A spill lane op has a literal lane (v_readlane_b32 s6, v127, 11);
  the packet step's own v_readlane, whose lane is a scalar register, is not counted by --loops.
--asm FILE reads an assembly file made before (hipcc --cuda-device-only -S) instead of compiling."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mafrixraytracing_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", f"-I{ROOT}/include"]


def compile_asm():
    out = os.path.join(tempfile.mkdtemp(), "wf.s")
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "--cuda-device-only", "-S", "-o", out,
                    os.path.join(SRC, "mfx_wavefront.hip")], check=True, capture_output=True)
    return open(out).read()


def kernels(asm):
    for m in re.finditer(r"^(_Z\w+):", asm, re.M):
        name = m.group(1)
        end = asm.index("s_endpgm", m.end())
        meta = re.search(r"; NumVgprs: (\d+)", asm[end:end + 4000])
        scr = re.search(r"; ScratchSize: (\d+)", asm[end:end + 4000])
        yield name, asm[m.end():end], (meta.group(1) if meta else "?"), (scr.group(1) if scr else "?")


def blocks(body):
    cur = ["entry", "", []]
    out = [cur]
    for line in body.split("\n"):
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", line)
        if m:
            cur = [m.group(1), m.group(2), []]
            out.append(cur)
            continue
        t = line.strip()
        if line.startswith("\t") and t and not t.startswith((".", ";")):
            cur[2].append(t.split()[0])
    return out


SPILL_LANE = re.compile(r"^v_(readlane|writelane)_b32 \S+ \S+ \d+$")


def loops(body):
    """{header: [depth, parent, instructions, spill lane ops, scratch ops, marks]} in order of appearance"""
    out = {}
    cur = None
    label = None
    pending = False
    for line in body.split("\n"):
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)", line)
        if m:
            label, cur, pending = m.group(1), None, True
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", m.group(2))
            if h:
                cur = h.group(1)
                out.setdefault(cur, [int(h.group(2)), None, 0, 0, 0, set()])
            line = m.group(2)
        t = line.strip()
        if pending and t.startswith(";"):
            h = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", t)
            p = re.search(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", t)
            if h and label:
                cur = label
                out.setdefault(cur, [0, None, 0, 0, 0, set()])[0] = int(h.group(1))
            if p and label:  # the innermost parent is the last one named
                out.setdefault(label, [0, None, 0, 0, 0, set()])[1] = p.group(1)
            continue
        if line.startswith("\t") and t and not t.startswith((".", ";")):
            pending = False
            if cur is None:
                continue
            e = out[cur]
            e[2] += 1
            text = " ".join(t.replace(",", " ").split())
            if SPILL_LANE.match(text):
                e[3] += 1
            if t.startswith("scratch_"):
                e[4] += 1
            if t.startswith("v_cmpx_lt_u32"):
                e[5].add("push")
            if re.match(r"v_readlane_b32 \S+ \S+ s\d+$", text):
                e[5].add("packet-step")
    return out


def main():
    argv = sys.argv[1:]
    asm_file = None
    if "--asm" in argv:
        i = argv.index("--asm")
        asm_file = argv[i + 1]
        del argv[i:i + 2]
    args = [a for a in argv if a not in ("--all-blocks", "--loops")]
    every = "--all-blocks" in argv
    by_loop = "--loops" in argv
    want = args or ["k_extendILb0ELb0ELi0ELb0E", "k_extendILb0ELb0ELi0ELb1E", "k_shadowILb0ELb1ELi4ELi0ELb0E",
                    "k_shadowILb0ELb1ELi4ELi0ELb1E", "k_cameraILb0E"]
    asm = open(asm_file).read() if asm_file else compile_asm()
    for name, body, vgpr, scratch in kernels(asm):
        if not any(w in name for w in want):
            continue
        bl = blocks(body)
        ins = sum(len(b[2]) for b in bl)
        rl = sum(b[2].count("v_readlane_b32") for b in bl)
        wl = sum(b[2].count("v_writelane_b32") for b in bl)
        print(f"{name}: {ins} instructions, VGPRs {vgpr}, scratch {scratch} B/lane, v_readlane {rl}, v_writelane {wl}")
        if by_loop:
            for h, (depth, parent, n, lane, sc, marks) in loops(body).items():
                if n < 100:
                    marks.discard("packet-step")  # (a short readlane loop of the window scan)
                print(f"  loop {h:>10} depth {depth} (in {parent or '-':>10}): {n:4d} instr, spill lane ops {lane:3d}, "
                      f"scratch ops {sc}{'  [' + ', '.join(sorted(marks)) + ']' if marks else ''}")
            continue
        for lab, comment, ops in bl:
            d = re.search(r"Depth=(\d+)", comment)
            if not d:
                continue
            sc = sum(1 for o in ops if o.startswith("scratch_"))
            r = ops.count("v_readlane_b32") + ops.count("v_writelane_b32")
            if every or sc or r >= 8:
                print(f"  {lab:>12} loop depth {d.group(1)}: {len(ops):4d} instr, scratch ops {sc}, SGPR spill lane ops {r}")


if __name__ == "__main__":
    main()
