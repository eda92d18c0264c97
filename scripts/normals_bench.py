#!/usr/bin/env python3
"""What smooth shading costs: the C2 workload (spot.xml, 1920x1080), a 64-spp step and mfx_aov(4) with corner normals
on every primitive (mfx_set_normals with normals.smooth_normals of the scene) against without. The two contexts take
their steps in turn, timed by device time (mfx_last_trace_ms: HIP events around the trace's kernels; mfx_aov's own
events), with the per-kernel split of the last step (mfx_trace_timing). Only k_shadow and k_aov differ between the
two: the SN twins gather a flag and a 96-B record per vertex on a smooth primitive. Prints one JSON line.
Usage: scripts/normals_bench.py [--rounds 3] [--spp 64] [--crease 60]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext  # noqa: E402
from mafrixraytracing_amd.normals import smooth_normals  # noqa: E402
from mafrixraytracing_amd.scene_io import load_scene_file  # noqa: E402


def step(ctx, spp):
    ctx.accum_clear()
    ctx.trace_accumulate(spp, 0)
    ctx.sync()
    return ctx.last_trace_ms()


def aov(ctx, spp):
    ctx.aov(spp)
    return ctx.last_aov_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--aov-spp", type=int, default=4)
    ap.add_argument("--crease", type=float, default=60.0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "spot.xml"))
    args = ap.parse_args()
    a = load_scene_file(args.scene).with_film(args.width, args.height)
    pn = smooth_normals(a.prims, args.crease)
    out = {"scene": os.path.basename(args.scene), "width": args.width, "height": args.height, "spp": args.spp,
           "aov_spp": args.aov_spp, "rounds": args.rounds, "primitives": int(len(a.prims)),
           "smooth_primitives": int((pn["smooth"] != 0).sum()), "variants": {}}
    with NativeContext(a, seed=DEFAULT_SEED) as face, NativeContext(a, seed=DEFAULT_SEED, normals=pn) as smooth:
        ctxs = (("face", face), ("smooth", smooth))
        ms = {name: [] for name, _ in ctxs}
        ams = {name: [] for name, _ in ctxs}
        for name, c in ctxs:
            for _ in range(args.warmup):
                step(c, args.spp)
                aov(c, args.aov_spp)
        for _ in range(args.rounds):  # alternating: a drift of the device's clocks meets both alike
            for name, c in ctxs:
                ms[name].append(step(c, args.spp))
        for name, c in ctxs:
            tt = c.trace_timing()
            rays = [float(x) for x in c.ray_counts()[:3]]
            med = statistics.median(ms[name])
            out["variants"][name] = {
                "device_ms": ms[name], "device_ms_median": med, "mrays_per_s": sum(rays) / med / 1e3,
                "camera_ms": float(tt["camera_ms"]), "closest_ms": float(tt["extend_ms"]), "shadow_ms": float(tt["shadow_ms"]),
                "resolve_rest_ms": float(tt["total_ms"] - tt["extend_ms"] - tt["shadow_ms"]), "rays": rays,
                "shadow_waves": c.launch_info()["shadow_waves"], "normal_info": [float(x) for x in c.normal_info()]}
        for _ in range(args.rounds):
            for name, c in ctxs:
                ams[name].append(aov(c, args.aov_spp))
        for name, _ in ctxs:
            out["variants"][name]["aov_ms"] = ams[name]
            out["variants"][name]["aov_ms_median"] = statistics.median(ams[name])
    f, s = out["variants"]["face"], out["variants"]["smooth"]
    out["smooth_over_face_ms"] = s["device_ms_median"] / f["device_ms_median"]
    out["smooth_over_face_shadow_ms"] = s["shadow_ms"] / f["shadow_ms"]
    out["smooth_over_face_aov_ms"] = s["aov_ms_median"] / f["aov_ms_median"]
    out["device_bytes_added"] = s["normal_info"][2]
    out["blocks_per_cu"] = {"k_shadow": s["normal_info"][4], "k_aov": s["normal_info"][5]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
