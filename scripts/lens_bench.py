#!/usr/bin/env python3
"""What a thin lens costs: the C2 workload (spot.xml, 1920x1080), a 64-spp step with a lens (mfx_set_lens) against
without. The two contexts take their steps in turn, timed by device time (mfx_last_trace_ms: HIP events around the
trace's kernels), with the per-kernel split of the last step (mfx_trace_timing). With a lens a flat scene's camera
rays run k_extend's LENS instance, one ray per lane, instead of k_camera's packets, and no cut table is built: the
difference shows in the first iteration (`camera_ms` without, the first `extend` share with). Prints one JSON line.
Usage: scripts/lens_bench.py [--rounds 3] [--spp 64] [--aperture 0.05] [--focus 4.2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext  # noqa: E402
from mafrixraytracing_amd.scene_io import load_scene_file  # noqa: E402


def step(ctx, spp):
    ctx.accum_clear()
    ctx.trace_accumulate(spp, 0)
    ctx.sync()
    return ctx.last_trace_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--aperture", type=float, default=0.05)
    ap.add_argument("--focus", type=float, default=4.2)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "spot.xml"))
    args = ap.parse_args()
    a = load_scene_file(args.scene).with_film(args.width, args.height)
    out = {"scene": os.path.basename(args.scene), "width": args.width, "height": args.height, "spp": args.spp,
           "rounds": args.rounds, "lens": [args.aperture, args.focus], "variants": {}}
    with NativeContext(a, seed=DEFAULT_SEED) as pin, NativeContext(a, seed=DEFAULT_SEED, lens=(args.aperture, args.focus)) as lens:
        ctxs = (("pinhole", pin), ("lens", lens))
        ms = {name: [] for name, _ in ctxs}
        for name, c in ctxs:
            for _ in range(args.warmup):
                step(c, args.spp)
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
                "lens_info": [float(x) for x in c.lens_info()]}
    p, l = out["variants"]["pinhole"], out["variants"]["lens"]
    out["lens_over_pinhole_ms"] = l["device_ms_median"] / p["device_ms_median"]
    # closest_ms holds every iteration's k_extend / k_camera time, camera_ms the packets' share of it. The bounces
    # trace other rays under a lens but run the same kernels, so the lens's first iteration is about what its
    # closest_ms exceeds the pinhole's bounces by
    out["first_iteration_ms"] = {"pinhole_k_camera": p["camera_ms"],
                                 "lens_k_extend_estimate": l["closest_ms"] - (p["closest_ms"] - p["camera_ms"])}
    out["blocks_per_cu"] = {"k_extend_start": l["lens_info"][12], "k_aov": l["lens_info"][13]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
