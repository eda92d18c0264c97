#!/usr/bin/env python3
"""What a sky costs: the C2 workload (spot.xml, 1920x1080, 64 spp per step) without an environment against the
same scene under a 256 x 256 gradient map (mfx_set_environment). The two contexts take their steps in turn,
--rounds rounds of --steps steps each, timed by device time (mfx_last_trace_ms: HIP events around the
trace's kernels). The ray counts must be equal: the sky adds no ray and no draw. Prints one JSON line: per
variant the device ms of every step and their median, the k_shadow and closest-hit device time of the last
step, what is left of it (k_resolve, the memsets, the gaps), and mfx_environment_info (the pool bytes per slot
and the resident blocks per CU of k_extend and k_resolve among it).
Usage: scripts/environment_bench.py [--rounds 3] [--steps 1] [--warmup 1] [--spp 64] [--size 256]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mafrixraytracing_amd.environment import gradient  # noqa: E402
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
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "spot.xml"))
    args = ap.parse_args()
    a = load_scene_file(args.scene).with_film(args.width, args.height)
    sky = gradient(args.size, (0.25, 0.45, 1.0), (0.9, 0.9, 0.85), (0.15, 0.12, 0.1))
    out = {"scene": os.path.basename(args.scene), "width": args.width, "height": args.height, "spp": args.spp,
           "rounds": args.rounds, "steps": args.steps, "map": [args.size, args.size], "variants": {}}
    with NativeContext(a, seed=DEFAULT_SEED) as plain, NativeContext(a, seed=DEFAULT_SEED, environment=sky) as lit:
        ctxs = (("no_environment", plain), ("environment", lit))
        ms = {name: [] for name, _ in ctxs}
        for name, c in ctxs:
            for _ in range(args.warmup):
                step(c, args.spp)
        for _ in range(args.rounds):  # alternating: a drift of the device's clocks meets both alike
            for name, c in ctxs:
                for _ in range(args.steps):
                    ms[name].append(step(c, args.spp))
        for name, c in ctxs:
            tt = c.trace_timing()
            mean = c.accum_read_mean(float(args.spp))
            out["variants"][name] = {
                "device_ms": ms[name], "device_ms_median": statistics.median(ms[name]),
                "shadow_ms": float(tt["shadow_ms"]), "closest_ms": float(tt["extend_ms"]), "camera_ms": float(tt["camera_ms"]),
                "resolve_rest_ms": float(tt["total_ms"] - tt["extend_ms"] - tt["shadow_ms"]),
                "rays": [float(x) for x in c.ray_counts()[:3]],
                "mean_luminance": float(((mean[:, 0] + mean[:, 1]) + mean[:, 2]).mean()),
                "environment_info": [float(x) for x in c.environment_info()]}
    u, t = out["variants"]["no_environment"], out["variants"]["environment"]
    if u["rays"] != t["rays"]:
        raise SystemExit(f"ray counts differ: {u['rays']} vs {t['rays']}")
    out["environment_over_none"] = t["device_ms_median"] / u["device_ms_median"]
    out["added_pool_bytes_per_slot"] = t["environment_info"][3]
    out["blocks_per_cu"] = {"k_extend": t["environment_info"][4], "k_resolve": t["environment_info"][5]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
