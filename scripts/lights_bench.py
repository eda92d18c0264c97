#!/usr/bin/env python3
"""What several lights cost: the C2 workload (spot.xml, 1920x1080, 64 spp per step) with its one light,
with that light cut into 4 strips and into 16 (the same surface and the same ray counts; not the same image:
NewAreaLight.L carries the light's area, so N strips sum to 1 / N of the whole light). Prints one JSON
line: per variant the ms per step (median of --steps after --warmup), the k_shadow and closest-hit device
time of the last step (mfx_trace_timing: shadow_ms, closest_ms), what is left of that trace's device time
(resolve_rest_ms: k_resolve, the state memsets and the launches' gaps; the stage events do not time
k_resolve alone), and mfx_light_info. Usage: scripts/lights_bench.py [--steps 5] [--warmup 1] [--spp 64] [--width 1920 --height 1080]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mafrixraytracing_amd.lights import strips  # noqa: E402
from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext  # noqa: E402
from mafrixraytracing_amd.scene_io import load_scene_file  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "spot.xml"))
    args = ap.parse_args()
    a = load_scene_file(args.scene).with_film(args.width, args.height)
    out = {"scene": os.path.basename(args.scene), "width": args.width, "height": args.height, "spp": args.spp,
           "steps": args.steps, "variants": {}}
    for name, lights in (("one", None), ("strips4", strips(a.light, 4)), ("strips16", strips(a.light, 16))):
        with NativeContext(a, seed=DEFAULT_SEED, lights=lights) as ctx:
            ms, dev = [], []
            for k in range(args.warmup + args.steps):
                ctx.accum_clear()
                ctx.sync()
                t0 = time.perf_counter()
                ctx.trace_accumulate(args.spp, 0)
                ctx.sync()
                if k >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
                    dev.append(ctx.last_trace_ms())
            tt = ctx.trace_timing()
            counts = ctx.ray_counts()
            mean = ctx.accum_read_mean(float(args.spp))
            out["variants"][name] = {
                "ms_per_step": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                "device_ms": statistics.median(dev),
                "timing": {k: (float(v) if not isinstance(v, int) else v) for k, v in tt.items()},
                # what the stage events leave of the trace: k_resolve, the state memsets and the launches' gaps
                "shadow_ms": float(tt["shadow_ms"]), "closest_ms": float(tt["extend_ms"]),
                "resolve_rest_ms": float(tt["total_ms"] - tt["extend_ms"] - tt["shadow_ms"]),
                "rays": [float(x) for x in counts[:3]],
                "mean_luminance": float(((mean[:, 0] + mean[:, 1]) + mean[:, 2]).mean()),
                "light_info": [float(x) for x in ctx.light_info()]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
