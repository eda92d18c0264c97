#!/usr/bin/env python3
"""What sampling the sky buys and costs: the C2 workload (spot.xml, 1920x1080) under a 512 x 512 map with a
one-texel sun, the sky unsampled (mfx_set_environment) against sampled (mfx_set_environment_sampled). The two
contexts take three 64-spp steps each in turn, timed by device time (mfx_last_trace_ms: HIP events around the
trace's kernels). Then the noise: the RMSE of each variant's 8-spp and 64-spp images against a 4096-spp sampled
image traced on other sample indices. The sampled sky lights vertices 0 .. max_depth and the unsampled one
0 .. max_depth - 1, so the unsampled images keep a small bias against the reference that no sample count removes;
it is reported as the RMSE of a 4096-spp unsampled image's film mean (`bias_of_the_means`). Prints one JSON line.
Usage: scripts/sky_sampling_bench.py [--rounds 3] [--spp 64] [--size 512] [--ref-spp 4096]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mafrixraytracing_amd.environment import sun_map  # noqa: E402
from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext  # noqa: E402
from mafrixraytracing_amd.scene_io import load_scene_file  # noqa: E402

REF_BASE = 1 << 20  # the reference image's first sample index: disjoint from the measured images'


def step(ctx, spp, base=0, clear=True):
    if clear:
        ctx.accum_clear()
    ctx.trace_accumulate(spp, base)
    ctx.sync()
    return ctx.last_trace_ms()


def image(ctx, spp, base=0, chunk=64):
    ctx.accum_clear()
    for k in range(0, spp, chunk):
        step(ctx, min(chunk, spp - k), base + k, clear=False)
    return ctx.accum_read_mean(float(spp))[:, :3].copy()


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "spot.xml"))
    args = ap.parse_args()
    a = load_scene_file(args.scene).with_film(args.width, args.height)
    s = args.size
    # the sun: one texel of the upper hemisphere (a = 0.19, b = -0.19 of the octahedral square), about 1e-5 of the sphere
    sun_texel = (s * 13 // 32) * s + s * 19 // 32
    sky = sun_map(s, sun_texel, (60000.0, 54000.0, 42000.0), (0.25, 0.35, 0.5))
    out = {"scene": os.path.basename(args.scene), "width": args.width, "height": args.height, "spp": args.spp,
           "rounds": args.rounds, "map": [s, s], "sun_texel": sun_texel, "variants": {}}
    with NativeContext(a, seed=DEFAULT_SEED, environment=sky) as plain, \
            NativeContext(a, seed=DEFAULT_SEED, environment=sky, sample_sky=True) as smp:
        ctxs = (("unsampled", plain), ("sampled", smp))
        ms = {name: [] for name, _ in ctxs}
        for name, c in ctxs:
            for _ in range(args.warmup):
                step(c, args.spp)
        for _ in range(args.rounds):  # alternating: a drift of the device's clocks meets both alike
            for name, c in ctxs:
                ms[name].append(step(c, args.spp))
        for name, c in ctxs:
            tt = c.trace_timing()
            out["variants"][name] = {
                "device_ms": ms[name], "device_ms_median": statistics.median(ms[name]),
                "shadow_ms": float(tt["shadow_ms"]), "closest_ms": float(tt["extend_ms"]), "camera_ms": float(tt["camera_ms"]),
                "resolve_rest_ms": float(tt["total_ms"] - tt["extend_ms"] - tt["shadow_ms"]),
                "rays": [float(x) for x in c.ray_counts()[:3]],
                "pool_bytes_per_slot_added": float(c.environment_info()[3] + c.sky_sampling_info()[3]),
                "sky_sampling_info": [float(x) for x in c.sky_sampling_info()]}
        ref = image(smp, args.ref_spp, REF_BASE)
        for name, c in ctxs:
            v = out["variants"][name]
            v["rmse_8spp"] = rmse(image(c, 8), ref)
            v["rmse_64spp"] = rmse(image(c, 64), ref)
        far = image(plain, args.ref_spp, REF_BASE)
        out["bias_of_the_means"] = rmse(far.mean(axis=0), ref.mean(axis=0))
        out["unsampled_ref_rmse"] = rmse(far, ref)
    u, t = out["variants"]["unsampled"], out["variants"]["sampled"]
    out["sampled_over_unsampled_ms"] = t["device_ms_median"] / u["device_ms_median"]
    out["rmse_ratio_8spp"] = u["rmse_8spp"] / t["rmse_8spp"]
    out["rmse_ratio_64spp"] = u["rmse_64spp"] / t["rmse_64spp"]
    out["blocks_per_cu"] = {"k_shadow": t["sky_sampling_info"][4], "k_resolve": t["sky_sampling_info"][5]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
