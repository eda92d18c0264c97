#!/usr/bin/env python3
"""What adaptive sampling (mfx_sample_adaptive) costs and saves on C2 (spot, 1920x1080): one JSON line.

The baseline is the uniform 64-spp step of `bench.py --config C2`, run first in a process of its own
(--baseline-lib PATH: against another build of the library, e.g. the parent commit's, through
MFX_LIB_PATH). Against it:
  a  min = max = 64: one pass over every tile. The cost of the moment resolve, the one check and the
     mean kernel (extra traffic from shapes: the two FP64 moment planes read and written once per
     generation, 32 B per pixel).
  b  min 8, step 8, max 64, rel_error 1e-12: only exactly black tiles stop; the per-pass cost.
  c  practical thresholds (--rel, default 0.2 0.1 0.05; abs_floor 0.01), each with the schedules
     min 8 / step 8 and min 16 / step 16 (max 64).
Each run reports total rays, mean spp, passes, device ms (the passes' traces and checks and the mean
kernel, from HIP events; `stages`: the closest-hit kernels, k_shadow and the rest — resolve, memsets,
check, mean) and the wall ms of a call that reads back only the tile counts; its RMSE against a
uniform --ref-spp render of the same library (other samples: sample base 2^20) next to the RMSE of a
uniform render of equal ray count (the spp whose rays come nearest)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def baseline(args):
    env = dict(os.environ)
    if args.baseline_lib:
        env["MFX_LIB_PATH"] = os.path.abspath(args.baseline_lib)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--gpus", "1", "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(f"adaptive_bench: the baseline bench.py run failed ({p.returncode})")
    d = json.loads(p.stdout.strip().splitlines()[-1])
    return {"lib": args.baseline_lib or "this build", "ms_per_step": d["ms_per_step"], "mrays_per_s": d["value"],
            "rays_per_step": d.get("rays_per_step"), "cmd": " ".join(cmd[1:])}


def stages(t):
    """mfx_trace_timing's split in ms: closest-hit kernels, k_shadow, and the rest of the device time."""
    return {"closest_ms": round(t["extend_ms"], 3), "shadow_ms": round(t["shadow_ms"], 3),
            "rest_ms": round(t["total_ms"] - t["extend_ms"] - t["shadow_ms"], 3), "launches": t["launches"],
            "generations": t["generations"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--rel", type=float, nargs="*", default=[0.2, 0.1, 0.05])
    ap.add_argument("--calls", type=int, default=3, help="timed calls per run (the fastest is reported)")
    args = ap.parse_args()
    base = baseline(args)  # before this process touches the GPU

    import numpy as np
    from mafrixraytracing_amd.abi import MfxAdaptive, iptr
    from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext
    from mafrixraytracing_amd.scene_io import load_scene_file

    a = load_scene_file(os.path.join(ROOT, "scenes", "spot.xml"))
    w, h = a.width, a.height
    npix = w * h
    ty_n, tx_n = (h + 7) // 8, (w + 7) // 8
    valid = np.minimum(8, w - 8 * np.arange(tx_n))[None, :] * np.minimum(8, h - 8 * np.arange(ty_n))[:, None]

    with NativeContext(a, seed=DEFAULT_SEED) as ctx:  # the reference: other samples than any run's
        ctx.accum_clear()
        ctx.trace_accumulate(args.ref_spp, 1 << 20)
        ref = ctx.accum_read_mean(float(args.ref_spp))[:, :3].copy()
        # this build's own uniform 64-spp trace (device ms), the figure (a) adds to
        own = []
        for k in range(args.calls + 1):
            ctx.accum_clear()
            ctx.trace_accumulate(64, 64 * k)
            ctx.sync()
            own.append((ctx.last_trace_ms(), stages(ctx.trace_timing())))
        uniform64_ms, uniform64_stages = min(own[1:], key=lambda t: t[0])

    rays_per_spp = [None]

    def rmse(img):
        return float(np.sqrt(np.mean((img[:, :3] - ref) ** 2)))

    uniform_cache = {}

    def uniform(spp):
        if spp not in uniform_cache:
            with NativeContext(a, seed=DEFAULT_SEED) as ctx:
                img = ctx.sample(spp)
                c = ctx.ray_counts()
                uniform_cache[spp] = {"spp": spp, "rays": float(c[0] + c[1] + c[2]), "rmse": rmse(img),
                                      "device_ms": ctx.last_trace_ms()}
        return uniform_cache[spp]

    def run(label, mn, mx, step, rel, floor=0.01):
        with NativeContext(a, seed=DEFAULT_SEED) as ctx:
            frame, tiles = ctx.sample_adaptive(mn, mx, step, rel, floor)  # samples from 0; allocates the pool
            c = ctx.ray_counts()
            cfg = MfxAdaptive(min_spp=mn, max_spp=mx, step_spp=step, reserved=0, rel_error=rel, abs_floor=floor)
            t = np.zeros((ty_n, tx_n), dtype=np.int32)
            dev, wall = [], []
            for _ in range(args.calls):  # later sample ranges: the same work within noise
                t0 = time.perf_counter()
                rc = ctx.lib.mfx_sample_adaptive(ctx._h, C.byref(cfg), None, iptr(t), None)
                wall.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0, ctx.lib.mfx_last_error()
                dev.append((ctx.last_trace_ms(), stages(ctx.trace_timing())))
            dev_stages = min(dev, key=lambda t: t[0])[1]
            dev = [d[0] for d in dev]
        sched = [mn]
        while sched[-1] < mx:
            sched.append(min(mx, sched[-1] + step))
        passes = sched.index(int(tiles.max())) + 1
        mean_spp = float((tiles * valid).sum() / npix)
        r = {"run": label, "min_spp": mn, "max_spp": mx, "step_spp": step, "rel_error": rel, "abs_floor": floor,
             "rays": float(c[0] + c[1] + c[2]), "mean_spp": round(mean_spp, 3), "passes": passes,
             "tiles_at_max": int((tiles == mx).sum()), "tiles": int(tiles.size),
             "device_ms": round(min(dev), 3), "wall_ms_counts_only": round(min(wall), 3),
             "device_ms_per_pass": round(min(dev) / passes, 3), "stages": dev_stages, "rmse": rmse(frame),
             "vs_baseline_ms": round(min(dev) / base["ms_per_step"], 4)}
        if rays_per_spp[0] is None:
            rays_per_spp[0] = uniform(64)["rays"] / 64
        r["uniform_equal_rays"] = uniform(max(1, int(round(r["rays"] / rays_per_spp[0]))))
        return r

    runs = [run("a", 64, 64, 8, 0.1), run("b", 8, 64, 8, 1e-12)]
    runs += [run(f"c rel {rel:g} {mn}/{mn}", mn, 64, mn, rel) for rel in args.rel for mn in (8, 16)]
    out = {"workload": f"C2 spot {w}x{h}", "baseline": base, "uniform64_trace_ms_this_build": round(uniform64_ms, 3),
           "uniform64_stages_this_build": uniform64_stages, "reference_spp": args.ref_spp, "uniform64": uniform(64),
           "moment_plane_traffic_MB_per_full_pass": round(npix * 2 * 8 * 2 / 1e6, 1), "runs": runs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
