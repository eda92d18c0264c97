#!/usr/bin/env python3
"""What resuming the adaptive sampler (mfx_sample_adaptive_resume) costs on C2 (spot, 1920x1080): one
JSON line. Everything is measured against (a) of the same build in the same process:
  a  one mfx_sample_adaptive call, min 8 / step 8 / max 64 at rel_error --rel (default 0.05).
  b  min = max = 8, then one resume to 64 without a pass limit: the same samples and rays as (a).
  c  min = max = 8, then resumes of one pass each until none is active: (a) again, one call per pass;
     per_call_overhead_ms is what a call adds over (a), per resume call.
  d  a finished (a) resumed to --more (default 256) in steps of --more-step (default 32).
  noop  a repeated resume on a finished result: the entry check over every tile and the mean kernel,
     which every resume call pays whatever it traces.
Each run reports rays, passes (traces), device ms (the checks, the passes and the mean kernel, from
HIP events; summed over the run's calls), wall ms of calls that read back only the tile counts, and
its RMSE against a uniform --ref-spp render of other samples (sample base 2^20); `stages` splits the
device time into the closest-hit kernels, k_shadow and the rest (resolve, memsets, checks, mean).
Timed figures are the fastest of --calls repetitions, each on later sample ranges of one context."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rel", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--more", type=int, default=256)
    ap.add_argument("--more-step", type=int, default=32)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=3, help="timed repetitions per run (the fastest is reported)")
    args = ap.parse_args()

    import numpy as np
    from mafrixraytracing_amd.abi import MfxAdaptive, MfxAdaptiveResume, iptr
    from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext
    from mafrixraytracing_amd.scene_io import load_scene_file

    a = load_scene_file(os.path.join(ROOT, "scenes", "spot.xml"))
    w, h = a.width, a.height
    ty_n, tx_n = (h + 7) // 8, (w + 7) // 8
    valid = np.minimum(8, w - 8 * np.arange(tx_n))[None, :] * np.minimum(8, h - 8 * np.arange(ty_n))[:, None]
    rel, floor = args.rel, args.floor

    with NativeContext(a, seed=DEFAULT_SEED) as ctx:  # the reference: other samples than any run's
        ctx.accum_clear()
        ctx.trace_accumulate(args.ref_spp, 1 << 20)
        ref = ctx.accum_read_mean(float(args.ref_spp))[:, :3].copy()

    def rmse(img):
        return float(np.sqrt(np.mean((img[:, :3] - ref) ** 2)))

    tiles = np.zeros((ty_n, tx_n), dtype=np.int32)

    def stages(ctx):  # mfx_trace_timing's split of the call's device time: closest-hit kernels, k_shadow, the rest
        t = ctx.trace_timing()
        return np.array([t["extend_ms"], t["shadow_ms"], t["total_ms"] - t["extend_ms"] - t["shadow_ms"]])

    def first(ctx, mn, mx):  # counts only; returns (device ms, wall ms, rays)
        cfg = MfxAdaptive(min_spp=mn, max_spp=mx, step_spp=8, reserved=0, rel_error=rel, abs_floor=floor)
        t0 = time.perf_counter()
        rc = ctx.lib.mfx_sample_adaptive(ctx._h, C.byref(cfg), None, iptr(tiles), None)
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, ctx.lib.mfx_last_error()
        return ctx.last_trace_ms(), wall, float(ctx.ray_counts()[:3].sum()), stages(ctx)

    def resume(ctx, mx, step, max_passes):  # counts only; returns (device ms, wall ms, rays, active)
        cfg = MfxAdaptiveResume(max_spp=mx, step_spp=step, max_passes=max_passes, reserved=0, rel_error=rel, abs_floor=floor)
        active = C.c_int32(-1)
        t0 = time.perf_counter()
        rc = ctx.lib.mfx_sample_adaptive_resume(ctx._h, C.byref(cfg), None, iptr(tiles), None, C.byref(active))
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, ctx.lib.mfx_last_error()
        return ctx.last_trace_ms(), wall, float(ctx.ray_counts()[:3].sum()), active.value, stages(ctx)

    def run_a(ctx):
        d, wl, rays, st = first(ctx, 8, 64)
        return dict(device_ms=d, wall_ms=wl, rays=rays, calls=1, passes=(int(tiles.max()) - 8) // 8 + 1, stages=st)

    def run_b(ctx):
        d, wl, rays, st = first(ctx, 8, 8)
        d2, wl2, rays2, active, st2 = resume(ctx, 64, 8, 0)
        assert active == 0
        return dict(device_ms=d + d2, wall_ms=wl + wl2, rays=rays + rays2, calls=2, passes=(int(tiles.max()) - 8) // 8 + 1,
                    resume_device_ms=d2, stages=st + st2)

    def run_c(ctx):
        d, wl, rays, st = first(ctx, 8, 8)
        calls, passes = 1, 1
        while True:
            d2, wl2, rays2, active, st2 = resume(ctx, 64, 8, 1)
            d, wl, rays, calls, st = d + d2, wl + wl2, rays + rays2, calls + 1, st + st2
            passes += 1 if rays2 > 0 else 0
            if active == 0:
                return dict(device_ms=d, wall_ms=wl, rays=rays, calls=calls, passes=passes, stages=st)

    def run_d(ctx):
        first(ctx, 8, 64)
        before = int((tiles * valid).sum())
        d, wl, rays, active, st = resume(ctx, args.more, args.more_step, 0)
        assert active == 0
        return dict(device_ms=d, wall_ms=wl, rays=rays, calls=1, passes=-(-(int(tiles.max()) - 64) // args.more_step), stages=st,
                    mean_spp_before=before / (w * h), mean_spp_after=float((tiles * valid).sum() / (w * h)),
                    tiles_resumed=int((tiles > 64).sum()), tiles_at_max=int((tiles == args.more).sum()))

    def run_noop(ctx):
        first(ctx, 8, 64)
        d, wl, rays, active, st = resume(ctx, 64, 8, 0)
        assert active == 0 and rays == 0
        return dict(device_ms=d, wall_ms=wl, rays=rays, calls=1, passes=0, stages=st)

    def timed(fn):
        with NativeContext(a, seed=DEFAULT_SEED) as ctx:
            fn(ctx)  # warm: allocates the pool and the planes
            best = min((fn(ctx) for _ in range(args.calls)), key=lambda r: r["device_ms"])
        best["stages"] = dict(zip(("closest_ms", "shadow_ms", "rest_ms"), (round(float(v), 3) for v in best["stages"])))
        return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in best.items()}

    runs = {"a": timed(run_a), "b": timed(run_b), "c": timed(run_c), "d": timed(run_d), "noop": timed(run_noop)}

    # the images, from fresh contexts (samples from 0): (a), (b) and (c) are one image; (d) goes on from it
    with NativeContext(a, seed=DEFAULT_SEED) as ctx:
        fa, ta = ctx.sample_adaptive(8, 64, 8, rel, floor)
        fd, td, _ = ctx.sample_adaptive_resume(args.more, args.more_step, rel, floor)
    with NativeContext(a, seed=DEFAULT_SEED) as ctx:
        ctx.sample_adaptive(8, 8, 8, rel, floor)
        fb, tb, _ = ctx.sample_adaptive_resume(64, 8, rel, floor)
    runs["a"]["rmse"] = runs["c"]["rmse"] = rmse(fa)
    runs["b"]["rmse"] = rmse(fb)
    runs["d"]["rmse"] = rmse(fd)
    runs["a"]["mean_spp"] = round(float((ta * valid).sum() / (w * h)), 3)
    A = runs["a"]
    out = {"workload": f"C2 spot {w}x{h}", "rel_error": rel, "abs_floor": floor, "reference_spp": args.ref_spp,
           "b_equals_a": bool(np.array_equal(fa, fb) and np.array_equal(ta, tb)), "runs": runs,
           "b_over_a_device_ms": round(runs["b"]["device_ms"] - A["device_ms"], 3),
           "c_over_a_device_ms": round(runs["c"]["device_ms"] - A["device_ms"], 3),
           "per_call_overhead_ms": {"device": round((runs["c"]["device_ms"] - A["device_ms"]) / (runs["c"]["calls"] - 1), 3),
                                    "wall": round((runs["c"]["wall_ms"] - A["wall_ms"]) / (runs["c"]["calls"] - 1), 3)},
           "d_device_ms_per_Mray": round(runs["d"]["device_ms"] / (runs["d"]["rays"] / 1e6), 5),
           "a_device_ms_per_Mray": round(A["device_ms"] / (A["rays"] / 1e6), 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
