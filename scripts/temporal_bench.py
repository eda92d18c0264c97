#!/usr/bin/env python3
"""What a camera move costs and what the temporal history buys on C2 (spot, 1920x1080): one JSON line.

mfx_set_camera: host wall ms of the call (it waits for the context's work; the fastest of --calls), in
place (a move towards the scene) and with a rebuild (moves away from it, each farther out than the one
before), against a fresh context's mfx_build_info out[2] (the whole scene preparation) and the wall ms of
creating one: the process's first context, and a second one (the GPU build's kernels are loaded by then).
mfx_temporal: device ms (HIP events inside the call, the fastest of --calls) from the adaptive sampler's
result on the device, without outputs and with the FP64 frame and the RGBA8 post, beside mfx_denoise_var's
at the default DenoiseVarConfig from the same source.
RMSE against a uniform --ref-spp render of other samples (sample base 2^20) at the moved camera of: the raw
8-spp frame there, the same after mfx_temporal with a 64-spp history from the camera before the move,
and both through mfx_denoise_var; `accepted` is the share of pixels that took history."""
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
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per figure (the fastest is reported)")
    ap.add_argument("--move", type=float, default=0.03, help="the move, as a share of the camera's distance from the origin")
    args = ap.parse_args()

    import numpy as np
    from mafrixraytracing_amd.abi import MFX_DN_SRC_ADAPTIVE, MfxTemporalCfg, SceneArrays
    from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext
    from mafrixraytracing_amd.scene_io import load_scene_file
    from mafrixraytracing_amd.temporal import TemporalConfig

    a = load_scene_file(os.path.join(ROOT, "scenes", "spot.xml"))
    w, h = a.width, a.height

    def scaled(f):
        return {**a.camera, "position": tuple(float(p) * f for p in a.camera["position"])}

    near = scaled(1.0 - args.move)
    tc = TemporalConfig()

    t0 = time.perf_counter()
    ctx = NativeContext(a, seed=DEFAULT_SEED)
    create_ms = (time.perf_counter() - t0) * 1e3
    with ctx:
        scene_ms = ctx.build_info()["scene_ms"]
        t0 = time.perf_counter()
        with NativeContext(a, seed=DEFAULT_SEED) as second:  # a create in a process that has created before
            warm_create_ms = (time.perf_counter() - t0) * 1e3
            warm_scene_ms = second.build_info()["scene_ms"]
        ctx.sample(1)  # (the pool)

        def wall(fn):
            t = time.perf_counter()
            fn()
            return (time.perf_counter() - t) * 1e3

        in_place, rebuild, rebuild_scene = [], [], []
        for _ in range(args.calls):
            in_place.append(wall(lambda: ctx.set_camera(near)))
            assert ctx.camera_info()["rebuilds"] == len(rebuild)
            in_place.append(wall(lambda: ctx.set_camera(a.camera)))
        for k in range(args.calls):  # each farther out than the images were built for: a rebuild every time
            rebuild.append(wall(lambda: ctx.set_camera(scaled(1.5 + 0.5 * k))))
            assert ctx.camera_info()["rebuilds"] == k + 1
            rebuild_scene.append(ctx.build_info()["scene_ms"])

    with NativeContext(SceneArrays(a.prims, a.albedo, a.light, near, w, h, a.max_depth), seed=DEFAULT_SEED) as r:
        r.accum_clear()
        r.trace_accumulate(args.ref_spp, 1 << 20)
        ref = r.accum_read_mean(float(args.ref_spp))[:, :3].copy()

    def rmse(img):
        return float(np.sqrt(np.mean((img[:, :3] - ref) ** 2)))

    with NativeContext(a, seed=DEFAULT_SEED) as ctx:
        ctx.aov(4)
        ctx.sample_adaptive(64, 64, 1, 0.0, 0.0)  # 64 spp before the move
        ctx.temporal(None, cfg=tc, restart=True)
        ctx.set_camera(near)
        assert ctx.camera_info()["rebuilds"] == 0
        ctx.aov(4, 64)
        raw, _ = ctx.sample_adaptive(8, 8, 1, 0.0, 0.0)  # 8 spp after it
        raw_dn = ctx.denoise_var(None)
        dv_ms = []
        for _ in range(args.calls):
            ctx.denoise_var(None)
            dv_ms.append(ctx.last_denoise_ms)
        merged, _, cnt, acc = ctx.temporal(None, cfg=tc)
        merged_dn = ctx.denoise_var(source="temporal")
        cfg = MfxTemporalCfg(source=MFX_DN_SRC_ADAPTIVE, restart=0, tol_depth=tc.tol_depth, tol_normal2=tc.tol_normal2,
                             max_history=tc.max_history)
        bare, full = [], []
        ms = C.c_double()
        for _ in range(args.calls):
            assert ctx.lib.mfx_temporal(ctx._h, C.byref(cfg), None, None, None, None, None, None, None, None, C.byref(ms)) == 0
            bare.append(ms.value)
            ctx.temporal(None, cfg=tc, want_rgba=True)
            full.append(ctx.last_temporal_ms)

    print(json.dumps({
        "config": "C2", "width": w, "height": h, "move": args.move,
        "create_wall_ms": create_ms, "create_scene_ms": scene_ms,
        "second_create_wall_ms": warm_create_ms, "second_create_scene_ms": warm_scene_ms,
        "set_camera_in_place_ms": min(in_place), "set_camera_rebuild_ms": min(rebuild),
        "rebuild_scene_ms": min(rebuild_scene),
        "temporal_ms": min(bare), "temporal_with_outputs_ms": min(full), "denoise_var_ms": min(dv_ms),
        "accepted": acc / float(w * h), "history_mean_count": float(cnt.mean()),
        "rmse_raw8": rmse(raw), "rmse_temporal": rmse(merged), "rmse_raw8_denoised": rmse(raw_dn),
        "rmse_temporal_denoised": rmse(merged_dn), "ref_spp": args.ref_spp,
        "tol_depth": tc.tol_depth, "tol_normal2": tc.tol_normal2, "max_history": tc.max_history,
    }))


if __name__ == "__main__":
    main()
