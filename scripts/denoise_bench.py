#!/usr/bin/env python3
"""What the feature buffers (mfx_aov) and the denoiser (mfx_denoise) cost and buy on C2 (spot,
1920x1080): one JSON line.

Device ms (HIP events inside the calls, the fastest of --calls): mfx_aov(4), mfx_denoise at the
default DenoiseConfig from the accumulator (the fill, the iterations; once without outputs and once
with the FP64 frame and the RGBA8 post), and this build's uniform 64-spp trace, the step
`bench.py --config C2` times. RMSE against a uniform --ref-spp render of other samples (sample base
2^20) of: the raw 8-spp image (samples 0..7), its denoised image (features of samples 0..3), the raw
64-spp image, and the denoised 64-spp image.
`detail` is what the decision about LDS tiling rests on: the device ms of 1, 2, 3 and 4 iterations (an
iteration's cost by its step: neighbouring pixels' taps overlap at steps 1 and 2, not at 4 and 8) and of
three iterations with every sigma 0 (the same colour taps, no feature loads and no divisions per tap).
The variance-guided filter (mfx_denoise_var at the default DenoiseVarConfig): `denoise_var_ms` is the
fastest warm call from the adaptive sampler's result on the device after sample_adaptive(min = max = 8),
`denoise_var_vs_denoise_ms` its ratio to `denoise_ms`, `rmse_var8` / `rmse_var64` the RMSE of its image
of samples 0..7 / 0..63; `detail` has its ms by iterations and with the luminance term off."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per figure (the fastest is reported)")
    ap.add_argument("--aov-spp", type=int, default=4)
    args = ap.parse_args()

    import numpy as np
    from mafrixraytracing_amd.abi import MFX_DN_SRC_ACCUM, MFX_DN_SRC_ADAPTIVE, MfxDenoiseCfg, MfxDenoiseVarCfg, dptr
    from mafrixraytracing_amd.denoise import DenoiseConfig, DenoiseVarConfig
    from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext
    from mafrixraytracing_amd.scene_io import load_scene_file

    a = load_scene_file(os.path.join(ROOT, "scenes", "spot.xml"))
    w, h = a.width, a.height
    dc = DenoiseConfig()

    with NativeContext(a, seed=DEFAULT_SEED) as ctx:  # the reference: other samples than any image's
        ctx.accum_clear()
        ctx.trace_accumulate(args.ref_spp, 1 << 20)
        ref = ctx.accum_read_mean(float(args.ref_spp))[:, :3].copy()
        own = []
        for k in range(args.calls + 1):  # the first call allocates the pool
            ctx.accum_clear()
            ctx.trace_accumulate(64, 64 * k)
            ctx.sync()
            own.append(ctx.last_trace_ms())
        uniform64_ms = min(own[1:])

    def rmse(img):
        return float(np.sqrt(np.mean((img[:, :3] - ref) ** 2)))

    def timed(fn):
        ms = C.c_double()
        got = []
        for _ in range(args.calls + 1):  # the first call allocates the buffers
            rc = fn(C.byref(ms))
            assert rc == 0, rc
            got.append(ms.value)
        return min(got[1:])

    res = {}
    for spp in (8, 64):
        with NativeContext(a, seed=DEFAULT_SEED) as ctx:
            raw = ctx.sample(spp)
            hit = ctx.aov(args.aov_spp)[:, 7]
            den = ctx.denoise(None, count=spp, cfg=dc)
            res[spp] = {"raw_rmse": rmse(raw), "denoised_rmse": rmse(den)}
            if spp != 8:
                continue
            cfg = MfxDenoiseCfg(iterations=dc.iterations, source=MFX_DN_SRC_ACCUM, count=float(spp),
                                sigma_normal=dc.sigma_normal, sigma_depth=dc.sigma_depth,
                                sigma_albedo=dc.sigma_albedo, sigma_color=dc.sigma_color)
            out = np.empty((w * h, 4))
            rgba = np.empty(w * h * 4, dtype=np.uint8)
            aov_ms = timed(lambda ms: ctx.lib.mfx_aov(ctx._h, args.aov_spp, 0, None, ms))
            dn_ms = timed(lambda ms: ctx.lib.mfx_denoise(ctx._h, C.byref(cfg), None, None, None, ms))
            dn_out_ms = timed(lambda ms: ctx.lib.mfx_denoise(ctx._h, C.byref(cfg), None, dptr(out),
                                                             rgba.ctypes.data_as(C.POINTER(C.c_uint8)), ms))
            hit_fraction = float(hit.mean())

            def variant(**kw):
                d = dict(iterations=dc.iterations, source=MFX_DN_SRC_ACCUM, count=float(spp), sigma_normal=dc.sigma_normal,
                         sigma_depth=dc.sigma_depth, sigma_albedo=dc.sigma_albedo, sigma_color=dc.sigma_color)
                d.update(kw)
                v = MfxDenoiseCfg(**d)
                return round(timed(lambda ms: ctx.lib.mfx_denoise(ctx._h, C.byref(v), None, None, None, ms)), 3)

            detail = {"ms_by_iterations": [variant(iterations=n) for n in (1, 2, 3, 4)],
                      "ms_all_sigmas_0": variant(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
                      "ms_normal_only": variant(sigma_depth=0.0, sigma_albedo=0.0)}
    # the variance-guided filter from the adaptive sampler's result on the device (min = max: uniform
    # counts, the same samples 0..spp-1 as the images above)
    dv = DenoiseVarConfig()
    for spp in (8, 64):
        with NativeContext(a, seed=DEFAULT_SEED) as ctx:
            ctx.aov(args.aov_spp)
            ctx.sample_adaptive(spp, spp, 1, 0.0, 0.0)
            res[spp]["var_rmse"] = rmse(ctx.denoise_var(None, cfg=dv))
            if spp != 8:
                continue

            def var_variant(**kw):
                d = dict(iterations=dv.iterations, source=MFX_DN_SRC_ADAPTIVE, sigma_normal=dv.sigma_normal,
                         sigma_depth=dv.sigma_depth, sigma_albedo=dv.sigma_albedo, sigma_luma=dv.sigma_luma,
                         luma_floor=dv.luma_floor)
                d.update(kw)
                v = MfxDenoiseVarCfg(**d)
                return timed(lambda ms: ctx.lib.mfx_denoise_var(ctx._h, C.byref(v), None, None, None, None, None, ms))

            dnv_ms = var_variant()
            detail["var_ms_by_iterations"] = [round(var_variant(iterations=n), 3) for n in (1, 2, 3, 4)]
            detail["var_ms_sigma_luma_0"] = round(var_variant(sigma_luma=0.0), 3)
    out = {"workload": f"C2 spot {w}x{h}", "aov_spp": args.aov_spp, "aov_ms": round(aov_ms, 3),
           "denoise": {"iterations": dc.iterations, "sigma_normal": dc.sigma_normal, "sigma_depth": dc.sigma_depth,
                       "sigma_albedo": dc.sigma_albedo, "sigma_color": dc.sigma_color},
           "denoise_ms": round(dn_ms, 3), "denoise_ms_with_outputs": round(dn_out_ms, 3),
           "denoise_var": {"iterations": dv.iterations, "sigma_normal": dv.sigma_normal, "sigma_depth": dv.sigma_depth,
                           "sigma_albedo": dv.sigma_albedo, "sigma_luma": dv.sigma_luma, "luma_floor": dv.luma_floor},
           "denoise_var_ms": round(dnv_ms, 3), "denoise_var_vs_denoise_ms": round(dnv_ms / dn_ms, 4),
           "rmse_var8": res[8]["var_rmse"], "rmse_var64": res[64]["var_rmse"],
           "uniform64_trace_ms": round(uniform64_ms, 3),
           "aov_plus_denoise_vs_uniform64": round((aov_ms + dn_ms) / uniform64_ms, 4),
           "reference_spp": args.ref_spp, "hit_fraction": round(hit_fraction, 4),
           "rmse_raw8": res[8]["raw_rmse"], "rmse_denoised8": res[8]["denoised_rmse"],
           "rmse_raw64": res[64]["raw_rmse"], "rmse_denoised64": res[64]["denoised_rmse"],
           "denoised8_vs_raw8": round(res[8]["denoised_rmse"] / res[8]["raw_rmse"], 4), "detail": detail}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
