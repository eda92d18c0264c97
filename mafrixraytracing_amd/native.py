"""Host-side mirror of the reference's render API over the C ABI.

`Scene`, `NativePixelIntegrator` and `Film` keep the names and argument meaning of
EngineCore/Scene/Scene.fs:291-333, Core/Integrator/Integrators.fs:143-172 and
Core/Film.fs:13-34; all work happens in libmafrix_rt.so on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import (INSTANCING_KEYS, LAUNCH_INFO_KEYS, MFX_DN_SRC_ACCUM, MFX_DN_SRC_ADAPTIVE, MFX_DN_SRC_HOST,
                  MFX_DN_SRC_TEMPORAL, MFX_F_NONE, MFX_F_TWO_LEVEL, MfxAdaptive, MfxAdaptiveResume, MfxDenoiseCfg,
                  MfxDenoiseVarCfg, MfxInstance, MfxOptions, MfxPrimNormals, MfxPrimUv, MfxTemporalCfg, PRIM_NORMALS_DTYPE,
                  PRIM_UV_DTYPE, SceneArrays, check, dptr,
                  iptr, load_library, pinhole_struct, quad_lights, texture_structs, environment_struct, lens_struct)
from .denoise import DenoiseConfig, DenoiseVarConfig
from .temporal import TemporalConfig

DEFAULT_SEED = 0x4D414652
DEFAULT_RENDER_AHEAD = 64  # fsharp/Native.fs DefaultRenderAhead: Scene.Render served from batches of 64 samples


class NativeContext:
    """One mfx_ctx: a scene resident in HBM on one GPU."""

    def __init__(self, arrays: SceneArrays, seed: int = DEFAULT_SEED, device: int = 0, flags: int = MFX_F_NONE,
                 part_index: int = 0, part_count: int = 1, devices: list[int] | None = None,
                 instancing: bool = True, render_ahead: int = 0, lights: list | None = None,
                 textures: list | None = None, prim_uv: np.ndarray | None = None, environment=None,
                 sample_sky: bool = False, lens=None, normals: np.ndarray | None = None):
        """devices: drive this list of HIP devices from one context (mfx_options.devices; the
        library's own RCCL reduce sums them into devices[0]); None: the single `device`.
        instancing: a scene with instancing data is created through mfx_create_instanced (two-level
        traversal; MFX_F_FLATTEN flattens it in the library); False: mfx_create on the world list.
        render_ahead: mfx_options.render_ahead (one-sample render calls served from batches of K
        samples; 0 = off).
        lights: a list of light dicts (scene_io's shape: p, normal, intensity) creates the context through
        mfx_create_lights (one light picked per path vertex, the image is the lights' sum; they replace
        arrays.light). Pass arrays.lights for a scene loaded with all_lights=True. None: mfx_create /
        mfx_create_instanced with arrays.light alone, whatever arrays.lights holds.
        textures, prim_uv: albedo textures ((H, W, 4) uint8 arrays, rows top to bottom) and the primitives' maps
        (abi.PRIM_UV_DTYPE, one per primitive the context is created from: the templates of an instanced
        scene, the world list otherwise) create the context through mfx_create_textured, with `lights` or
        arrays.light. Pass arrays.textures and arrays.prim_uv for a scene loaded with textures=True. None:
        an untextured context, whatever arrays holds.
        environment: an (S, S, 3) float32 octahedral map of linear RGB radiance (environment.py makes them), set
        with set_environment right after creation: rays that leave the scene return its texel. None: black.
        sample_sky: set it with mfx_set_environment_sampled instead: the sky is a light, sampled at every vertex.
        lens: (aperture, focus), set with set_lens right after creation: a thin lens with depth of field. None: the
        pinhole.
        normals: corner normals (abi.PRIM_NORMALS_DTYPE, one per primitive the context is created from, as prim_uv),
        set with set_normals right after creation: smooth shading. Pass arrays.prim_normals for a scene loaded with
        normals=True, or normals.smooth_normals(prims). None: face normals."""
        self.lib = load_library()
        self.arrays = arrays
        self.w, self.h = arrays.width, arrays.height
        inst = instancing and arrays.instancing is not None
        if inst and getattr(arrays, "two_level", False):
            flags |= MFX_F_TWO_LEVEL
        self._desc = arrays.desc(templates=inst)
        self.devices = list(devices) if devices else [device]
        self._devs = (C.c_int32 * len(self.devices))(*self.devices)
        opt = MfxOptions(seed=seed, device=device, flags=flags, part_index=part_index, part_count=part_count,
                         ndevices=len(devices) if devices else 0, render_ahead=render_ahead,
                         devices=C.cast(self._devs, C.POINTER(C.c_int32)) if devices else None)
        h = C.c_void_p()
        self.lights = list(lights) if lights is not None else None
        if textures is not None or prim_uv is not None:
            ls = self.lights if self.lights is not None else [arrays.light]
            self._lights = quad_lights(ls)
            self._inst = arrays.instancing[1] if inst else None
            ip = self._inst.ctypes.data_as(C.POINTER(MfxInstance)) if inst else None
            self._tex, self._tex_keep = texture_structs(textures or [])
            self._uv = np.ascontiguousarray(prim_uv, dtype=PRIM_UV_DTYPE) if prim_uv is not None else None
            if self._uv is not None and len(self._uv) != self._desc.nprims:
                raise ValueError(f"prim_uv has {len(self._uv)} entries for {self._desc.nprims} primitives")
            up = self._uv.ctypes.data_as(C.POINTER(MfxPrimUv)) if self._uv is not None else None
            check(self.lib.mfx_create_textured(C.byref(self._desc), self._lights, len(ls), ip,
                                               len(self._inst) if inst else 0, self._tex, len(self._tex_keep), up,
                                               C.byref(opt), C.byref(h)), "mfx_create_textured")
        elif self.lights is not None:
            self._lights = quad_lights(self.lights)
            self._inst = arrays.instancing[1] if inst else None
            ip = self._inst.ctypes.data_as(C.POINTER(MfxInstance)) if inst else None
            check(self.lib.mfx_create_lights(C.byref(self._desc), self._lights, len(self.lights), ip,
                                             len(self._inst) if inst else 0, C.byref(opt), C.byref(h)), "mfx_create_lights")
        elif inst:
            self._inst = arrays.instancing[1]
            ip = self._inst.ctypes.data_as(C.POINTER(MfxInstance))
            check(self.lib.mfx_create_instanced(C.byref(self._desc), ip, len(self._inst), C.byref(opt), C.byref(h)),
                  "mfx_create_instanced")
        else:
            check(self.lib.mfx_create(C.byref(self._desc), C.byref(opt), C.byref(h)), "mfx_create")
        self._h = h
        try:
            if environment is not None:
                self.set_environment(environment, sampled=sample_sky)
            if lens is not None:
                self.set_lens(lens)
            if normals is not None:
                self.set_normals(normals)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mfx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- reference API -------------------------------------------------------------------
    def sample(self, spp: int, out: np.ndarray | None = None) -> np.ndarray:
        """IPixelIntegrator.Sample(spp) into `out` (w*h x 4 doubles, x-major; allocated if None), as
        the reference writes the Color[w,h] array it owns (Integrators.fs:160-172)."""
        frame = out if out is not None else np.empty((self.w * self.h, 4), dtype=np.float64)
        assert frame.dtype == np.float64 and frame.size == self.w * self.h * 4 and frame.flags.c_contiguous
        check(self.lib.mfx_sample(self._h, spp, dptr(frame)), "mfx_sample")
        return frame

    def sample_adaptive(self, min_spp: int, max_spp: int, step_spp: int, rel_error: float, abs_floor: float,
                        want_rgba: bool = False):
        """mfx_sample_adaptive: Sample with a per-tile early stop (the rule: include/mafrix_rt.h,
        mafrixraytracing_amd/adaptive.py). Returns (frame, tile_spp) or (frame, tile_spp, rgba): the
        (w*h, 4) x-major mean of every pixel over its own tile's sample count, the (tiles_y, tiles_x)
        int32 counts of the film's 8x8 tiles, and the same mean as y-major RGBA8 (w*h*4 bytes)."""
        cfg = MfxAdaptive(min_spp=min_spp, max_spp=max_spp, step_spp=step_spp, reserved=0,
                          rel_error=rel_error, abs_floor=abs_floor)
        frame = np.empty((self.w * self.h, 4), dtype=np.float64)
        tiles = np.zeros(((self.h + 7) // 8, (self.w + 7) // 8), dtype=np.int32)
        rgba = np.empty(self.w * self.h * 4, dtype=np.uint8) if want_rgba else None
        check(self.lib.mfx_sample_adaptive(self._h, C.byref(cfg), dptr(frame), iptr(tiles),
                                           rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None),
              "mfx_sample_adaptive")
        return (frame, tiles, rgba) if want_rgba else (frame, tiles)

    def sample_adaptive_resume(self, max_spp: int, step_spp: int, rel_error: float, abs_floor: float,
                               max_passes: int = 0, want_rgba: bool = False):
        """mfx_sample_adaptive_resume: continue the adaptive result the context holds under this call's
        threshold and budget, every tile from its own count, for at most max_passes passes (0: until no
        tile is active; the rule: include/mafrix_rt.h, adaptive.py reference_resume). Returns
        (frame, tile_spp, active) or (frame, tile_spp, rgba, active): sample_adaptive's outputs for the
        tiles' current counts, and the number of tiles that would go on."""
        cfg = MfxAdaptiveResume(max_spp=max_spp, step_spp=step_spp, max_passes=max_passes, reserved=0,
                                rel_error=rel_error, abs_floor=abs_floor)
        frame = np.empty((self.w * self.h, 4), dtype=np.float64)
        tiles = np.zeros(((self.h + 7) // 8, (self.w + 7) // 8), dtype=np.int32)
        rgba = np.empty(self.w * self.h * 4, dtype=np.uint8) if want_rgba else None
        active = C.c_int32(-1)
        check(self.lib.mfx_sample_adaptive_resume(self._h, C.byref(cfg), dptr(frame), iptr(tiles),
                                                  rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None,
                                                  C.byref(active)),
              "mfx_sample_adaptive_resume")
        return (frame, tiles, rgba, active.value) if want_rgba else (frame, tiles, active.value)

    def aov(self, spp: int, sample_base: int = 0) -> np.ndarray:
        """mfx_aov: the (w*h, 8) x-major first-hit features of the film's own camera rays, averaged over
        global samples sample_base .. sample_base + spp - 1: normal xyz, hit t, albedo rgb, hit fraction.
        They stay on the device as the context's feature buffers (what denoise is guided by)."""
        out = np.empty((self.w * self.h, 8), dtype=np.float64)
        ms = C.c_double()
        check(self.lib.mfx_aov(self._h, spp, sample_base, dptr(out), C.byref(ms)), "mfx_aov")
        self.last_aov_ms = ms.value
        return out

    def denoise(self, frame: np.ndarray | None = None, count: float | None = None,
                cfg: DenoiseConfig = DenoiseConfig(), want_rgba: bool = False):
        """mfx_denoise: the edge-avoiding a-trous filter (the rule: include/mafrix_rt.h,
        mafrixraytracing_amd/denoise.py) of `frame` ((w*h, 4) x-major, alpha ignored), or with
        frame=None of the context's accumulator / count; guided by the feature buffers of the last
        aov call. Returns the (w*h, 4) filtered frame, or (frame, rgba) with its y-major RGBA8 post."""
        c = MfxDenoiseCfg(iterations=cfg.iterations, source=MFX_DN_SRC_ACCUM if frame is None else MFX_DN_SRC_HOST,
                          count=float(count) if count is not None else 0.0, sigma_normal=cfg.sigma_normal,
                          sigma_depth=cfg.sigma_depth, sigma_albedo=cfg.sigma_albedo, sigma_color=cfg.sigma_color)
        src = None
        if frame is not None:
            src = np.ascontiguousarray(frame, dtype=np.float64)
            assert src.size == self.w * self.h * 4
        out = np.empty((self.w * self.h, 4), dtype=np.float64)
        rgba = np.empty(self.w * self.h * 4, dtype=np.uint8) if want_rgba else None
        ms = C.c_double()
        check(self.lib.mfx_denoise(self._h, C.byref(c), dptr(src) if src is not None else None, dptr(out),
                                   rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None, C.byref(ms)),
              "mfx_denoise")
        self.last_denoise_ms = ms.value
        return (out, rgba) if want_rgba else out

    def denoise_var(self, frame: np.ndarray | None = None, variance: np.ndarray | None = None,
                    cfg: DenoiseVarConfig = DenoiseVarConfig(), want_rgba: bool = False, want_variance: bool = False,
                    source: str | None = None):
        """mfx_denoise_var: the variance-guided a-trous filter (the rule: include/mafrix_rt.h,
        mafrixraytracing_amd/denoise.py) of `frame` ((w*h, 4) x-major, alpha ignored) with `variance`
        ((w*h,) x-major, the variance of each pixel's mean luminance), or with frame=None of the last
        sample_adaptive's result (as resumed since) as it lies on the device (its accumulator, moments and tile counts);
        or with source="temporal" of the colour and variance the last temporal() call left on the device;
        guided by the feature buffers of the last aov call. Returns the (w*h, 4) filtered frame, or a
        tuple of it, the y-major RGBA8 post (want_rgba) and the (w*h,) filtered variance (want_variance)."""
        if source not in (None, "temporal"):
            raise ValueError('source: None (the frame given, else the adaptive result) or "temporal"')
        src_code = MFX_DN_SRC_TEMPORAL if source == "temporal" else (MFX_DN_SRC_ADAPTIVE if frame is None else MFX_DN_SRC_HOST)
        c = MfxDenoiseVarCfg(iterations=cfg.iterations, source=src_code,
                             sigma_normal=cfg.sigma_normal, sigma_depth=cfg.sigma_depth, sigma_albedo=cfg.sigma_albedo,
                             sigma_luma=cfg.sigma_luma, luma_floor=cfg.luma_floor)
        src = var = None
        if frame is not None:
            src = np.ascontiguousarray(frame, dtype=np.float64)
            assert src.size == self.w * self.h * 4
        if variance is not None:
            var = np.ascontiguousarray(variance, dtype=np.float64)
            assert var.size == self.w * self.h
        out = np.empty((self.w * self.h, 4), dtype=np.float64)
        rgba = np.empty(self.w * self.h * 4, dtype=np.uint8) if want_rgba else None
        vout = np.empty(self.w * self.h, dtype=np.float64) if want_variance else None
        ms = C.c_double()
        check(self.lib.mfx_denoise_var(self._h, C.byref(c), dptr(src) if src is not None else None,
                                       dptr(var) if var is not None else None, dptr(out),
                                       dptr(vout) if want_variance else None,
                                       rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None, C.byref(ms)),
              "mfx_denoise_var")
        self.last_denoise_ms = ms.value
        res = (out,) + ((rgba,) if want_rgba else ()) + ((vout,) if want_variance else ())
        return res if len(res) > 1 else out

    def set_camera(self, camera):
        """mfx_set_camera: make `camera` (a scene-file camera dict, a derived one with position, topleft,
        right, down, or an MfxPinhole) the camera of every later call. In place when the traversal images'
        box widening still covers it, else the images are built again (camera_info tells which). The
        film, the accumulator and next_sample are left as they are: reset() after a move, as the
        reference's Film.Reset. aov() and sample_adaptive() must run again before denoise, denoise_var,
        temporal and sample_adaptive_resume."""
        p = pinhole_struct(camera)
        check(self.lib.mfx_set_camera(self._h, C.byref(p)), "mfx_set_camera")

    def set_lens(self, lens):
        """mfx_set_lens: make lens = (aperture, focus) the thin lens of every later call (aperture: the lens radius in
        world units, focus: the distance of the sharp plane along the forward axis); None or an aperture of 0 removes
        it. In place when the traversal images' box widening covers the lens disk, else the images are built again
        (lens_info tells). The film, the accumulator and next_sample are left as they are; aov() and
        sample_adaptive() must run again before denoise, denoise_var and sample_adaptive_resume, and temporal() is
        refused under a lens."""
        if lens is None:
            check(self.lib.mfx_set_lens(self._h, None), "mfx_set_lens")
            return
        ln = lens_struct(lens)
        check(self.lib.mfx_set_lens(self._h, C.byref(ln)), "mfx_set_lens")

    def set_normals(self, normals):
        """mfx_set_normals: make `normals` (abi.PRIM_NORMALS_DTYPE, one per primitive the context was created from:
        the templates of an instanced scene, the world list otherwise) the corner normals of every later call: a
        smooth primitive is shaded with the interpolated normal of the hit point (the rule: include/mafrix_rt.h,
        normals.py); None removes them. The film, the accumulator and next_sample are left as they are; aov() and
        sample_adaptive() must run again before denoise, denoise_var and sample_adaptive_resume."""
        if normals is None:
            check(self.lib.mfx_set_normals(self._h, None, 0), "mfx_set_normals")
            return
        pn = np.ascontiguousarray(normals, dtype=PRIM_NORMALS_DTYPE)
        check(self.lib.mfx_set_normals(self._h, pn.ctypes.data_as(C.POINTER(MfxPrimNormals)), len(pn)), "mfx_set_normals")

    def normal_info(self) -> np.ndarray:
        """mfx_normal_info: [0] smooth world primitives, [1] 1 if the SN kernel instances run, [2] device bytes of the
        tables, [3] 0 (no pool bytes), [4] / [5] resident blocks per CU of the k_shadow / k_aov instance in use; the
        rest 0. All 0 without normals."""
        out = np.zeros(8)
        check(self.lib.mfx_normal_info(self._h, dptr(out)), "mfx_normal_info")
        return out

    def lens_info(self) -> np.ndarray:
        """mfx_lens_info: [0] 1 with a lens, [1] aperture, [2] focus, [3:6] U, [6:9] V, [9] s, [10] the eps the lens
        camera needs, [11] the image rebuilds set_lens caused, [12] / [13] resident blocks per CU of the k_extend
        instance that starts the paths / of the k_aov instance in use; the rest 0. All 0 without a lens."""
        out = np.zeros(16)
        check(self.lib.mfx_lens_info(self._h, dptr(out)), "mfx_lens_info")
        return out

    def set_environment(self, environment, sampled: bool = False):
        """mfx_set_environment: make the (S, S, 3) float32 octahedral map `environment` (linear RGB radiance; a
        (3,) constant works too) the sky of every later call, or with None remove it. The texels are copied.
        The film, the accumulator, next_sample and the feature buffers are left as they are; sample_adaptive()
        must run again before sample_adaptive_resume and the adaptive source of denoise_var.
        sampled: mfx_set_environment_sampled: the sky becomes the (N+1)-th light of the pick and is sampled at
        every path vertex in proportion to its radiance (at most 63 area lights beside it)."""
        name = "mfx_set_environment_sampled" if sampled else "mfx_set_environment"
        fn = getattr(self.lib, name)
        if environment is None:
            check(fn(self._h, None), name)
            return
        e, keep = environment_struct(environment)
        check(fn(self._h, C.byref(e)), name)
        del keep

    def sky_sampling_info(self) -> np.ndarray:
        """mfx_sky_sampling_info: [0] 1 if the sky is sampled, [1] N + 1, [2] bytes of the sampling table, [3] bytes
        per path slot the sampling adds to the pool, [4] / [5] resident blocks per CU of the k_shadow / k_resolve
        instance in use; [6], [7] 0. All 0 otherwise."""
        out = np.zeros(8)
        check(self.lib.mfx_sky_sampling_info(self._h, dptr(out)), "mfx_sky_sampling_info")
        return out

    def environment_info(self) -> np.ndarray:
        """mfx_environment_info: [0] size, [1] 1 if the environment kernel instances run, [2] bytes of texels,
        [3] bytes per path slot the environment adds to the pool, [4] / [5] resident blocks per CU of the
        k_extend / k_resolve instance in use; [6], [7] 0. All 0 without an environment."""
        out = np.zeros(8)
        check(self.lib.mfx_environment_info(self._h, dptr(out)), "mfx_environment_info")
        return out

    def camera_info(self) -> dict:
        """mfx_camera_info: the current derived camera (position, topleft, right, down; `derived` the twelve
        doubles in that order), the camera epoch, the box widening the images were built with, the one the
        current camera needs, and how often set_camera had to build the images again."""
        out = np.zeros(16)
        check(self.lib.mfx_camera_info(self._h, dptr(out)), "mfx_camera_info")
        return {"position": out[0:3].copy(), "topleft": out[3:6].copy(), "right": out[6:9].copy(), "down": out[9:12].copy(),
                "derived": out[0:12].copy(), "epoch": int(out[12]), "eps_built": float(out[13]),
                "eps_needed": float(out[14]), "rebuilds": int(out[15])}

    def temporal(self, frame: np.ndarray | None = None, variance: np.ndarray | None = None,
                 count: np.ndarray | None = None, cfg: TemporalConfig | None = None, restart: bool = False,
                 want_rgba: bool = False, **tolerances):
        """mfx_temporal: reproject the context's history into the current view and merge it with `frame`
        ((w*h, 4) x-major), its `variance` and sample `count` ((w*h,) each), or with frame=None with the
        last sample_adaptive's result as it lies on the device (the rule: include/mafrix_rt.h,
        mafrixraytracing_amd/temporal.py). Returns (frame, variance, count, accepted), plus the y-major
        RGBA8 post of the frame with want_rgba. cfg: a TemporalConfig, or its fields as keywords
        (tol_depth, tol_normal2, max_history)."""
        cfg = cfg if cfg is not None else TemporalConfig(**tolerances)
        c = MfxTemporalCfg(source=MFX_DN_SRC_ADAPTIVE if frame is None else MFX_DN_SRC_HOST, restart=1 if restart else 0,
                           tol_depth=cfg.tol_depth, tol_normal2=cfg.tol_normal2, max_history=cfg.max_history)
        n = self.w * self.h
        src = var = cnt = None
        if frame is not None:
            src = np.ascontiguousarray(frame, dtype=np.float64)
            assert src.size == n * 4
        if variance is not None:
            var = np.ascontiguousarray(variance, dtype=np.float64)
            assert var.size == n
        if count is not None:
            cnt = np.ascontiguousarray(count, dtype=np.float64)
            assert cnt.size == n
        out = np.empty((n, 4), dtype=np.float64)
        vout = np.empty(n, dtype=np.float64)
        nout = np.empty(n, dtype=np.float64)
        rgba = np.empty(n * 4, dtype=np.uint8) if want_rgba else None
        acc = C.c_int64(-1)
        ms = C.c_double()
        check(self.lib.mfx_temporal(self._h, C.byref(c), dptr(src) if src is not None else None,
                                    dptr(var) if var is not None else None, dptr(cnt) if cnt is not None else None,
                                    dptr(out), dptr(vout), dptr(nout),
                                    rgba.ctypes.data_as(C.POINTER(C.c_uint8)) if want_rgba else None, C.byref(acc),
                                    C.byref(ms)), "mfx_temporal")
        self.last_temporal_ms = ms.value
        return (out, vout, nout, acc.value) + ((rgba,) if want_rgba else ())

    def render_rgba8(self, spp: int = 1, want_pixels: bool = True, out: np.ndarray | None = None) -> np.ndarray | None:
        """Film.GetFrame(spp) + post into `out` (a uint8 buffer of w*h*4, allocated if None), as
        Scene.Render writes its byte[] (mfx_render_rgba8)."""
        if not want_pixels:
            check(self.lib.mfx_render_rgba8(self._h, spp, None), "mfx_render_rgba8")
            return None
        if out is None:
            out = np.empty(self.w * self.h * 4, dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size == self.w * self.h * 4 and out.flags.c_contiguous
        check(self.lib.mfx_render_rgba8(self._h, spp, out.ctypes.data_as(C.POINTER(C.c_uint8))), "mfx_render_rgba8")
        return out

    def reset(self):
        check(self.lib.mfx_reset(self._h), "mfx_reset")

    def film_mean(self) -> np.ndarray:
        frame = np.empty((self.w * self.h, 4), dtype=np.float64)
        check(self.lib.mfx_film_mean(self._h, dptr(frame)), "mfx_film_mean")
        return frame

    # -- lower level ---------------------------------------------------------------------
    def trace_accumulate(self, spp: int, sample_base: int):
        check(self.lib.mfx_trace_accumulate(self._h, spp, sample_base), "mfx_trace_accumulate")

    def accum_reduce(self):
        """Multi-device context: sum the devices' accumulators into devices[0] (mfx_accum_reduce)."""
        check(self.lib.mfx_accum_reduce(self._h), "mfx_accum_reduce")

    def accum_clear(self):
        check(self.lib.mfx_accum_clear(self._h), "mfx_accum_clear")

    def accum_device_ptr(self) -> tuple[int, int]:
        p = C.c_void_p()
        n = C.c_int64()
        check(self.lib.mfx_accum_device_ptr(self._h, C.byref(p), C.byref(n)), "mfx_accum_device_ptr")
        return p.value, n.value

    def accum_attach(self, dptr: int | None, nbytes: int = 0):
        check(self.lib.mfx_accum_attach(self._h, C.c_void_p(dptr) if dptr else None, nbytes), "mfx_accum_attach")

    def accum_read_mean(self, count: float) -> np.ndarray:
        frame = np.empty((self.w * self.h, 4), dtype=np.float64)
        check(self.lib.mfx_accum_read_mean(self._h, float(count), dptr(frame)), "mfx_accum_read_mean")
        return frame

    def sync(self):
        check(self.lib.mfx_sync(self._h), "mfx_sync")

    def stream(self) -> int:
        s = C.c_void_p()
        check(self.lib.mfx_stream(self._h, C.byref(s)), "mfx_stream")
        return s.value or 0

    def ray_counts(self) -> np.ndarray:
        out = np.zeros(16)
        check(self.lib.mfx_ray_counts(self._h, dptr(out)), "mfx_ray_counts")
        return out

    def ray_counts_total(self, reset: bool = True) -> np.ndarray:
        """The ray counters summed over every trace since creation or the last reset
        (mfx_ray_counts_total): no host read between back-to-back traces."""
        out = np.zeros(16)
        check(self.lib.mfx_ray_counts_total(self._h, dptr(out), 1 if reset else 0), "mfx_ray_counts_total")
        return out

    def stats(self) -> tuple[float, float]:
        """(rays traced, device seconds) of the last trace call (mfx_stats)."""
        rays, sec = C.c_double(), C.c_double()
        check(self.lib.mfx_stats(self._h, C.byref(rays), C.byref(sec)), "mfx_stats")
        return rays.value, sec.value

    def last_trace_ms(self) -> float:
        ms = C.c_double()
        check(self.lib.mfx_last_trace_ms(self._h, C.byref(ms)), "mfx_last_trace_ms")
        return ms.value

    def trace_timing(self) -> dict:
        out = np.zeros(8)
        check(self.lib.mfx_trace_timing(self._h, dptr(out)), "mfx_trace_timing")
        return {"total_ms": out[0], "camera_ms": out[1], "extend_ms": out[2], "camera_launches": int(out[3]),
                "shadow_ms": out[4], "iterations": int(out[5]), "launches": int(out[6]), "generations": int(out[7])}

    def closest_hit(self, rays: np.ndarray, tmin: float = 1e-6, tmax: float = 99999999.0):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = len(rays)
        t = np.zeros(n)
        prim = np.zeros(n, dtype=np.int32)
        nrm = np.zeros((n, 3))
        check(self.lib.mfx_closest_hit(self._h, n, dptr(rays), tmin, tmax, dptr(t), iptr(prim), dptr(nrm)),
              "mfx_closest_hit")
        return t, prim, nrm

    def any_hit(self, rays: np.ndarray, tmax: np.ndarray, tmin: float = 1e-6):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        tmax = np.ascontiguousarray(tmax, dtype=np.float64)
        occ = np.zeros(len(rays), dtype=np.int32)
        check(self.lib.mfx_any_hit(self._h, len(rays), dptr(rays), tmin, dptr(tmax), iptr(occ)), "mfx_any_hit")
        return occ

    def build_info(self) -> dict:
        """How the scene was prepared (mfx_build_info): timings, BVH sizes, image digest."""
        out = np.zeros(8)
        dig = C.c_uint64()
        check(self.lib.mfx_build_info(self._h, dptr(out), C.byref(dig)), "mfx_build_info")
        return {"ref_bvh_ms": out[0], "bvh_ms": out[1], "scene_ms": out[2], "gpu_bvh": bool(out[3]),
                "gpu_images": bool(out[3] == 2),
                "nodes4": int(out[4]), "slots": int(out[5]), "nodes2": int(out[6]), "levels": int(out[7]),
                "digest": dig.value}

    def device_info(self) -> dict:
        """How the context's work lies over devices (mfx_device_info): the HIP ordinals, the RCCL
        communicators it created, how mfx_accum_reduce merges, and the primary's tile-row band."""
        out = np.zeros(5 + len(self.devices), dtype=np.int32)
        check(self.lib.mfx_device_info(self._h, iptr(out), len(out)), "mfx_device_info")
        g = int(out[0])
        return {"devices": [int(d) for d in out[5:5 + g]], "communicators": int(out[1]),
                "merge": {0: "none", 1: "rccl_reduce", 2: "ordered_adds"}[int(out[2])],
                "band_index": int(out[3]), "band_count": int(out[4])}

    def launch_info(self) -> dict:
        """What creation chose for the kernels (mfx_launch_info): the traversal-stack bound and its LDS
        shares, the spill flags, top nodes / slots / instance records in LDS, the k_shadow and megakernel
        builds, lit_in_hit, gray_light, camera packets, the grids and the spill buffer's size. The
        flags are bools, the rest ints."""
        out = np.zeros(len(LAUNCH_INFO_KEYS), dtype=np.int32)
        check(self.lib.mfx_launch_info(self._h, iptr(out), len(out)), "mfx_launch_info")
        flags = ("spill_ext", "spill_shd", "lit_in_hit", "gray_light", "camera_packets", "shd_half", "camera_cuts")
        return {k: bool(v) if k in flags else int(v) for k, v in zip(LAUNCH_INFO_KEYS, out)}

    def camera_cut_info(self) -> dict:
        """mfx_camera_cut_info: the last camera-cut build of the primary device."""
        out = np.zeros(32)
        check(self.lib.mfx_camera_cut_info(self._h, dptr(out)), "mfx_camera_cut_info")
        return {"builds": int(out[0]), "build_ms": float(out[1]), "len_sum": int(out[2]), "len_max": int(out[3]),
                "root_tiles": int(out[4]), "empty_tiles": int(out[5]), "tiles": int(out[6]), "cap": int(out[7]),
                "hist": [int(v) for v in out[8:25]], "slots_seen": int(out[25]), "slots_culled": int(out[26]),
                "leaves_dropped": int(out[27]), "leaves_narrowed": int(out[28]), "culled": bool(out[29])}

    def camera_cut_table(self, host: bool = False) -> np.ndarray:
        """mfx_camera_cut_table: the camera-cut table for the current camera as bytes, [tiles][cut_cap][32];
        host=True: the host twin's."""
        n = C.c_int64()
        check(self.lib.mfx_camera_cut_table(self._h, None, 0, C.byref(n), int(host)), "mfx_camera_cut_table")
        out = np.zeros(n.value, dtype=np.uint8)
        check(self.lib.mfx_camera_cut_table(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n), int(host)),
              "mfx_camera_cut_table")
        return out.reshape(-1, self.launch_info()["cut_cap"], 32)

    def light_info(self) -> np.ndarray:
        """mfx_light_info: [0] lights N, [1] 1 if the several-light kernel instances run, [2] bytes of the
        device light table, [3] bytes per path slot the lights add to the pool, [4] / [5] resident blocks
        per CU of the k_shadow / k_resolve instance in use; the rest 0."""
        out = np.zeros(8)
        check(self.lib.mfx_light_info(self._h, dptr(out)), "mfx_light_info")
        return out

    def texture_info(self) -> np.ndarray:
        """mfx_texture_info: [0] textures, [1] 1 if the textured kernel instances run, [2] bytes of texels,
        [3] bytes of the UV table, [4] bytes per path slot the textures add to the pool, [5] / [6] resident
        blocks per CU of the k_shadow / k_resolve instance in use; [7] 0."""
        out = np.zeros(8)
        check(self.lib.mfx_texture_info(self._h, dptr(out)), "mfx_texture_info")
        return out

    def instancing_info(self) -> dict:
        """How instances are traced (mfx_instancing_info): two-level shape and image bytes."""
        out = np.zeros(8)
        check(self.lib.mfx_instancing_info(self._h, dptr(out)), "mfx_instancing_info")
        return {k: int(v) for k, v in zip(INSTANCING_KEYS, out)}

    def ref_leaves(self):
        n = len(self.arrays.prims)
        idx = np.zeros(n, dtype=np.int32)
        lf = np.zeros(n, dtype=np.int32)
        lc = np.zeros(n, dtype=np.int32)
        nl = C.c_int32()
        check(self.lib.mfx_ref_leaves(self._h, iptr(idx), iptr(lf), iptr(lc), C.byref(nl)), "mfx_ref_leaves")
        return idx, lf[:nl.value], lc[:nl.value]


def fp64_selftest(a: np.ndarray, b: np.ndarray, device: int = 0):
    lib = load_library()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    dv = np.zeros_like(a)
    sq = np.zeros_like(a)
    check(lib.mfx_fp64_selftest(device, len(a), dptr(a), dptr(b), dptr(dv), dptr(sq)), "mfx_fp64_selftest")
    return dv, sq


def aabb_selftest(rec: np.ndarray, device: int = 0):
    """(FP64 AABB.hit answers, FP32-screen answers: 1, 0 or -1 = left to FP64, vertex-box proofs:
    1 or 0, plus 2 where the proof's folded and plain forms disagree: never) for n x 24 records
    (mfx_aabb_selftest)."""
    lib = load_library()
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 24)
    out = np.zeros((len(rec), 3), dtype=np.int32)
    check(lib.mfx_aabb_selftest(device, len(rec), dptr(rec), iptr(out)), "mfx_aabb_selftest")
    return out[:, 0], out[:, 1], out[:, 2]


# ---- the reference's object model -----------------------------------------------------------
class Film:
    """Film (Film.fs:13-34): progressive accumulation; here the accumulator lives on the GPU."""

    def __init__(self, ctx: NativeContext):
        self._ctx = ctx
        self.Size = (ctx.w, ctx.h)

    def Reset(self):
        self._ctx.reset()

    def GetFrame(self, integrator: "NativePixelIntegrator", samples: int) -> np.ndarray:
        self._ctx.render_rgba8(samples, want_pixels=False)
        return self._ctx.film_mean()


class NativePixelIntegrator:
    """IPixelIntegrator (IIntegrator.fs:35-40) backed by the GPU: Sample(n) -> Color[w,h] x-major."""

    def __init__(self, ctx: NativeContext):
        self._ctx = ctx

    def Sample(self, n: int) -> np.ndarray:
        return self._ctx.sample(n)

    def SampleAdaptive(self, minSpp: int, maxSpp: int, stepSpp: int, relError: float, absFloor: float):
        """fsharp/Native.fs SampleAdaptive: (Color[w,h] x-major, the tiles' sample counts)."""
        return self._ctx.sample_adaptive(minSpp, maxSpp, stepSpp, relError, absFloor)

    def SampleAdaptiveResume(self, maxSpp: int, stepSpp: int, maxPasses: int, relError: float, absFloor: float):
        """fsharp/Native.fs SampleAdaptiveResume: (Color[w,h] x-major, the tiles' sample counts, tiles still active)."""
        return self._ctx.sample_adaptive_resume(maxSpp, stepSpp, relError, absFloor, max_passes=maxPasses)


class Scene:
    """Scene (Scene.fs:291-333) with the path-tracing hot path on the GPU. Render's one-sample calls
    are served from batches of `render_ahead` samples (the F# binding's DefaultRenderAhead;
    mfx_options.render_ahead): the same bytes per frame as one sample per call."""

    def __init__(self, state, seed: int = DEFAULT_SEED, device: int = 0, max_depth: int = 3,
                 render_ahead: int = DEFAULT_RENDER_AHEAD):
        arrays = state.arrays(max_depth=max_depth) if hasattr(state, "arrays") else state
        self._ctx = NativeContext(arrays, seed=seed, device=device, render_ahead=render_ahead)
        self.width, self.height = arrays.width, arrays.height
        self.film = Film(self._ctx)
        self.pixelIntegrator = NativePixelIntegrator(self._ctx)

    @property
    def ScreenSize(self):
        return (self.width, self.height)

    def Render(self, delta: float, buffer) -> None:
        """Scene.Render(delta, buffer) (Scene.fs:331-333): one 1-spp frame into the film, then
        ACES -> sqrt -> RGBA8 into `buffer` (byte[w*h*4], y-major)."""
        out = self._ctx.render_rgba8(1)
        mv = memoryview(buffer).cast("B")
        mv[:] = out.tobytes()

    def close(self):
        self._ctx.close()
