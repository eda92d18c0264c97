"""ctypes mirror of include/mafrix_rt.h and the loader for libmafrix_rt.so.

This is the Python stand-in for the F# P/Invoke declarations a maintainer adds to
EngineCore/Library.fs: the same structs, the same entry points.
The library is the HIP build for gfx950; there is no CPU fallback — loading fails loudly
if the shared object is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

MFX_PRIM_TRIANGLE = 0
MFX_PRIM_RECT = 1
MFX_PRIM_SPHERE = 2

MFX_F_NONE = 0
MFX_F_COUNT_STATS = 1
MFX_F_MEGAKERNEL = 2
MFX_F_HOST_BVH = 4
MFX_F_WAVEFRONT = 8
MFX_F_FLATTEN = 16
MFX_F_TWO_LEVEL = 32
MFX_F_ROW_PARTITION = 64
MFX_F_IN_FLIGHT = 128
MFX_INSTANCE_VERBATIM = 1
MFX_MAX_DEVICES = 64
MFX_MAX_LIGHTS = 64
MFX_MAX_TEXTURES = 4096
MFX_MAX_TEXTURE_DIM = 16384
MFX_MAX_ENV_SIZE = 4096
MFX_MAX_SKY_LIGHTS = 63
MFX_DN_SRC_HOST = 0
MFX_DN_SRC_ACCUM = 1
MFX_DN_SRC_ADAPTIVE = 2
MFX_DN_SRC_TEMPORAL = 3
MFX_ABI_VERSION = 6
# mfx_launch_info's entries, in order (MFX_LAUNCH_INFO_N of them)
LAUNCH_INFO_KEYS = ("stack_size", "stack_lds_ext", "stack_lds_shd", "spill_ext", "spill_shd", "ntop_ext", "ntop_shd",
                    "nslot_ext", "nslot_shd", "ninst_lds", "shadow_waves", "mega_waves", "lit_in_hit", "gray_light",
                    "camera_packets", "wf_ext_grid", "wf_shd_grid", "wf_cam_grid", "spill_entries_per_lane",
                    "spill_lanes", "chunk", "shd_half", "queue_from", "pool_max", "camera_cuts", "cut_cap",
                    "cut_table_bytes", "cut_len_mean_x1000", "cut_len_max", "cut_root_tiles", "cut_builds", "cut_min_samples")

_HERE = os.path.dirname(os.path.abspath(__file__))
# MFX_LIB_PATH: another build of the same library (scripts' A/B and roof passes on a variant)
LIB_PATH = os.environ.get("MFX_LIB_PATH") or os.path.join(_HERE, "libmafrix_rt.so")


class MfxPrim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("p", (C.c_double * 3) * 4)]


class MfxQuadLight(C.Structure):
    _fields_ = [("p", (C.c_double * 3) * 4), ("normal", C.c_double * 3), ("intensity", C.c_double * 3)]


class MfxPinhole(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("direction", C.c_double * 3),
                ("fov", C.c_double), ("aspect", C.c_double),
                ("topleft", C.c_double * 3), ("right", C.c_double * 3), ("down", C.c_double * 3),
                ("derived", C.c_int32), ("reserved", C.c_int32)]


class MfxSceneDesc(C.Structure):
    _fields_ = [("prims", C.POINTER(MfxPrim)), ("nprims", C.c_int64),
                ("albedo", C.POINTER(C.c_double)), ("nmat", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("max_depth", C.c_int32),
                ("light", MfxQuadLight), ("camera", MfxPinhole)]


class MfxOptions(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("device", C.c_int32), ("flags", C.c_int32),
                ("part_index", C.c_int32), ("part_count", C.c_int32),
                ("ndevices", C.c_int32), ("render_ahead", C.c_int32), ("devices", C.POINTER(C.c_int32))]


class MfxInstance(C.Structure):
    _fields_ = [("first", C.c_int64), ("count", C.c_int64), ("offset", C.c_double * 3),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class MfxTexture(C.Structure):
    """mfx_texture: width * height RGBA8 texels, rows top to bottom."""
    _fields_ = [("rgba", C.POINTER(C.c_uint8)), ("width", C.c_int32), ("height", C.c_int32)]


class MfxPrimUv(C.Structure):
    """mfx_prim_uv: a primitive's texture (-1: none) and the (u, v) of its first three corners."""
    _fields_ = [("texture", C.c_int32), ("reserved", C.c_int32), ("uv", (C.c_double * 2) * 3)]


class MfxEnvironment(C.Structure):
    """mfx_environment: size * size texels of three floats (linear RGB radiance), an octahedral map."""
    _fields_ = [("rgb", C.POINTER(C.c_float)), ("size", C.c_int32), ("reserved", C.c_int32)]


class MfxLens(C.Structure):
    """mfx_lens: the lens radius (world units; 0: no lens) and the distance of the focus plane along the forward axis."""
    _fields_ = [("aperture", C.c_double), ("focus", C.c_double)]


class MfxPrimNormals(C.Structure):
    """mfx_prim_normals: smooth (0: the face normal stays) and the normals of corners p[0], p[1], p[2]."""
    _fields_ = [("smooth", C.c_int32), ("reserved", C.c_int32), ("n", (C.c_double * 3) * 3)]


class MfxAdaptive(C.Structure):
    """mfx_adaptive: the schedule and threshold of mfx_sample_adaptive."""
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("step_spp", C.c_int32), ("reserved", C.c_int32),
                ("rel_error", C.c_double), ("abs_floor", C.c_double)]


class MfxAdaptiveResume(C.Structure):
    """mfx_adaptive_resume: the budget, pass limit and threshold of mfx_sample_adaptive_resume."""
    _fields_ = [("max_spp", C.c_int32), ("step_spp", C.c_int32), ("max_passes", C.c_int32), ("reserved", C.c_int32),
                ("rel_error", C.c_double), ("abs_floor", C.c_double)]


class MfxDenoiseCfg(C.Structure):
    """mfx_denoise_cfg: iterations, source and the four sigmas of mfx_denoise."""
    _fields_ = [("iterations", C.c_int32), ("source", C.c_int32), ("reserved", C.c_int32 * 2),
                ("count", C.c_double), ("sigma_normal", C.c_double), ("sigma_depth", C.c_double),
                ("sigma_albedo", C.c_double), ("sigma_color", C.c_double)]


class MfxDenoiseVarCfg(C.Structure):
    """mfx_denoise_var_cfg: iterations, source, the four sigmas and the luminance floor of mfx_denoise_var."""
    _fields_ = [("iterations", C.c_int32), ("source", C.c_int32), ("reserved", C.c_int32 * 2),
                ("sigma_normal", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double),
                ("sigma_luma", C.c_double), ("luma_floor", C.c_double)]


class MfxTemporalCfg(C.Structure):
    """mfx_temporal_cfg: source, restart, the two tolerances and the history cap of mfx_temporal."""
    _fields_ = [("source", C.c_int32), ("restart", C.c_int32), ("reserved", C.c_int32 * 2),
                ("tol_depth", C.c_double), ("tol_normal2", C.c_double), ("max_history", C.c_double)]


assert C.sizeof(MfxPrim) == 104
assert C.sizeof(MfxInstance) == 48
assert C.sizeof(MfxTexture) == 16
assert C.sizeof(MfxPrimUv) == 56
assert C.sizeof(MfxEnvironment) == 16
assert C.sizeof(MfxPrimNormals) == 80
assert C.sizeof(MfxAdaptive) == 32
assert C.sizeof(MfxAdaptiveResume) == 32
assert C.sizeof(MfxDenoiseCfg) == 56
assert C.sizeof(MfxDenoiseVarCfg) == 56
assert C.sizeof(MfxTemporalCfg) == 40

# numpy structured dtype with the same layout as mfx_prim (for building big prim arrays fast)
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("material", "<i4"), ("p", "<f8", (4, 3))], align=True)
assert PRIM_DTYPE.itemsize == 104
# mfx_instance: template range, translation, flags
INSTANCE_DTYPE = np.dtype([("first", "<i8"), ("count", "<i8"), ("offset", "<f8", (3,)), ("flags", "<i4"),
                           ("reserved", "<i4")], align=True)
assert INSTANCE_DTYPE.itemsize == 48
# mfx_prim_uv: texture index (-1: untextured), (u, v) of p[0], p[1], p[2]
PRIM_UV_DTYPE = np.dtype([("texture", "<i4"), ("reserved", "<i4"), ("uv", "<f8", (3, 2))], align=True)
assert PRIM_UV_DTYPE.itemsize == 56
# mfx_prim_normals: smooth (0: the face normal stays), the normals of p[0], p[1], p[2]
PRIM_NORMALS_DTYPE = np.dtype([("smooth", "<i4"), ("reserved", "<i4"), ("n", "<f8", (3, 3))], align=True)
assert PRIM_NORMALS_DTYPE.itemsize == 80


class SceneArrays:
    """Owns the numpy buffers an MfxSceneDesc points into (keeps them alive).

    prims is the world primitive list (the reference's flat scene). `instancing`, when given, is
    (templates, instances): the same world scene as template primitives and mfx_instance entries
    whose expansion is `prims` (mfx_create_instanced: flattened when the flat image fits the library's
    budget, two-level otherwise). two_level: ask for the two-level traversal regardless
    (MFX_F_TWO_LEVEL)."""

    def __init__(self, prims: np.ndarray, albedo: np.ndarray, light: dict, camera: dict,
                 width: int, height: int, max_depth: int = 3, instancing=None, two_level: bool = False,
                 lights=None, textures=None, prim_uv=None, prim_normals=None):
        self.prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
        # albedo textures ((H, W, 4) uint8 arrays, rows top to bottom) and the primitives' maps (PRIM_UV_DTYPE,
        # one per entry of `prims`; mfx_create_textured), or None: an untextured scene
        self.textures = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures] if textures is not None else None
        self.prim_uv = np.ascontiguousarray(prim_uv, dtype=PRIM_UV_DTYPE) if prim_uv is not None else None
        # corner normals (PRIM_NORMALS_DTYPE, one per entry of `prims`; mfx_set_normals), or None: face normals
        self.prim_normals = np.ascontiguousarray(prim_normals, dtype=PRIM_NORMALS_DTYPE) if prim_normals is not None else None
        self.two_level = bool(two_level)
        # every area light of the scene, in order (light dicts; mfx_create_lights), or None: `light` alone
        self.lights = list(lights) if lights is not None else None
        self.instancing = None
        if instancing is not None:
            self.instancing = (np.ascontiguousarray(instancing[0], dtype=PRIM_DTYPE),
                               np.ascontiguousarray(instancing[1], dtype=INSTANCE_DTYPE))
        self.albedo = np.ascontiguousarray(albedo, dtype=np.float64).reshape(-1, 3)
        self.light = light
        self.camera = camera
        self.width = int(width)
        self.height = int(height)
        self.max_depth = int(max_depth)

    def desc(self, templates: bool = False) -> MfxSceneDesc:
        """templates: point at the instancing template primitives instead of the world list."""
        d = MfxSceneDesc()
        pr = self.instancing[0] if templates else self.prims
        d.prims = pr.ctypes.data_as(C.POINTER(MfxPrim))
        d.nprims = len(pr)
        d.albedo = self.albedo.ctypes.data_as(C.POINTER(C.c_double))
        d.nmat = len(self.albedo)
        d.width, d.height, d.max_depth = self.width, self.height, self.max_depth
        for k in range(4):
            for c in range(3):
                d.light.p[k][c] = float(self.light["p"][k][c])
        for c in range(3):
            d.light.normal[c] = float(self.light["normal"][c])
            d.light.intensity[c] = float(self.light["intensity"][c])
            d.camera.position[c] = float(self.camera["position"][c])
            d.camera.direction[c] = float(self.camera["direction"][c])
        d.camera.fov = float(self.camera["fov"])
        d.camera.aspect = float(self.camera["aspect"])
        return d

    def with_film(self, width: int, height: int) -> "SceneArrays":
        return SceneArrays(self.prims, self.albedo, self.light, self.camera, width, height, self.max_depth,
                           self.instancing, self.two_level, self.lights, self.textures, self.prim_uv, self.prim_normals)

    def flat(self) -> "SceneArrays":
        """The same scene without its instancing (the reference's flat primitive list)."""
        return SceneArrays(self.prims, self.albedo, self.light, self.camera, self.width, self.height,
                           self.max_depth, lights=self.lights, textures=self.textures, prim_uv=self.prim_uv,
                           prim_normals=self.prim_normals)


def quad_lights(lights):
    """A ctypes array of MfxQuadLight from light dicts (p: four corners, normal, intensity)."""
    arr = (MfxQuadLight * max(1, len(lights)))()
    for n, L in enumerate(lights):
        for k in range(4):
            for c in range(3):
                arr[n].p[k][c] = float(L["p"][k][c])
        for c in range(3):
            arr[n].normal[c] = float(L["normal"][c])
            arr[n].intensity[c] = float(L["intensity"][c])
    return arr


def light_table(lights) -> np.ndarray:
    """Host-only: (N, 4) area, 1 / area, pdf_n, 0 of the lights as context creation derives them
    (mfx_light_table; lights.light_table is the numpy statement of the same)."""
    lib = load_library()
    out = np.zeros((max(1, len(lights)), 4))
    check(lib.mfx_light_table(quad_lights(lights), len(lights), dptr(out)), "mfx_light_table")
    return out[:len(lights)]


def texture_structs(textures):
    """A ctypes array of MfxTexture over (H, W, 4) uint8 arrays, and the arrays it points into (keep both
    alive for the call)."""
    keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
    arr = (MfxTexture * max(1, len(keep)))()
    for k, t in enumerate(keep):
        if t.ndim != 3 or t.shape[2] != 4:
            raise ValueError(f"texture {k}: expected an (H, W, 4) uint8 array, got shape {t.shape}")
        arr[k].rgba = t.ctypes.data_as(C.POINTER(C.c_uint8))
        arr[k].height, arr[k].width = t.shape[0], t.shape[1]
    return arr, keep


def uv_table(prims, prim_uv) -> np.ndarray:
    """Host-only: (n, 8) UV records gu[3], cu, gv[3], cv of `prims` as context creation computes them
    (mfx_uv_table; textures.uv_table is the Python statement of the same)."""
    lib = load_library()
    pr = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
    uv = np.ascontiguousarray(prim_uv, dtype=PRIM_UV_DTYPE)
    if len(pr) != len(uv):
        raise ValueError("one prim_uv entry per primitive")
    out = np.zeros((max(1, len(pr)), 8))
    check(lib.mfx_uv_table(pr.ctypes.data_as(C.POINTER(MfxPrim)), len(pr), uv.ctypes.data_as(C.POINTER(MfxPrimUv)),
                           dptr(out)), "mfx_uv_table")
    return out[:len(pr)]


def normal_table(prims, prim_normals) -> np.ndarray:
    """Host-only: (n, 12) normal records g_0[3], k_0, g_1[3], k_1, g_2[3], k_2 of `prims` as mfx_set_normals computes
    them (mfx_normal_table; normals.normal_table is the Python statement of the same)."""
    lib = load_library()
    pr = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
    pn = np.ascontiguousarray(prim_normals, dtype=PRIM_NORMALS_DTYPE)
    if len(pr) != len(pn):
        raise ValueError("one prim_normals entry per primitive")
    out = np.zeros((max(1, len(pr)), 12))
    check(lib.mfx_normal_table(pr.ctypes.data_as(C.POINTER(MfxPrim)), len(pr), pn.ctypes.data_as(C.POINTER(MfxPrimNormals)),
                               dptr(out)), "mfx_normal_table")
    return out[:len(pr)]


def shading_normal(rec, ng, hp) -> np.ndarray:
    """Host-only: (n, 3) shading normals at hit points hp (n, 3) under records rec (n, 12) of vertices whose normal is
    ng (n, 3), by the code the kernels compile (mfx_shading_normal; normals.shading_normal is the Python statement)."""
    lib = load_library()
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 12)
    ng = np.ascontiguousarray(ng, dtype=np.float64).reshape(-1, 3)
    hp = np.ascontiguousarray(hp, dtype=np.float64).reshape(-1, 3)
    if not (len(rec) == len(ng) == len(hp)):
        raise ValueError("shading_normal: one record, normal and hit point per vertex")
    out = np.zeros((max(1, len(rec)), 3))
    check(lib.mfx_shading_normal(len(rec), dptr(rec), dptr(ng), dptr(hp), dptr(out)), "mfx_shading_normal")
    return out[:len(rec)]


def texel_index(sizes, texture: int, uv) -> np.ndarray:
    """Host-only: the texel ids of uv (n, 2) in texture `texture` of textures with (height, width) `sizes`
    (mfx_texel_index: only the sizes are read; textures.texel_index is the Python statement of the same)."""
    lib = load_library()
    arr = (MfxTexture * max(1, len(sizes)))()
    for k, (h, w) in enumerate(sizes):
        arr[k].height, arr[k].width = int(h), int(w)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(max(1, len(uv)), dtype=np.uint32)
    check(lib.mfx_texel_index(arr, len(sizes), texture, len(uv), dptr(uv), out.ctypes.data_as(C.POINTER(C.c_uint32))),
          "mfx_texel_index")
    return out[:len(uv)]


def environment_struct(env):
    """An MfxEnvironment over an (S, S, 3) float32 map (a constant sky may be given as its three values), and
    the array it points into (keep both alive for the call)."""
    keep = np.ascontiguousarray(env, dtype=np.float32)
    if keep.shape == (3,):
        keep = keep.reshape(1, 1, 3)
    if keep.ndim != 3 or keep.shape[0] != keep.shape[1] or keep.shape[2] != 3:
        raise ValueError(f"environment: expected an (S, S, 3) float32 array, got shape {keep.shape}")
    e = MfxEnvironment()
    e.rgb = keep.ctypes.data_as(C.POINTER(C.c_float))
    e.size = keep.shape[0]
    return e, keep


def env_texel_index(dirs, size: int) -> np.ndarray:
    """Host-only: the texel ids of unit directions dirs (n, 3) in a size x size octahedral map
    (mfx_env_texel_index; environment.texel_index is the Python statement of the same)."""
    lib = load_library()
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(max(1, len(d)), dtype=np.uint32)
    check(lib.mfx_env_texel_index(int(size), len(d), dptr(d), out.ctypes.data_as(C.POINTER(C.c_uint32))),
          "mfx_env_texel_index")
    return out[:len(d)]


def env_sample_table(env):
    """Host-only: the sampling table mfx_set_environment_sampled builds from the map env ((S, S, 3) float32):
    (q float32 (n,), alias uint32 (n,), prob float64 (n,)), n = S * S (mfx_env_sample_table)."""
    lib = load_library()
    e, keep = environment_struct(env)
    n = int(e.size) * int(e.size)
    q = np.zeros(n, dtype=np.float32)
    alias = np.zeros(n, dtype=np.uint32)
    prob = np.zeros(n, dtype=np.float64)
    check(lib.mfx_env_sample_table(C.byref(e), q.ctypes.data_as(C.POINTER(C.c_float)),
                                   alias.ctypes.data_as(C.POINTER(C.c_uint32)), dptr(prob)), "mfx_env_sample_table")
    del keep
    return q, alias, prob


def env_sample_direction(size: int, texel, jitter) -> np.ndarray:
    """Host-only: the direction rule of a sampled sky by the code the kernels compile: for texel (n,) and jitter
    (n, 2) = (ju, jv), (n, 4) = the unit direction and len2 * len (mfx_env_sample_direction;
    environment.sample_direction is the Python statement of the same)."""
    lib = load_library()
    t = np.ascontiguousarray(texel, dtype=np.uint32).reshape(-1)
    j = np.ascontiguousarray(jitter, dtype=np.float64).reshape(-1, 2)
    if len(j) != len(t):
        raise ValueError("env_sample_direction: one (ju, jv) per texel")
    out = np.zeros((max(1, len(t)), 4), dtype=np.float64)
    check(lib.mfx_env_sample_direction(int(size), len(t), t.ctypes.data_as(C.POINTER(C.c_uint32)), dptr(j), dptr(out)),
          "mfx_env_sample_direction")
    return out[:len(t)]


def lens_struct(lens) -> "MfxLens":
    """An MfxLens from (aperture, focus); an MfxLens passes through."""
    if isinstance(lens, MfxLens):
        return lens
    aperture, focus = lens
    return MfxLens(aperture=float(aperture), focus=float(focus))


def lens_derive(camera, lens) -> np.ndarray:
    """Host-only: the lens record of `camera` (pinhole_struct's shapes) under lens = (aperture, focus), by the code
    the kernels compile (mfx_lens_derive): U[3], V[3], s (lens.derive is the Python statement of the same)."""
    lib = load_library()
    p, ln = pinhole_struct(camera), lens_struct(lens)
    out = np.zeros(7)
    check(lib.mfx_lens_derive(C.byref(p), C.byref(ln), dptr(out)), "mfx_lens_derive")
    return out


def lens_rays(camera, lens, seed: int, width: int, height: int, px, py, sample):
    """Host-only: the lens camera rays of paths (px[i], py[i], sample[i]) of a width x height film under `seed`, by
    the code the kernels compile (mfx_lens_rays): ((n, 8) float64 = o, d, a, b, (n,) int32 = the trials each took)."""
    lib = load_library()
    p, ln = pinhole_struct(camera), lens_struct(lens)
    x = np.ascontiguousarray(px, dtype=np.int32).reshape(-1)
    y = np.ascontiguousarray(py, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(sample, dtype=np.int64).reshape(-1)
    if not (len(x) == len(y) == len(s)):
        raise ValueError("lens_rays: one px, py and sample per path")
    out = np.zeros((max(1, len(x)), 8))
    trials = np.zeros(max(1, len(x)), dtype=np.int32)
    check(lib.mfx_lens_rays(C.byref(p), C.byref(ln), C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), int(width), int(height), len(x),
                            iptr(x), iptr(y), s.ctypes.data_as(C.POINTER(C.c_int64)), dptr(out), iptr(trials)), "mfx_lens_rays")
    return out[:len(x)], trials[:len(x)]


_P = C.POINTER
_dp = _P(C.c_double)
_ip = _P(C.c_int32)


def _bind(lib, strict: bool = True):
    sig = {
        "mfx_create": (C.c_int, [_P(MfxSceneDesc), _P(MfxOptions), _P(C.c_void_p)]),
        "mfx_create_instanced": (C.c_int, [_P(MfxSceneDesc), _P(MfxInstance), C.c_int32, _P(MfxOptions),
                                           _P(C.c_void_p)]),
        "mfx_create_lights": (C.c_int, [_P(MfxSceneDesc), _P(MfxQuadLight), C.c_int32, _P(MfxInstance), C.c_int32,
                                        _P(MfxOptions), _P(C.c_void_p)]),
        "mfx_create_textured": (C.c_int, [_P(MfxSceneDesc), _P(MfxQuadLight), C.c_int32, _P(MfxInstance), C.c_int32,
                                          _P(MfxTexture), C.c_int32, _P(MfxPrimUv), _P(MfxOptions), _P(C.c_void_p)]),
        "mfx_texture_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_uv_table": (C.c_int, [_P(MfxPrim), C.c_int64, _P(MfxPrimUv), _dp]),
        "mfx_texel_index": (C.c_int, [_P(MfxTexture), C.c_int32, C.c_int32, C.c_int64, _dp, _P(C.c_uint32)]),
        "mfx_light_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_light_table": (C.c_int, [_P(MfxQuadLight), C.c_int32, _dp]),
        "mfx_expand_instances": (C.c_int, [_P(MfxPrim), C.c_int64, _P(MfxInstance), C.c_int32, _P(MfxPrim),
                                           C.c_int64, _P(C.c_int64)]),
        "mfx_instancing_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_build_instanced_info": (C.c_int, [_P(MfxSceneDesc), _P(MfxInstance), C.c_int32, C.c_int32, _dp, _ip]),
        "mfx_destroy": (None, [C.c_void_p]),
        "mfx_sample": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
        "mfx_sample_adaptive": (C.c_int, [C.c_void_p, _P(MfxAdaptive), _dp, _ip, _P(C.c_uint8)]),
        "mfx_sample_adaptive_resume": (C.c_int, [C.c_void_p, _P(MfxAdaptiveResume), _dp, _ip, _P(C.c_uint8), _ip]),
        "mfx_aov": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _dp, _dp]),
        "mfx_denoise": (C.c_int, [C.c_void_p, _P(MfxDenoiseCfg), _dp, _dp, _P(C.c_uint8), _dp]),
        "mfx_denoise_var": (C.c_int, [C.c_void_p, _P(MfxDenoiseVarCfg), _dp, _dp, _dp, _dp, _P(C.c_uint8), _dp]),
        "mfx_temporal": (C.c_int, [C.c_void_p, _P(MfxTemporalCfg), _dp, _dp, _dp, _dp, _dp, _dp, _P(C.c_uint8),
                                   _P(C.c_int64), _dp]),
        "mfx_pinhole_derive": (C.c_int, [_P(MfxPinhole), _dp]),
        "mfx_camera_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_set_camera": (C.c_int, [C.c_void_p, _P(MfxPinhole)]),
        "mfx_set_environment": (C.c_int, [C.c_void_p, _P(MfxEnvironment)]),
        "mfx_environment_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_env_texel_index": (C.c_int, [C.c_int32, C.c_int64, _dp, _P(C.c_uint32)]),
        "mfx_set_environment_sampled": (C.c_int, [C.c_void_p, _P(MfxEnvironment)]),
        "mfx_sky_sampling_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_env_sample_table": (C.c_int, [_P(MfxEnvironment), _P(C.c_float), _P(C.c_uint32), _dp]),
        "mfx_env_sample_direction": (C.c_int, [C.c_int32, C.c_int64, _P(C.c_uint32), _dp, _dp]),
        "mfx_set_lens": (C.c_int, [C.c_void_p, _P(MfxLens)]),
        "mfx_lens_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_lens_derive": (C.c_int, [_P(MfxPinhole), _P(MfxLens), _dp]),
        "mfx_lens_rays": (C.c_int, [_P(MfxPinhole), _P(MfxLens), C.c_uint64, C.c_int32, C.c_int32, C.c_int64, _ip, _ip,
                                    _P(C.c_int64), _dp, _ip]),
        "mfx_set_normals": (C.c_int, [C.c_void_p, _P(MfxPrimNormals), C.c_int64]),
        "mfx_normal_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_normal_table": (C.c_int, [_P(MfxPrim), C.c_int64, _P(MfxPrimNormals), _dp]),
        "mfx_shading_normal": (C.c_int, [C.c_int64, _dp, _dp, _dp, _dp]),
        "mfx_render_rgba8": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_uint8)]),
        "mfx_accumulate_render_rgba8": (C.c_int, [C.c_void_p, C.c_int32, _P(C.c_uint8)]),
        "mfx_stats": (C.c_int, [C.c_void_p, _dp, _dp]),
        "mfx_reset": (C.c_int, [C.c_void_p]),
        "mfx_film_mean": (C.c_int, [C.c_void_p, _dp]),
        "mfx_trace_accumulate": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64]),
        "mfx_accum_clear": (C.c_int, [C.c_void_p]),
        "mfx_accum_reduce": (C.c_int, [C.c_void_p]),
        "mfx_accum_device_ptr": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)]),
        "mfx_accum_read_mean": (C.c_int, [C.c_void_p, C.c_double, _dp]),
        "mfx_accum_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
        "mfx_sync": (C.c_int, [C.c_void_p]),
        "mfx_stream": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
        "mfx_ray_counts": (C.c_int, [C.c_void_p, _dp]),
        "mfx_last_trace_ms": (C.c_int, [C.c_void_p, _dp]),
        "mfx_trace_timing": (C.c_int, [C.c_void_p, _dp]),
        "mfx_ray_counts_total": (C.c_int, [C.c_void_p, _dp, C.c_int32]),
        "mfx_closest_hit": (C.c_int, [C.c_void_p, C.c_int64, _dp, C.c_double, C.c_double, _dp, _ip, _dp]),
        "mfx_any_hit": (C.c_int, [C.c_void_p, C.c_int64, _dp, C.c_double, _dp, _ip]),
        "mfx_ref_leaves": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip]),
        "mfx_fp64_selftest": (C.c_int, [C.c_int32, C.c_int64, _dp, _dp, _dp, _dp]),
        "mfx_aabb_selftest": (C.c_int, [C.c_int32, C.c_int64, _dp, _ip]),
        "mfx_build_leaves": (C.c_int, [_P(MfxSceneDesc), _ip, _ip, _ip, _ip, _ip]),
        "mfx_build_info": (C.c_int, [C.c_void_p, _dp, _P(C.c_uint64)]),
        "mfx_device_info": (C.c_int, [C.c_void_p, _ip, C.c_int32]),
        "mfx_launch_info": (C.c_int, [C.c_void_p, _ip, C.c_int32]),
        "mfx_camera_cut_info": (C.c_int, [C.c_void_p, _dp]),
        "mfx_camera_cut_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int32]),
        "mfx_last_error": (C.c_char_p, []),
        "mfx_abi_version": (C.c_int, []),
        "mfx_device_count": (C.c_int, []),
    }
    for name, (res, args) in sig.items():
        if not strict and not hasattr(lib, name):  # (an older build under A/B: scripts only)
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


EXPORTED_SYMBOLS = [
    "mfx_create", "mfx_create_instanced", "mfx_create_lights", "mfx_light_info", "mfx_light_table", "mfx_create_textured", "mfx_texture_info", "mfx_uv_table", "mfx_texel_index", "mfx_expand_instances", "mfx_instancing_info", "mfx_build_instanced_info", "mfx_destroy", "mfx_sample", "mfx_sample_adaptive", "mfx_sample_adaptive_resume", "mfx_aov", "mfx_denoise", "mfx_denoise_var", "mfx_temporal", "mfx_pinhole_derive", "mfx_camera_info", "mfx_set_camera", "mfx_set_environment", "mfx_environment_info", "mfx_env_texel_index", "mfx_set_environment_sampled", "mfx_sky_sampling_info", "mfx_env_sample_table", "mfx_env_sample_direction", "mfx_set_lens", "mfx_lens_info", "mfx_lens_derive", "mfx_lens_rays", "mfx_set_normals", "mfx_normal_info", "mfx_normal_table", "mfx_shading_normal", "mfx_render_rgba8", "mfx_accumulate_render_rgba8", "mfx_reset",
    "mfx_film_mean", "mfx_stats",
    "mfx_trace_accumulate", "mfx_accum_clear", "mfx_accum_reduce", "mfx_accum_device_ptr", "mfx_accum_attach", "mfx_accum_read_mean",
    "mfx_sync", "mfx_stream", "mfx_ray_counts", "mfx_last_trace_ms", "mfx_trace_timing", "mfx_ray_counts_total", "mfx_closest_hit", "mfx_any_hit", "mfx_ref_leaves",
    "mfx_fp64_selftest", "mfx_aabb_selftest", "mfx_build_leaves", "mfx_build_info", "mfx_device_info", "mfx_launch_info", "mfx_camera_cut_table", "mfx_camera_cut_info", "mfx_last_error", "mfx_abi_version", "mfx_device_count",
]

_lib = None


def load_library(path: str | None = None, strict: bool = True):
    """Load libmafrix_rt.so (the HIP build). Raises if it is missing — no fallback exists.
    strict=False (A/B scripts timing an older build) binds only the entry points it exports."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if path is None and os.environ.get("MFX_LIB_PATH"):
        strict = False  # another build under A/B (an older commit's: bench.py against it as the baseline)
    if not os.path.exists(p):
        raise RuntimeError(f"mafrix_rt native library not built: {p} (run __graft_entry__.build())")
    lib = _bind(C.CDLL(p, mode=C.RTLD_GLOBAL), strict)
    if path is None:
        _lib = lib
    return lib


class MfxError(RuntimeError):
    pass


def check(rc: int, what: str):
    if rc != 0:
        msg = load_library().mfx_last_error()
        raise MfxError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def dptr(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def iptr(a: np.ndarray):
    return a.ctypes.data_as(_ip)


def pinhole_struct(camera) -> MfxPinhole:
    """An MfxPinhole from a camera dict: position, direction, fov, aspect as scene files give them (the
    library runs the constructor), or position, topleft, right, down (derived: taken as they are). An
    MfxPinhole passes through."""
    if isinstance(camera, MfxPinhole):
        return camera
    p = MfxPinhole()
    derived = "topleft" in camera
    for c in range(3):
        p.position[c] = float(camera["position"][c])
        if derived:
            p.topleft[c] = float(camera["topleft"][c])
            p.right[c] = float(camera["right"][c])
            p.down[c] = float(camera["down"][c])
        else:
            p.direction[c] = float(camera["direction"][c])
    if not derived:
        p.fov = float(camera["fov"])
        p.aspect = float(camera["aspect"])
    p.derived = 1 if derived else 0
    return p


def pinhole_derive(camera) -> dict:
    """Host-only: the derived camera the library makes of `camera` (mfx_pinhole_derive): a dict of
    position, topleft, right, down, each a (3,) float64 array."""
    lib = load_library()
    p = pinhole_struct(camera)
    out = np.zeros(12)
    check(lib.mfx_pinhole_derive(C.byref(p), dptr(out)), "mfx_pinhole_derive")
    return {"position": out[0:3].copy(), "topleft": out[3:6].copy(), "right": out[6:9].copy(), "down": out[9:12].copy()}


def build_leaves(arrays: SceneArrays):
    """Host-only: reference leaf grouping + traversal-BVH shape of a scene (no GPU needed)."""
    lib = load_library()
    d = arrays.desc()
    n = len(arrays.prims)
    idx = np.zeros(n, dtype=np.int32)
    lf = np.zeros(n, dtype=np.int32)
    lc = np.zeros(n, dtype=np.int32)
    nl = np.zeros(1, dtype=np.int32)
    info = np.zeros(4, dtype=np.int32)
    check(lib.mfx_build_leaves(C.byref(d), iptr(idx), iptr(lf), iptr(lc), iptr(nl), iptr(info)), "mfx_build_leaves")
    k = int(nl[0])
    return idx, lf[:k], lc[:k], {"clusters": int(info[0]), "nodes": int(info[1]), "stack": int(info[2]),
                                 "slots": int(info[3])}


def expand_instances(templates: np.ndarray, instances: np.ndarray) -> np.ndarray:
    """Host-only: the world primitive list the library derives from an instanced scene."""
    lib = load_library()
    t = np.ascontiguousarray(templates, dtype=PRIM_DTYPE)
    ins = np.ascontiguousarray(instances, dtype=INSTANCE_DTYPE)
    n = C.c_int64()
    tp = t.ctypes.data_as(_P(MfxPrim))
    ip = ins.ctypes.data_as(_P(MfxInstance))
    check(lib.mfx_expand_instances(tp, len(t), ip, len(ins), None, 0, C.byref(n)), "mfx_expand_instances")
    out = np.zeros(n.value, dtype=PRIM_DTYPE)
    check(lib.mfx_expand_instances(tp, len(t), ip, len(ins), out.ctypes.data_as(_P(MfxPrim)), len(out), C.byref(n)),
          "mfx_expand_instances")
    return out


INSTANCING_KEYS = ("instances", "templates", "top_nodes", "template_nodes", "template_slots", "top_slots",
                   "world_slots", "image_bytes")


def build_instanced_info(arrays: SceneArrays, flags: int = 0) -> dict:
    """Host-only: how an instanced scene's traversal images come out (no GPU needed)."""
    lib = load_library()
    d = arrays.desc(templates=True)
    ins = arrays.instancing[1]
    out = np.zeros(8)
    st = np.zeros(1, dtype=np.int32)
    check(lib.mfx_build_instanced_info(C.byref(d), ins.ctypes.data_as(_P(MfxInstance)), len(ins), flags, dptr(out),
                                       iptr(st)), "mfx_build_instanced_info")
    r = {k: int(v) for k, v in zip(INSTANCING_KEYS, out)}
    r["stack"] = int(st[0])
    return r
