"""Shared by tests/test_coordinate_range_reference.py (CPU) and tests/test_gpu_coordinate_range.py (GPU):
scenes whose coordinates lie past or below what binary16 holds, where the per-lane trace kernels' FP16
nodes (mfx_half.h) have planes at +-inf and +-65504 or in the subnormal range, and the oracle's answers
for them (computed once per case and left unchanged).

similar(a, s, off) is the similarity x -> x*s + off applied to everything that has a position: points,
sphere centres, light corners and the camera's position; radii scale by s. The cases are those of
DESIGN.md §3's table of plane shares (scene_digest's `range` lines) less the identity."""
import numpy as np

from conftest import SEED
from soup_helpers import soup_case

IMAGE_SOUP = (777, 40000, 0, True)  # 44x27, with the ground sphere
SPP = 4
# (s, off): beyond 65504 on two axes, on all three at the last finite half itself, by scale, below 6.1e-5
# (subnormal halves), and far enough out that FP32 itself is coarse (an ulp of 1 at 1e7)
CASES = [(1.0, (1e5, 0.0, -7e4)), (1.0, (65504.0, 65504.0, -65504.0)), (1e5, (0.0, 0.0, 0.0)),
         (1e-4, (0.0, 0.0, 0.0)), (1.0, (1e7, 0.0, 0.0))]
TWO_LEVEL_OFF = (1e5, 0.0, -7e4)


def case_id(c):
    s, off = c
    return f"s{s:g}_off" + "_".join(f"{x:g}" for x in off)


def similar_prims(prims, s, off):
    p = prims.copy()
    sp = p["kind"] == 2
    r = p["p"][sp, 1, 0].copy()
    p["p"] = p["p"] * s + np.asarray(off, dtype=np.float64)
    p["p"][sp, 1:] = 0.0
    p["p"][sp, 1, 0] = r * s
    return p


def _moved(q, s, off):
    return [float(v) for v in np.asarray(q, dtype=np.float64) * s + np.asarray(off, dtype=np.float64)]


def similar(a, s, off):
    """The flat scene a under x -> x*s + off: geometry, light and camera together."""
    from mafrixraytracing_amd.abi import SceneArrays
    light = dict(a.light, p=[_moved(q, s, off) for q in a.light["p"]])
    cam = dict(a.camera, position=_moved(a.camera["position"], s, off))
    return SceneArrays(similar_prims(a.prims, s, off), a.albedo, light, cam, a.width, a.height, a.max_depth)


_scenes = {}
_images = {}


def range_scene(c):
    if c not in _scenes:
        b = similar(soup_case(*IMAGE_SOUP), *c)
        b.prims.setflags(write=False)
        _scenes[c] = b
    return _scenes[c]


def range_image(oracle, c, spp=SPP):
    """The oracle's (frame, stats) of Sample(spp) on one case."""
    k = (c, spp)
    if k not in _images:
        r = oracle.OracleScene(range_scene(c)).sample(spp, SEED, with_stats=True)
        for x in r:
            x.setflags(write=False)
        _images[k] = r
    return _images[k]


def moved_instanced_scene(off=TWO_LEVEL_OFF):
    """test_gpu_instancing.instanced_scene(default_rng(21)) moved by off: the loose primitives (verbatim
    entries' templates), every other entry's offset, the light and the camera. The template ranges used
    through an offset stay at local scale, so the template BVHs do; the top level's planes lie at off."""
    from mafrixraytracing_amd.abi import MFX_INSTANCE_VERBATIM, SceneArrays, expand_instances
    from test_gpu_instancing import instanced_scene
    a = instanced_scene(np.random.default_rng(21))
    T, I = a.instancing[0].copy(), a.instancing[1].copy()
    o = np.asarray(off, dtype=np.float64)
    for e in I:
        if e["flags"] & MFX_INSTANCE_VERBATIM:
            f, n = int(e["first"]), int(e["count"])
            T[f:f + n] = similar_prims(T[f:f + n], 1.0, o)
    moved = (I["flags"] & MFX_INSTANCE_VERBATIM) == 0
    I["offset"][moved] = I["offset"][moved] + o
    light = dict(a.light, p=[_moved(q, 1.0, o) for q in a.light["p"]])
    cam = dict(a.camera, position=_moved(a.camera["position"], 1.0, o))
    return SceneArrays(expand_instances(T, I), a.albedo, light, cam, a.width, a.height, instancing=(T, I))
