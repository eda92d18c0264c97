"""Shared by tests/test_deep_scenes.py (CPU) and tests/test_gpu_stack_shapes.py (GPU): chain scenes whose
binned-SAH trees degenerate, so that the traversal-stack bound (MfxHostScene::stack_entries) goes far
past the bundled scenes' 44, rays that have to pop such a stack to find their hit, and the oracle's
answers (computed once per case and left unchanged).

The chain: template primitive k (k = 0..n-1) sits at x = r^k with size s = rel * x, a triangle
v0 = (x, 0, 0), v1 = (x + s, s, 0), v2 = (x, s, s) (or, spheres=True, every fourth one a sphere of
radius s at v0). Every prefix of the chain is as lopsided as the whole, so the SAH split peels a few
large primitives off a box that still holds all the small ones, again and again. Instance j
(j = 0..m-1) is the whole template translated by (0, 4 * r2^j, 0): the top level over the instances'
boxes is a second such chain, and a two-level bound is the top level's entries at the instance leaf
plus the template's own (mfx_scene.cpp), the deepest case there is.

Only the largest triangles of a chain can be hit (Triangle.Hit culls |divisor| < 1e-6 absolutely, and
the divisor scales with s^2); the deep end is traversed all the same: a ray through the dense end
pushes the large siblings first and pops every one of them on its way to the hit."""
import numpy as np

from conftest import SEED, scene
from test_gpu_edge_parity import edge_rays
from test_gpu_parity import random_rays

W, H = 32, 18
SPP = 2
M_RAYS = 4000
K_LARGE = 20  # chain positions below this count as the large end

# (n, r, rel) flat; (n, r, rel, m, r2) two-level. Bounds from the host builder (tests/test_deep_scenes.py
# asserts the ranges) under these scenes' own cameras: 51, 67, 75, 81.
FLAT51 = (1500, 0.95, 0.02)
TWO67 = (200, 0.7, 0.1, 100, 0.85)
TWO76 = (200, 0.7, 0.1, 200, 0.9)
TWO80 = (400, 0.85, 0.05, 300, 0.9)
SWEEP = [FLAT51, TWO67, TWO80]  # the three scenes of the stack-share, query and megakernel tests
# Built with MFX_LEAF_MAX=1 (one primitive per BVH4 leaf: deeper trees): 93 with 80,000 world primitives,
# the deepest the library accepts (<= 96), and 97 with 199,000, which it refuses. The smallest found
# by scanning n in 50..150, r in 0.5..0.8, rel in 0.001..0.03 and m up to 200,000 / n.
DEEPEST = (100, 0.6, 0.02, 800, 0.8)
REFUSED = (100, 0.6, 0.02, 1990, 0.8)
STACK_MAX = 96  # mfx_create refuses deeper bounds


def stack_bound(a):
    """The traversal-stack bound of a scene from the host builder (no GPU)."""
    from mafrixraytracing_amd.abi import MFX_F_TWO_LEVEL, build_instanced_info, build_leaves
    if a.instancing is None:
        return build_leaves(a)[3]["stack"]
    return build_instanced_info(a, MFX_F_TWO_LEVEL)["stack"]


def _camera(flat):
    """A pinhole at the chain's dense end looking up the chain: every pixel's ray crosses the nested
    boxes around the origin before it reaches the large primitives. A flat chain is seen from the origin
    under the angle rel, so its camera is narrow; the instanced one looks across the instances too."""
    pos, at, fov = ((-0.05, 0.0005, 0.0003), (1.0, 0.012, 0.006), 4.0) if flat else ((-0.12, -0.09, 0.07), (0.5, 0.3, 0.03), 40.0)
    return {"position": pos, "direction": tuple(np.subtract(at, pos)), "fov": fov, "aspect": W / H}


def chain_template(n, r, rel, spheres=False):
    """The n template primitives of a chain (PRIM_DTYPE, material 0)."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE
    p = np.zeros(n, dtype=PRIM_DTYPE)
    x = r ** np.arange(n, dtype=np.float64)
    s = rel * x
    P = p["p"]
    P[:, 0, 0] = x
    P[:, 1, 0], P[:, 1, 1] = x + s, s
    P[:, 2, 0], P[:, 2, 1], P[:, 2, 2] = x, s, s
    if spheres:
        sp = np.arange(n) % 4 == 2
        p["kind"][sp] = 2
        P[sp, 1:] = 0.0
        P[sp, 1, 0] = s[sp]
    return p


def _arrays(prims, instancing=None, two_level=False, max_depth=3):
    from mafrixraytracing_amd.abi import SceneArrays
    base = scene("spot", W, H)
    return SceneArrays(prims, base.albedo[:1], base.light, _camera(instancing is None), W, H, max_depth, instancing,
                       two_level)


def chain_flat(n, r, rel, spheres=False):
    return _arrays(chain_template(n, r, rel, spheres))


def chain_instanced(n, r, rel, m, r2, spheres=False):
    """m translated instances of an n-primitive chain, two-level; .prims is the library's own expansion
    (instance j's primitive k is world primitive j * n + k)."""
    from mafrixraytracing_amd.abi import INSTANCE_DTYPE, expand_instances
    T = chain_template(n, r, rel, spheres)
    I = np.zeros(m, dtype=INSTANCE_DTYPE)
    I["count"] = n
    I["offset"][:, 1] = 4.0 * r2 ** np.arange(m, dtype=np.float64)
    return _arrays(expand_instances(T, I), (T, I), True)


def with_film(a, w, h, narrow=False):
    """The scene on a w x h film; narrow: a 12-degree view from the same position (the builder's box
    padding, and with it the bound, depends on where the camera is) at the x axis, where the instances
    closest to y = 0 pile up."""
    b = a.with_film(w, h)
    b.camera = dict(a.camera, aspect=w / h)
    if narrow:
        b.camera.update(direction=tuple(np.subtract((0.5, 0.005, 0.005), a.camera["position"])), fov=12.0)
    return b


def chain_shape(a):
    """(n, r, rel, offsets): the chain's length, ratio and relative size, and the instances' offsets
    ((1, 3) zeros for a flat chain), read back from the scene."""
    T = a.instancing[0] if a.instancing is not None else a.prims
    off = a.instancing[1]["offset"] if a.instancing is not None else np.zeros((1, 3))
    x = T["p"][:, 0, 0]
    k = np.flatnonzero(T["kind"] == 0)[0]
    return len(T), x[1] / x[0], T["p"][k, 1, 1] / x[k], off


def through_rays(a, n, rng):
    """n rays, (n, 6) origin and unit direction: the first n // 2 aimed through the dense end (each at a
    point within rel of a chain position r^k of the small half of the chain, from an origin outside the
    chain on the small side, along the line to a point inside one of the largest primitives of the same
    instance), then n // 4 random_rays and the rest edge_rays."""
    nt, r, rel, off = chain_shape(a)
    h = n // 2
    q = n // 4
    j = rng.integers(0, len(off), size=h)
    k1 = rng.integers(nt // 2, nt, size=h)
    tgt = np.zeros((h, 3))
    tgt[:, 0] = r ** k1
    tgt += rng.uniform(-rel, rel, size=(h, 3))
    # the far point's primitive: one of the largest, and at least 4 rel away in x, so the ray runs up the chain
    kmax = max(1, min(K_LARGE // 2, int(np.log(4 * rel) / np.log(r)) + 1))
    k0 = rng.integers(0, kmax, size=h)
    x0 = r ** k0
    s0 = rel * x0
    u = rng.uniform(0.15, 0.7, size=h)
    v = rng.uniform(0.15, 0.85 - u)
    far = np.stack([x0 + u * s0, (u + v) * s0, v * s0], axis=1)  # v0 + u (v1 - v0) + v (v2 - v0)
    d = far - tgt
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = tgt - rng.uniform(0.3, 1.5, size=(h, 1)) * d + off[j]
    rays = np.concatenate([np.concatenate([o, d], axis=1), random_rays(a, q, rng), edge_rays(n - h - q, rng, False)])
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    return rays


def chain_index(a, prim):
    """The chain position k of world primitive indices (instance j's primitive k is j * n + k)."""
    return np.asarray(prim) % chain_shape(a)[0]


# ---- the cases, built once --------------------------------------------------------------------------
_scenes = {}
_oracles = {}
_rays = {}
_hits = {}
_images = {}


def deep_scene(key, spheres=False):
    k = (key, spheres)
    if k not in _scenes:
        a = chain_flat(*key, spheres=spheres) if len(key) == 3 else chain_instanced(*key, spheres=spheres)
        a.prims.setflags(write=False)
        _scenes[k] = a
    return _scenes[k]


def oracle_scene(oracle, a):
    if id(a) not in _oracles:
        _oracles[id(a)] = (a, oracle.OracleScene(a.flat()))
    return _oracles[id(a)][1]


def query_rays(key, m=M_RAYS):
    if (key, m) not in _rays:
        rays = through_rays(deep_scene(key), m, np.random.default_rng(4100 + key[0] + len(key)))
        tmax = np.random.default_rng(4200 + key[0]).uniform(0.05, 3.0, size=m)
        rays.setflags(write=False)
        tmax.setflags(write=False)
        _rays[(key, m)] = (rays, tmax)
    return _rays[(key, m)]


def query_answer(oracle, key, m=M_RAYS):
    """The oracle's ((t, prim, normal), occlusion under the random tmax) of a scene's query rays."""
    if (key, m) not in _hits:
        rays, tmax = query_rays(key, m)
        o = oracle_scene(oracle, deep_scene(key))
        r = (o.closest_hit(rays), o.any_hit(rays, tmax))
        for x in r[0] + (r[1],):
            x.setflags(write=False)
        _hits[(key, m)] = r
    return _hits[(key, m)]


ADAPTIVE = (2, 8, 2, 0.3, 0.01)  # min, max, step, rel_error, abs_floor
_adaptive = {}


def adaptive_answer(oracle, key, sched=ADAPTIVE):
    """(tile_spp, mean, rgba8, ray statistics, smallest gap) mfx_sample_adaptive must return on a scene: the
    host rule (mafrixraytracing_amd/adaptive.py) over the oracle's one-sample frames, composed as
    tests/soup_helpers.py's adaptive_answer does."""
    from mafrixraytracing_amd.adaptive import (AdaptiveConfig, luminance, reference_mean, reference_tile_spp,
                                               tile_pixels)
    if (key, sched) in _adaptive:
        return _adaptive[(key, sched)]
    cfg = AdaptiveConfig(*sched)
    a = deep_scene(key)
    w, h = a.width, a.height
    o = oracle_scene(oracle, a)
    frames = np.stack([o.sample(1, SEED, sample_base=s) for s in range(cfg.max_spp)])
    spp, gap = reference_tile_spp(luminance(frames), w, h, cfg)
    mean = reference_mean(frames, spp, w, h)
    px, py, ps = [], [], []
    for ty in range(spp.shape[0]):
        for tx in range(spp.shape[1]):
            p = tile_pixels(w, h, tx, ty)
            n = int(spp[ty, tx])
            px.append(np.repeat(p // h, n))
            py.append(np.repeat(p % h, n))
            ps.append(np.tile(np.arange(n), len(p)))
    st = o.paths(np.concatenate(px), np.concatenate(py), np.concatenate(ps), SEED)[1][:3]
    r = (spp, mean, oracle.post_rgba8(mean, w, h), st, gap)
    for x in r[:4]:
        x.setflags(write=False)
    _adaptive[(key, sched)] = r
    return r


def image_answer(oracle, a, spp=SPP, name=None):
    """The oracle's (frame, stats) of Sample(spp) on a scene (keyed by name, or by the object)."""
    k = (name if name is not None else id(a), a.width, a.height, a.max_depth, spp)
    if k not in _images:
        r = oracle.OracleScene(a.flat()).sample(spp, SEED, with_stats=True)
        for x in r:
            x.setflags(write=False)
        _images[k] = (a, r)
    return _images[k][1]
