"""Shared by tests/test_mixed_soup_reference.py (CPU) and tests/test_gpu_mixed_parity.py (GPU): random
soups that mix triangles, rects and spheres with many materials, ray sets aimed at the places where
the three Hit rules differ, the parameter lists both files run, and the oracle's answers for them
(computed once per case and left unchanged).

What the mix is for: Sphere.Hit honours tMax and compares tmin >= tMin but tmax > tMin
(Sphere.fs:33-38), Triangle.Hit ignores tMax (Trangle.fs:148), Rect.Hit tries trig1 and otherwise
trig2 (Rect.fs:26-31), and a reference leaf takes Array.minBy over (hit ? t : tMax) (BvhNode.fs:80):
a leaf holding a sphere and a triangle is the only place where a sphere's miss key meets a triangle's
hit beyond tMax."""
import numpy as np

from conftest import SEED, scene
from test_gpu_edge_parity import edge_rays

W, H = 44, 27  # both sides leave partial 8x8 tiles
PINNED = (0, 255, 256, 32767, 32768)
EPS = (-1e-9, -1e-13, 0.0, 1e-13, 1e-9)
CLASSES = "abcdefg"

# ---- the cases both files run -----------------------------------------------------------------------
QUERY_SOUPS = [(12, 3), (777, 40000), (5000, 65536)]  # (n, nmat)
M_RAYS = 8000
T_DEFAULT = (1e-6, 99999999.0)
T_PAIRS = [T_DEFAULT, (1e-6, 0.3), (0.2, 1.0), (0.0, 99999999.0)]
BUILD_NS = [1, 2, 12, 777, 20000]
# (n, nmat, mat_lo, ground)
IMAGE_SOUPS = [(777, 40000, 0, False), (5000, 65536, 0, False), (777, 40000, 0, True)]
MATERIAL_SOUPS = [(777, 3, 0, False), (777, 257, 0, False), (777, 40000, 0, False), (777, 65536, 0, False),
                  (777, 65536, 32768, False)]
HIGH_MAT = (777, 65536, 32768, False)  # every material has bit 15 set
DEPTHS = [3, 5]
SPP = 4
ADAPTIVE = (2, 8, 2, 0.3, 0.01)  # min, max, step, rel_error, abs_floor


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rand_unit(rng, k):
    return _unit(rng.normal(size=(k, 3)))


def _perp(d, rng):
    """A random unit vector perpendicular to each row of d."""
    u = np.cross(d, rng.normal(size=d.shape))
    return _unit(u)


def mixed_soup(n, rng, nmat, grid=True, rmax=0.2, ground=False, mat_lo=0):
    """~40 % triangles, 30 % rects, 30 % spheres anchored in [-1,1]^3 under spot's camera and light, at
    44x27 and max_depth 3. Rects: v0, v0+e1, v0+e1+e2, v0+e2 with |e| <= 0.15, ~30 % warped (v3 off the
    plane by up to 0.03), a few degenerate (v3 == v2). Spheres: centre v0, radius log-uniform in
    [1e-3, rmax]; the first two have radii 0.0 and 1e-9, a few sit on a triangle's first vertex (with a
    radius that cuts its first edge), a few pairs share centre and radius (equal-t ties), a few are
    concentric. ~10 % of the triangles and rects are flat in y. The last 20 % are exact copies of the
    first 20 %. Materials: mat_lo + integers(0, nmat - mat_lo), with 0, 255, 256, 32767, 32768 and
    nmat-1 pinned (where they lie in [mat_lo, nmat)) on the first primitives, round robin over the first
    n/16 of them; albedo rows all distinct. ground: one more sphere, radius 1000 under the soup."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
    base = scene("spot", W, H)
    p = np.zeros(n, dtype=PRIM_DTYPE)
    kind = rng.choice(3, size=n, p=[0.4, 0.3, 0.3]).astype(np.int32)
    lead = [2, 0, 1, 2, 2, 0, 2, 1, 2, 2]  # small soups hold every kind and the special spheres
    kind[:min(n, len(lead))] = lead[:n]
    v0 = rng.uniform(-1, 1, size=(n, 3))
    if grid:
        v0 = np.round(v0 * 4) / 4
    P = p["p"]
    P[:, 0] = v0
    # triangles (as soup's)
    P[:, 1] = v0 + rng.uniform(-0.05, 0.05, size=(n, 3))
    P[:, 2] = v0 + rng.uniform(-0.05, 0.05, size=(n, 3))
    # rects
    e1 = rng.uniform(-0.15, 0.15, size=(n, 3))
    e2 = rng.uniform(-0.15, 0.15, size=(n, 3))
    warp = rng.random(n) < 0.3
    off = rng.uniform(-0.03, 0.03, size=n) * warp
    degen = rng.random(n) < 0.03
    flat = rng.random(n) < 0.1
    radius = np.exp(rng.uniform(np.log(1e-3), np.log(rmax), size=n))
    is_r = kind == 1
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    P[is_r, 1] = (v0 + e1)[is_r]
    P[is_r, 2] = (v0 + e1 + e2)[is_r]
    P[is_r, 3] = (v0 + e2 + off[:, None] * nrm)[is_r]
    dg = is_r & degen
    P[dg, 3] = P[dg, 2]
    fl = flat & (kind != 2)
    P[fl, :, 1] = P[fl, 0:1, 1]  # flat in y (zero box extent)
    # spheres
    is_s = kind == 2
    P[is_s, 1:] = 0.0
    P[is_s, 1, 0] = radius[is_s]
    nd = int(n * 0.2)
    S = np.flatnonzero(is_s[:n - nd])
    T = np.flatnonzero((kind == 0)[:n - nd])
    if len(S) > 0:  # (in opposite corners of the cube: a ray through one can leave a dense soup unhit)
        P[S[0], 0], P[S[0], 1, 0] = (1.0, 1.0, 1.0), 0.0
    if len(S) > 1:
        P[S[1], 0], P[S[1], 1, 0] = (-1.0, -1.0, -1.0), 1e-9
    k = max(1, len(S) // 25)
    s = 2
    for j in range(k):  # on a triangle's first vertex, cutting its first edge
        if s < len(S) and j < len(T):
            tri = P[T[j]]
            P[S[s], 0] = tri[0]
            P[S[s], 1, 0] = rng.uniform(0.2, 0.8) * np.linalg.norm(tri[1] - tri[0])
            s += 1
    for j in range(k):  # pairs with one centre and radius
        if s + 1 < len(S):
            P[S[s + 1]] = P[S[s]]
            s += 2
    for j in range(k):  # concentric
        if s + 1 < len(S):
            P[S[s + 1], 0] = P[S[s], 0]
            P[S[s + 1], 1, 0] = P[S[s], 1, 0] * rng.uniform(0.3, 0.9)
            s += 2
    p["kind"] = kind
    # materials
    mat = mat_lo + rng.integers(0, nmat - mat_lo, size=n)
    pins = [m for m in dict.fromkeys(PINNED + (nmat - 1,)) if mat_lo <= m < nmat]
    npin = min(n, max(len(pins), n // 16))
    mat[:npin] = [pins[i % len(pins)] for i in range(npin)]
    p["material"] = mat
    p[n - nd:] = p[:nd]  # exact duplicates
    albedo = rng.uniform(0.05, 0.95, size=(nmat, 3))
    if ground:
        g = np.zeros(1, dtype=PRIM_DTYPE)
        g["kind"] = 2
        g["material"] = mat_lo + int(rng.integers(0, nmat - mat_lo))
        g["p"][0, 0] = (0.0, -1001.3, 0.0)
        g["p"][0, 1, 0] = 1000.0
        p = np.concatenate([p, g])
        pts = [np.asarray(base.camera["position"], dtype=np.float64)] + [np.asarray(q, dtype=np.float64)
                                                                          for q in base.light["p"]]
        for q in pts:  # the floor encloses neither the camera nor the light
            assert np.linalg.norm(q - g["p"][0, 0]) > 1000.0 + 1e-3, q
    return SceneArrays(p, albedo, base.light, base.camera, W, H, 3)


def with_depth(a, max_depth):
    from mafrixraytracing_amd.abi import SceneArrays
    return SceneArrays(a.prims, a.albedo, a.light, a.camera, a.width, a.height, max_depth)


def with_materials(a, material):
    """The same scene with another material index per primitive (a host-side remap)."""
    from mafrixraytracing_amd.abi import SceneArrays
    p = a.prims.copy()
    p["material"] = material
    return SceneArrays(p, a.albedo, a.light, a.camera, a.width, a.height, a.max_depth)


def touching(a):
    """(sphere, triangle) index pairs: a sphere of positive radius centred on a triangle's first vertex."""
    p = a.prims
    tri = {}
    for j in np.flatnonzero(p["kind"] == 0):
        tri.setdefault(p["p"][j, 0].tobytes(), j)
    out = []
    for i in np.flatnonzero(p["kind"] == 2):
        j = tri.get(p["p"][i, 0].tobytes())
        if j is not None and 0 < p["p"][i, 1, 0] < 10:
            out.append((i, j))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def _aim(pt, d, back):
    """Rays that reach pt after `back` along the unit direction d."""
    return np.concatenate([pt - back[:, None] * d, d], axis=1)


def mixed_rays(a, m, rng):
    """(rays, classes): m rays split evenly over (a) edge_rays, (b) rays grazing a sphere at
    r*(1+eps), (c) origins inside a sphere, (d) origins on a sphere's surface, leaving and entering,
    (e) rays through a sphere's centre, (f) rays aimed at a rect's shared diagonal, (g) rays aimed at or
    tangent in the point where a vertex-centred sphere cuts its triangle's edge. classes[i] is 0..6."""
    p = a.prims
    P = p["p"]
    sph = np.flatnonzero((p["kind"] == 2) & (P[:, 1, 0] < 10))  # (not the ground)
    rec = np.flatnonzero(p["kind"] == 1)
    tch = touching(a)
    assert len(sph) and len(rec) and len(tch)
    q = m // 7
    out, cls = [], []

    def put(c, r):
        out.append(r)
        cls.append(np.full(len(r), c, dtype=np.int32))

    put(0, edge_rays(m - 6 * q, rng, True))

    def spheres(k):  # random ones; every 16th ray takes one of the first two (radii 0.0 and 1e-9)
        i = sph[rng.integers(0, len(sph), size=k)]
        tiny = np.arange(k) % 16 == 7
        i[tiny] = sph[rng.integers(0, min(2, len(sph)), size=k)][tiny]
        return P[i, 0], P[i, 1, 0], tiny

    def dirs(c, tiny):  # random; at the tiny spheres away from the soup's middle on every axis
        d = _rand_unit(rng, len(c))
        d[tiny] = (np.abs(d) * np.where(c < 0, -1.0, 1.0))[tiny]
        return d

    # (b) grazing: the closest approach to the centre is r*(1+eps)
    c, r, _ = spheres(q)
    d = _rand_unit(rng, q)
    u = _perp(d, rng)
    eps = np.array(EPS)[np.arange(q) % len(EPS)]
    put(1, _aim(c + (r * (1.0 + eps))[:, None] * u, d, rng.uniform(0.1, 2.0, size=q)))
    # (c) inside
    c, r, tiny = spheres(q)
    put(2, np.concatenate([c + (r * rng.uniform(0.0, 0.9, size=q))[:, None] * _rand_unit(rng, q), dirs(c, tiny)], axis=1))
    # (d) on the surface; a third along an axis (where c + r is exact, oc.oc - r*r is exactly 0)
    c, r, _ = spheres(q)
    u = _rand_unit(rng, q)
    ax = np.eye(3)[rng.integers(0, 3, size=q)] * rng.choice([-1.0, 1.0], size=(q, 1))
    third = np.arange(q) % 3 == 0
    u[third] = ax[third]
    d = _rand_unit(rng, q)
    leave = (np.arange(q) // 3) % 2 == 0
    flip = ((d * u).sum(1) > 0) != leave
    d[flip] = -d[flip]
    put(3, np.concatenate([c + r[:, None] * u, d], axis=1))
    # (e) through the centre
    c, r, tiny = spheres(q)
    put(4, _aim(c, dirs(c, tiny), np.where(tiny, rng.uniform(0.01, 0.1, size=q), rng.uniform(0.1, 2.0, size=q))))
    # (f) the rects' shared diagonal v0-v2: the midpoint and other points, exact and 1e-12 to either side
    i = rec[rng.integers(0, len(rec), size=q)]
    v0, v1, v2 = P[i, 0], P[i, 1], P[i, 2]
    s = rng.uniform(0.0, 1.0, size=q)
    s[np.arange(q) % 2 == 0] = 0.5
    s[np.arange(q) % 16 == 1] = 0.0
    s[np.arange(q) % 16 == 3] = 1.0
    diag = v2 - v0
    side = np.cross(np.cross(v1 - v0, diag), diag)  # in trig1's plane, across the diagonal
    side /= np.maximum(np.linalg.norm(side, axis=1, keepdims=True), 1e-300)
    delta = np.array([0.0, 1e-12, -1e-12])[(np.arange(q) // 2) % 3]
    put(5, _aim(v0 + s[:, None] * diag + delta[:, None] * side, _rand_unit(rng, q), rng.uniform(0.1, 2.0, size=q)))
    # (g) where a vertex-centred sphere cuts its triangle's first edge: aimed at it, and tangent in it
    j = tch[rng.integers(0, len(tch), size=q)]
    c, r = P[j[:, 0], 0], P[j[:, 0], 1, 0]
    e = _unit(P[j[:, 1], 1] - P[j[:, 1], 0])
    pt = c + r[:, None] * e
    d = _rand_unit(rng, q)
    tang = np.arange(q) % 2 == 0
    d[tang] = _perp(e, rng)[tang]
    put(6, _aim(pt, d, rng.uniform(0.1, 2.0, size=q)))
    rays = np.concatenate(out)
    rays[:, 3:] = _unit(rays[:, 3:])
    return rays, np.concatenate(cls)


# ---- the cases, built once --------------------------------------------------------------------------
_soups = {}
_cases = {}
_answers = {}
_images = {}
_oracles = {}


def soup_case(n, nmat, mat_lo=0, ground=False):
    """The soup of one parameter tuple (geometry depends on n alone: the materials are drawn last)."""
    key = (n, nmat, mat_lo, ground)
    if key not in _soups:
        a = mixed_soup(n, np.random.default_rng(7000 + n), nmat, grid=n != 5000, ground=ground, mat_lo=mat_lo)
        a.prims.setflags(write=False)
        a.albedo.setflags(write=False)
        _soups[key] = a
    return _soups[key]


def oracle_scene(oracle, a):
    k = id(a)
    if k not in _oracles:
        _oracles[k] = (a, oracle.OracleScene(a))
    return _oracles[k][1]


def query_case(n, nmat):
    """(soup, rays, classes) of one QUERY_SOUPS entry."""
    key = (n, nmat)
    if key not in _cases:
        a = soup_case(n, nmat)
        rays, cls = mixed_rays(a, M_RAYS, np.random.default_rng(8000 + n))
        rays.setflags(write=False)
        _cases[key] = (a, rays, cls)
    return _cases[key]


def query_answer(oracle, n, nmat, tpair):
    """The oracle's (t, prim, normal) of a query case at one (tmin, tmax)."""
    key = (n, nmat, tpair)
    if key not in _answers:
        a, rays, _ = query_case(n, nmat)
        r = oracle_scene(oracle, a).closest_hit(rays, tmin=tpair[0], tmax=tpair[1])
        for x in r:
            x.setflags(write=False)
        _answers[key] = r
    return _answers[key]


def image_answer(oracle, key, max_depth=3, spp=SPP):
    """The oracle's (frame, stats) of Sample(spp) on one soup tuple."""
    k = (key, max_depth, spp)
    if k not in _images:
        a = with_depth(soup_case(*key), max_depth)
        r = oracle.OracleScene(a).sample(spp, SEED, with_stats=True)
        for x in r:
            x.setflags(write=False)
        _images[k] = r
    return _images[k]


def scaled(a, rays, s, offset):
    """The soup's points and sphere centres times s plus offset, radii times s; the rays alike."""
    from mafrixraytracing_amd.abi import SceneArrays
    p = a.prims.copy()
    sp = p["kind"] == 2
    r = p["p"][sp, 1, 0].copy()
    p["p"] = p["p"] * s + offset
    p["p"][sp, 1:] = 0.0
    p["p"][sp, 1, 0] = r * s
    b = SceneArrays(p, a.albedo, a.light, a.camera, a.width, a.height, a.max_depth)
    rr = np.array(rays)
    rr[:, :3] = rr[:, :3] * s + offset
    return b, rr


_adaptive = {}


def adaptive_answer(oracle, key, sched=ADAPTIVE):
    """(tile_spp, mean, rgba8, ray statistics, smallest gap) mfx_sample_adaptive must return on one soup
    tuple: the host rule (mafrixraytracing_amd/adaptive.py) over the oracle's one-sample frames, as
    tests/test_gpu_adaptive.py's reference() composes it for the named scenes."""
    from mafrixraytracing_amd.adaptive import (AdaptiveConfig, luminance, reference_mean, reference_tile_spp,
                                               tile_pixels)
    k = (key, sched)
    if k in _adaptive:
        return _adaptive[k]
    cfg = AdaptiveConfig(*sched)
    a = soup_case(*key)
    o = oracle_scene(oracle, a)
    frames = np.stack([o.sample(1, SEED, sample_base=s) for s in range(cfg.max_spp)])
    spp, gap = reference_tile_spp(luminance(frames), W, H, cfg)
    mean = reference_mean(frames, spp, W, H)
    px, py, ps = [], [], []
    for ty in range(spp.shape[0]):
        for tx in range(spp.shape[1]):
            p = tile_pixels(W, H, tx, ty)
            n = int(spp[ty, tx])
            px.append(np.repeat(p // H, n))
            py.append(np.repeat(p % H, n))
            ps.append(np.tile(np.arange(n), len(p)))
    st = o.paths(np.concatenate(px), np.concatenate(py), np.concatenate(ps), SEED)[1][:3]
    r = (spp, mean, oracle.post_rgba8(mean, W, H), st, gap)
    for x in r[:4]:
        x.setflags(write=False)
    _adaptive[k] = r
    return r


_occl = {}


def any_hit_sets(oracle, n, nmat):
    """[(name, rays, tmax, the oracle's occlusion)] of one query case: random tmax, and tmax at, one
    ulp around and 1e-12 around the default closest hit's t for the rays that hit."""
    key = (n, nmat)
    if key not in _occl:
        a, rays, _ = query_case(n, nmat)
        o = oracle_scene(oracle, a)
        t0, p0, _ = query_answer(oracle, n, nmat, T_DEFAULT)
        hit = p0 >= 0
        sets = [("random", rays, np.random.default_rng(9000 + n).uniform(0.05, 3.0, size=len(rays)))]
        for name, tm in (("t0", t0), ("nextafter up", np.nextafter(t0, np.inf)),
                         ("nextafter down", np.nextafter(t0, -np.inf)), ("t0 (1 + 1e-12)", t0 * (1 + 1e-12)),
                         ("t0 (1 - 1e-12)", t0 * (1 - 1e-12))):
            sets.append((name, rays[hit], tm[hit]))
        _occl[key] = [(name, rr, tm, o.any_hit(rr, tm)) for name, rr, tm in sets]
    return _occl[key]


def far_case(s, offset):
    """The 777 query soup and its rays scaled by s and moved by offset, with random tmax."""
    a, rays, _ = query_case(777, 40000)
    b, rr = scaled(a, rays, s, offset)
    return a, b, rr, np.random.default_rng(9500).uniform(0.05, 3.0, size=len(rr)) * s


# (s, offset); from the third on the coordinates leave what binary16 holds (past 65504, or below 6.1e-5):
# the query kernels walk the FP32 nodes, tests/range_helpers.py has the images on the FP16 ones
FAR = [(1e3, 5e3), (1.0, 3e4), (1.0, 1e5), (1.0, (1e5, 0.0, -7e4)), (1.0, (65504.0, 65504.0, -65504.0)), (1e5, 0.0),
       (1e-4, 0.0), (1.0, 1e7)]


def moved_two_spheres_plane():
    """two_spheres_plane at 48x27 moved (1e4, -3e3, 2e4) away, geometry, light and camera together (a
    sphere's centre moves; its radius in p[1] does not)."""
    from mafrixraytracing_amd.abi import SceneArrays
    a = scene("two_spheres_plane", 48, 27)
    off = np.array([1e4, -3e3, 2e4])
    prims = a.prims.copy()
    sp = prims["kind"] == 2
    assert sp.any() and not sp.all()
    prims["p"][~sp] = prims["p"][~sp] + off
    prims["p"][sp, 0] = prims["p"][sp, 0] + off
    light = dict(a.light, p=[list(np.asarray(q) + off) for q in a.light["p"]])
    cam = dict(a.camera, position=list(np.asarray(a.camera["position"]) + off))
    return SceneArrays(prims, a.albedo, light, cam, a.width, a.height, a.max_depth)


def beyond_tmax_case():
    """(scene, rays, tmax): two large triangles in one reference leaf, in the planes z = 4.5 and x = 4.6,
    and rays along (1, 0, 1)/sqrt(2) from (-1, y, -1). The leaf's box [0,10]x[0,1]x[0,10] is entered at
    t = sqrt(2), each triangle's own (flat) box only where the ray hits it, at t = 7.78 and 7.92. With tMax
    in between, Bvh.Hit reports the hit at 7.78: the leaf's box test passes and, every primitive being hit
    (Triangle.Hit ignores tMax), Array.minBy has no miss key (BvhNode.fs:64-80). Rays at y = 0.9 miss the
    first triangle (its miss key tMax wins) and tMax = 1 lies before the leaf's box: no hit there."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
    base = scene("spot", W, H)
    p = np.zeros(2, dtype=PRIM_DTYPE)
    p["p"][0, :3] = [(0, 0, 4.5), (10, 0, 4.5), (0, 1, 4.5)]
    p["p"][1, :3] = [(4.6, 0, 0), (4.6, 0, 10), (4.6, 1, 0)]
    a = SceneArrays(p, base.albedo[:1], base.light, base.camera, W, H)
    d = np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0)
    rays, tmax = [], []
    for y in (0.1, 0.3, 0.45, 0.9):
        for tm in (1.0, 2.0, 5.0, 7.7, 7.8, 7.95, 100.0):
            rays.append(np.concatenate([[-1.0, y, -1.0], d]))
            tmax.append(tm)
    return a, np.array(rays), np.array(tmax)


def beyond_light_scene():
    """The same through shadow rays (tmax = dist - 1e-6, Integrators.fs:44): a floor of two triangles under
    spot's light (y = 2.2), and behind the light one reference leaf of two large triangles, in the planes
    y = 4 and x = 0.9 (the latter from y = 0.5 up, so the leaf's box starts below the light). A shadow ray
    that leaves the floor towards +x crosses x = 0.9 and y = 4 only beyond the light, yet Bvh.Hit reports
    it occluded: the floor is darker than physics would have it, and the GPU image must be too."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
    base = scene("spot", W, H)
    p = np.zeros(4, dtype=PRIM_DTYPE)
    p["p"][0, :3] = [(-2, 0, -2), (2, 0, -2), (2, 0, 2)]
    p["p"][1, :3] = [(-2, 0, -2), (2, 0, 2), (-2, 0, 2)]
    p["p"][2, :3] = [(-30, 4, -30), (30, 4, -30), (0, 4, 40)]
    p["p"][3, :3] = [(0.9, 0.5, -20), (0.9, 0.5, 20), (0.9, 60, 0)]
    p["material"] = [0, 0, 1, 1]
    return SceneArrays(p, base.albedo[:2], base.light, base.camera, W, H)


def floor_shadow_rays(a, k=24):
    """Shadow rays from a k x k grid of floor points to the light's centre: (rays, tmax)."""
    L = np.asarray(a.light["p"], dtype=np.float64).mean(0)
    g = (np.arange(k) + 0.5) / k * 3.6 - 1.8
    f = np.array([(x, 0.0, z) for x in g for z in g])
    to = L - f
    dist = np.linalg.norm(to, axis=1)
    return np.concatenate([f, to / dist[:, None]], axis=1), dist - 1e-6
