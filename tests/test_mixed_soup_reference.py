"""The conditions under which tests/test_gpu_mixed_parity.py means something, asserted on the CPU
oracle alone for exactly the soups and ray sets that file uses (tests/soup_helpers.py holds both):
every ray class hits and misses, the closest hits cover all three kinds, a rect's second triangle and
an equal-t tie, the non-default (tmin, tmax) pairs change answers (with a triangle hit returned
beyond tMax), the images are lit with bounce and shadow rays, and the many-material image depends on
all 16 bits of the material index. Last, Sphere.Hit (Sphere.fs:21-43) restated in plain Python floats
pins the oracle where the GPU tests lean on it."""
import math

import numpy as np
import pytest

from soup_helpers import (CLASSES, DEPTHS, EPS, FAR, HIGH_MAT, IMAGE_SOUPS, MATERIAL_SOUPS, QUERY_SOUPS, T_DEFAULT, T_PAIRS,
                          adaptive_answer, any_hit_sets, beyond_light_scene, beyond_tmax_case, far_case,
                          floor_shadow_rays, image_answer, mixed_rays, moved_two_spheres_plane,
                          oracle_scene, query_answer, query_case, soup_case, touching, with_materials)


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
def test_soup_shape(n, nmat):
    a, rays, cls = query_case(n, nmat)
    p = a.prims
    k = p["kind"]
    assert set(k.tolist()) == {0, 1, 2}
    if n >= 100:
        frac = np.bincount(k) / n
        assert np.all(np.abs(frac - [0.4, 0.3, 0.3]) < 0.06), frac
    r = p["p"][k == 2][:, 1, 0]
    assert r[0] == 0.0 and r[1] == 1e-9 and r.max() <= 0.2
    assert len(touching(a)) >= 1
    m = p["material"]
    assert m.min() >= 0 and m.max() == nmat - 1
    for pin in (0, 255, 256, 32767, 32768, nmat - 1):
        if pin < nmat:
            assert (m == pin).any(), pin
    assert len(np.unique(a.albedo, axis=0)) == nmat
    nd = int(n * 0.2)
    assert p[n - nd:].tobytes() == p[:nd].tobytes()
    assert len(rays) == len(cls) == 8000 and np.abs(np.linalg.norm(rays[:, 3:], axis=1) - 1).max() < 1e-12
    assert np.bincount(cls).min() >= 8000 // 7


@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
def test_every_ray_class_hits_and_misses(oracle, n, nmat):
    a, rays, cls = query_case(n, nmat)
    t, prim, _ = query_answer(oracle, n, nmat, T_DEFAULT)
    hit = prim >= 0
    for c in range(7):
        m = cls == c
        assert hit[m].any() and (~hit[m]).any(), (CLASSES[c], hit[m].sum(), (~hit[m]).sum())
    b = np.flatnonzero(cls == 1)
    eps = np.array(EPS)[np.arange(len(b)) % len(EPS)]
    hb = hit[b][eps != 0.0]
    assert hb.any() and (~hb).any()


@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
def test_closest_hits_cover_kinds_second_triangles_and_ties(oracle, n, nmat):
    from mafrixraytracing_amd.abi import SceneArrays
    a, rays, cls = query_case(n, nmat)
    t, prim, _ = query_answer(oracle, n, nmat, T_DEFAULT)
    hit = prim >= 0
    kinds = a.prims["kind"]
    assert set(kinds[prim[hit]].tolist()) == {0, 1, 2}
    # a rect hit taken by trig2: the rects' first triangles alone do not give that t
    first = a.prims[kinds == 1].copy()
    first["kind"] = 0
    o1 = oracle.OracleScene(SceneArrays(first, a.albedo, a.light, a.camera, a.width, a.height))
    on_rect = np.flatnonzero(hit & (kinds[np.where(hit, prim, 0)] == 1))
    t1, p1, _ = o1.closest_hit(rays[on_rect])
    second = (p1 < 0) | (t1 != t[on_rect])
    assert second.any() and (~second).any(), (second.sum(), len(on_rect))
    # an equal-t tie: without the winning primitive the same t is found again
    ties = 0
    nd = int(n * 0.2)  # rays won by a primitive that has an exact copy first
    order = np.flatnonzero(hit)
    order = order[np.argsort(~((prim[order] < nd) | (prim[order] >= n - nd)), kind="stable")]
    for i in order[:400]:
        rest = np.delete(a.prims, prim[i])
        o2 = oracle.OracleScene(SceneArrays(rest, a.albedo, a.light, a.camera, a.width, a.height))
        t2, p2, _ = o2.closest_hit(rays[i:i + 1])
        ties += int(p2[0] >= 0 and t2[0] == t[i])
        if ties and n > 12:
            break
    assert ties >= 1
    # a reference leaf that holds a sphere and a triangle or rect
    idx, lf, lc = oracle_scene(oracle, a).bvh_leaves()
    mixed = sum(1 for f, c in zip(lf, lc) if len({min(int(kinds[j]), 1) for j in idx[f:f + c]}) == 2)
    assert mixed >= 1
    print(f"n={n}: {second.sum()} of {len(on_rect)} rect hits by trig2, {mixed} of {len(lf)} leaves mix kinds")


@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
@pytest.mark.parametrize("tpair", T_PAIRS[1:], ids=_ids)
def test_tmin_tmax_pairs_change_answers(oracle, n, nmat, tpair):
    a, rays, cls = query_case(n, nmat)
    t0, p0, _ = query_answer(oracle, n, nmat, T_DEFAULT)
    t, p, _ = query_answer(oracle, n, nmat, tpair)
    assert ((t != t0) | (p != p0)).mean() >= 0.01
    hit = p >= 0
    kinds = a.prims["kind"][np.where(hit, p, 0)]
    if tpair == (1e-6, 0.3) and n == 5000:  # Triangle.Hit ignores tMax: hits are returned beyond it
        beyond = hit & (t >= tpair[1])
        assert beyond.sum() >= 1 and np.all(kinds[beyond] != 2)
        print(f"{beyond.sum()} hits at t >= tmax")
    if tpair[0] == 0.0:  # tmn >= tMin with tMin = 0: a sphere hit at exactly t = 0 (origin on the surface)
        assert (hit & (t == 0.0) & (kinds == 2)).any()
    assert np.all(t[hit & (kinds == 2)] < tpair[1])  # Sphere.Hit honours tMax


IMAGE_CASES = sorted({(k, d) for k in IMAGE_SOUPS + MATERIAL_SOUPS for d in DEPTHS})


@pytest.mark.parametrize("key,depth", IMAGE_CASES, ids=_ids)
def test_images_are_lit_and_bounce(oracle, key, depth):
    frame, st = image_answer(oracle, key, depth)
    assert (frame[:, :3].sum(1) != 0).mean() > 0.05
    assert st[0] == 44 * 27 * 4 and st[1] > 0 and st[2] > 0
    if key[3]:  # the floor: most paths go on
        assert st[1] > st[0]
    if depth == 5:  # vertices beyond the fourth exist
        assert st[1] > image_answer(oracle, key, 3)[1][1]
    one, st1 = image_answer(oracle, key, depth, spp=1)  # the megakernel's bit-for-bit case
    assert (one[:, :3].sum(1) != 0).mean() > 0.05 and st1[1] > 0 and st1[2] > 0


def test_many_material_image_needs_all_16_bits(oracle):
    from conftest import SEED
    a = soup_case(*HIGH_MAT)
    m = a.prims["material"]
    assert m.min() >= 32768 and (m == 32768).any() and (m == 65535).any()
    ref, _ = image_answer(oracle, HIGH_MAT, 3)
    lit = ref[:, :3].sum(1) != 0
    for name, f in (("& 0xff", m & 0xFF), ("& 0x7fff", m & 0x7FFF), ("- 65536 clamped", np.maximum(m - 65536, 0))):
        img = oracle.OracleScene(with_materials(a, f)).sample(4, SEED)
        assert not np.array_equal(img, ref), name
        assert np.all(np.any(img[lit, :3] != ref[lit, :3], axis=1)), name  # every lit pixel differs


@pytest.mark.parametrize("nmat", [257, 40000])
def test_material_256_is_seen(oracle, nmat):
    """The first material read from global memory (k_resolve keeps rows 0..255 in LDS) matters to the image."""
    from conftest import SEED
    key = (777, nmat, 0, False)
    a = soup_case(*key)
    m = a.prims["material"]
    for depth in (3,):
        ref, _ = image_answer(oracle, key, depth)
        img = oracle.OracleScene(with_materials(a, np.where(m == 256, 255, m))).sample(4, SEED)
        assert not np.array_equal(img, ref)


def test_adaptive_case_has_several_tile_counts(oracle):
    spp, mean, rgba, st, gap = adaptive_answer(oracle, HIGH_MAT)
    assert len(set(spp.ravel().tolist())) > 1 and gap > 1e-6, (spp.tolist(), gap)


@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
def test_any_hit_sets_have_both_answers(oracle, n, nmat):
    a, rays, cls = query_case(n, nmat)
    for name, rr, tm, occ in any_hit_sets(oracle, n, nmat):
        print(f"n={n} {name}: {occ.sum()} of {len(occ)} occluded")
        if name in ("random", "t0", "nextafter up", "t0 (1 + 1e-12)"):
            assert 0 < occ.sum() < len(occ), name
    # tmax exactly at the closest t: a sphere's t < tMax fails, a triangle's hit stands (it ignores tMax)
    name, rr, tm, occ = any_hit_sets(oracle, n, nmat)[1]
    t0, p0, _ = query_answer(oracle, n, nmat, T_DEFAULT)
    kinds = a.prims["kind"][p0[p0 >= 0]]
    assert occ[kinds != 2].any() and (occ[kinds == 2] == 0).any()


@pytest.mark.parametrize("s,offset", FAR)
def test_far_cases_hit(oracle, s, offset):
    a, b, rr, tmax = far_case(s, offset)
    o = oracle.OracleScene(b)
    t, prim, _ = o.closest_hit(rr)
    occ = o.any_hit(rr, tmax)
    print(f"s={s} offset={offset}: hit share {(prim >= 0).mean():.3f}, sphere hits {(a.prims['kind'][prim[prim >= 0]] == 2).sum()}")
    assert (prim >= 0).mean() > 0.01 and 0 < occ.sum() < len(occ)
    # Triangle.Hit culls |div| < 1e-6 absolutely (Trangle.fs:120-155), and div is a product of two edges:
    # at s = 1e-4 the soup's edges are below 3e-5, so no triangle or rect can be hit there, only spheres
    assert set(a.prims["kind"][prim[prim >= 0]].tolist()) == ({2} if s == 1e-4 else {0, 1, 2})


def test_moved_sphere_scene_is_lit(oracle):
    from conftest import SEED
    ref, st = oracle.OracleScene(moved_two_spheres_plane()).sample(4, SEED, with_stats=True)
    assert (ref[:, :3].sum(1) != 0).mean() > 0.05 and st[1] > 0 and st[2] > 0


def test_feature_case_has_silhouettes(oracle):
    from denoise_helpers import scene_features
    f = scene_features(oracle, soup_case(*HIGH_MAT), 3, 5)
    frac = f[:, 7]
    assert ((frac > 0) & (frac < 1)).any() and (frac == 0).any() and (frac == 1).any()
    assert np.array_equal(f[frac == 0], np.zeros(((frac == 0).sum(), 8)))


def test_beyond_tmax_case_is_what_it_says(oracle):
    """A leaf entered before tMax whose primitives are all hit beyond it is a hit, and neither primitive's
    own box passes AABB.hit at that tMax (a search that culls primitive boxes at tMax never tests them)."""
    a, rays, tmax = beyond_tmax_case()
    o = oracle.OracleScene(a)
    idx, lf, lc = o.bvh_leaves()
    assert lc.tolist() == [2]
    occ = o.any_hit(rays, tmax)
    P = a.prims["p"][:, :3]
    for i, (r, tm) in enumerate(zip(rays, tmax)):
        t, prim, _ = o.closest_hit(r[None], tmax=tm)
        want = r[1] < 0.5 and tm >= 2.0
        assert occ[i] == want and (prim[0] == 0) == want, (i, r[1], tm)
        if want:
            assert t[0] == oracle.kat_prim_hit(0, P[0], r[:3], r[3:], 1e-6, tm)[1] and 7.7 < t[0] < 7.8
        if want and tm <= 7.7:
            assert t[0] > tm
            assert oracle.kat_aabb(P.min((0, 1)), P.max((0, 1)), r[:3], r[3:], 1e-6, tm)
            assert not any(oracle.kat_aabb(P[k].min(0), P[k].max(0), r[:3], r[3:], 1e-6, tm) for k in range(2))


def test_beyond_light_scene_is_what_it_says(oracle):
    from conftest import SEED
    a = beyond_light_scene()
    o = oracle.OracleScene(a)
    idx, lf, lc = o.bvh_leaves()
    assert sorted(sorted(idx[f:f + c].tolist()) for f, c in zip(lf, lc)) == [[0, 1], [2, 3]]
    rays, tmax = floor_shadow_rays(a)
    occ = o.any_hit(rays, tmax)
    P = a.prims["p"][:, :3]
    quirk = 0
    for i in np.flatnonzero(occ):
        r = rays[i]
        hits = [oracle.kat_prim_hit(0, P[k], r[:3], r[3:], 1e-6, tmax[i]) for k in (2, 3)]
        if all(h[0] and h[1] > tmax[i] for h in hits):  # occluded by hits beyond the light alone
            quirk += 1
            assert not any(oracle.kat_aabb(P[k].min(0), P[k].max(0), r[:3], r[3:], 1e-6, tmax[i]) for k in (2, 3))
    assert quirk > 20 and 0 < occ.sum() < len(occ), (quirk, occ.sum())
    frame, st = o.sample(4, SEED, with_stats=True)
    assert (frame[:, :3].sum(1) != 0).mean() > 0.05 and st[1] > 0 and st[2] > 0
    # with the plane y = 4 out of reach the image changes: the occlusion above is in it
    b = beyond_light_scene()
    b.prims["p"][2, :3, 1] = 1000.0
    assert np.any(oracle.OracleScene(b).sample(4, SEED) != frame, axis=1).mean() > 0.05
    print(f"{quirk} of {len(occ)} floor points shadowed by hits beyond the light alone")


# ---- Sphere.Hit in plain floats ----------------------------------------------------------------------
def sphere_hit(c, r, o, d, tMin, tMax):
    """Sphere.fs:21-43, one rounding per operation: (hit, t)."""
    oc = [o[0] - c[0], o[1] - c[1], o[2] - c[2]]
    dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]  # noqa: E731 (Vector.Dot's order)
    a = 1.0
    b = 2.0 * dot(oc, d)
    cc = dot(oc, oc) - r * r
    disc = b * b - 4.0 * a * cc
    if disc > 0:
        root = math.sqrt(disc)
        q = -0.5 * (b - root) if b < 0.0 else -0.5 * (b + root)
        t0 = q
        t1 = cc / q if q != 0.0 else (math.nan if cc == 0.0 else math.copysign(math.inf, cc) * math.copysign(1.0, q))
        tmn, tmx = (t0 if t0 < t1 else t1), (t0 if t0 > t1 else t1)
        if tmn >= tMin and tmn < tMax:
            return True, tmn
        if tmx > tMin and tmx < tMax:
            return True, tmx
    return False, 0.0


@pytest.mark.parametrize("radius", [0.0, 1e-9, 1e-3, 0.07, 0.2])
def test_scalar_sphere_hit_pins_the_oracle(oracle, radius):
    """Single-sphere scenes, ray classes (b)-(e), every (tmin, tmax) pair: Sphere.Hit's (hit, t) from the
    scalar statement equals the oracle's primitive test everywhere, and oracle.closest_hit where the
    single leaf's box test (AABB.hit on c -+ (r,r,r), the oracle's own: tests/test_oracle_kat.py) passes."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
    base = soup_case(12, 3)
    rng = np.random.default_rng(int(radius * 1e9) + 5)
    c = np.array([0.25, -0.5, 0.0])
    p = np.zeros(4, dtype=PRIM_DTYPE)  # (mixed_rays wants a rect and a touching pair too: far away, never hit)
    p["kind"] = [2, 1, 0, 2]
    p["p"][0, 0], p["p"][0, 1, 0] = c, radius
    far = np.array([500.0, 500.0, 500.0])
    p["p"][1] = far + np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    p["p"][2, :3] = far + np.array([[9, 0, 0], [10, 0, 0], [9, 1, 0]])
    p["p"][3, 0], p["p"][3, 1, 0] = far + np.array([9.0, 0, 0]), 0.5
    helper = SceneArrays(p, base.albedo, base.light, base.camera, 44, 27)
    rays, cls = mixed_rays(helper, 7 * 600, rng)
    rays = rays[(cls >= 1) & (cls <= 4)]
    near = np.linalg.norm(rays[:, :3] - c, axis=1) < 100  # those aimed at the sphere under test
    rays = rays[near]
    assert len(rays) > 1000
    one = SceneArrays(p[:1], base.albedo, base.light, base.camera, 44, 27)
    o = oracle.OracleScene(one)
    lo, hi = c - radius, c + radius
    pts = np.zeros((4, 3))
    pts[0], pts[1, 0] = c, radius
    for tmin, tmax in T_PAIRS:
        t, prim, nrm = o.closest_hit(rays, tmin=tmin, tmax=tmax)
        hits = box_rejects = 0
        for i, ray in enumerate(rays):
            ro, rd = [float(x) for x in ray[:3]], [float(x) for x in ray[3:]]
            h, ts = sphere_hit([float(x) for x in c], radius, ro, rd, tmin, tmax)
            kh, kt, _, kn = oracle.kat_prim_hit(2, pts, ro, rd, tmin, tmax)
            assert kh == h and (not h or kt == ts), (radius, tmin, tmax, i, h, ts, kh, kt)
            inbox = oracle.kat_aabb(lo, hi, ro, rd, tmin, tmax)
            want = h and inbox
            box_rejects += int(h and not inbox)
            assert (prim[i] == 0) == want, (radius, tmin, tmax, i)
            if want:
                assert t[i] == ts
                hp = ray[:3] + ray[3:] * ts
                assert np.array_equal(nrm[i], kn)
                if radius > 0:
                    assert np.abs(nrm[i] - (hp - c) / np.linalg.norm(hp - c)).max() < 1e-9
                hits += 1
        if radius > 0:
            assert hits > 0
        assert hits < len(rays)
        print(f"r={radius} ({tmin}, {tmax}): {hits} hits of {len(rays)}, {box_rejects} more rejected by the leaf box")
