"""GPU parity on soups that mix triangles, rects and spheres with up to 65,536 materials, at default
and non-default (tmin, tmax): every comparison is array_equal against the CPU oracle (the megakernel
above 1 spp keeps test_gpu_parity.py's 1e-12 bar). tests/soup_helpers.py holds the generators and the
cases; tests/test_mixed_soup_reference.py asserts on the oracle alone that these cases reach what they
are for (every ray class hits and misses, second triangles, ties, hits beyond tMax, lit images, all 16
bits of the material index).

What depends on it in the kernels: leaf_hit's branch on the slot kind in its four load variants (global,
scalar loads in the camera packets, the small-scene LDS copy; a rect's two slots and the second one's
info), sphere_hit64's asymmetric comparisons and its tMax against tri_hit64 that ignores it,
ref_leaf_hit on leaves that mix kinds, the sphere normal in k_shadow, the megakernel and mfx_aov, the
sphere's bound in the GPU build, and the material index as a 16-bit WfMat read back by k_resolve's
three instances from LDS (< 256) or global memory.

Value-only mutants of the library this file was run against, and the first test each fails (none
fails test_gpu_edge_parity.py or test_gpu_build.py, whose soups are triangles with one material):
  1 sphere_hit64 `tmn > tMin`                        test_closest_hit_exact[0.0-99999999.0-12-3]
  2 sphere_hit64 without `tmx < tMax`                test_closest_hit_exact[1e-06-0.3-12-3]
  3 `typedef uint8_t WfMat`                          test_wavefront_image_exact[default-3-777-40000-0-False]
  4 `R.mat[v] = (int16_t)P.vmat[...]`                test_wavefront_image_exact[default-3-777-40000-0-False]
  5 fold_vertex `mat <= WF_RES_MAT_LDS`              test_wavefront_image_exact[default-3-777-40000-0-False]
  6 leaf_hit: a rect's trig2 keeps trig1's `info`    test_closest_hit_exact[1e-06-99999999.0-12-3]
  7 beats() `pos <= bpos`                            none: it changes nothing. (first, pos) names one
    primitive, so pos == bpos at equal `first` is the same candidate again (a leaf evaluated whole twice),
    replaced by itself. The tie rules themselves are held: `pos > bpos` and `first < B.first` both fail
    test_closest_hit_exact[1e-06-99999999.0-777-40000] (and the triangle soups too).
The parent of this file's commit (node tests culled at tMax, DESIGN.md §3 `tslack`) fails
test_any_hit_exact[5000-65536], test_leaf_entered_before_tmax_with_every_primitive_hit_beyond_it and
test_shadow_rays_occluded_beyond_the_light[*]."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SEED
from soup_helpers import (ADAPTIVE, BUILD_NS, DEPTHS, FAR, H, HIGH_MAT, IMAGE_SOUPS, MATERIAL_SOUPS, QUERY_SOUPS, SPP,
                          T_PAIRS, W, adaptive_answer, any_hit_sets, beyond_light_scene, beyond_tmax_case, far_case,
                          floor_shadow_rays, image_answer, moved_two_spheres_plane,
                          oracle_scene, query_answer, query_case, soup_case, with_depth)
from test_gpu_build import both

pytestmark = pytest.mark.gpu


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _ctx(a, env=None, **kw):
    """A context created under `env` (the library reads these at creation)."""
    from mafrixraytracing_amd.native import NativeContext
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return NativeContext(a, seed=SEED, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- queries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
@pytest.mark.parametrize("tpair", T_PAIRS, ids=_ids)
def test_closest_hit_exact(gpu, oracle, n, nmat, tpair):
    a, rays, cls = query_case(n, nmat)
    ot, op, on = query_answer(oracle, n, nmat, tpair)
    with _ctx(a) as ctx:
        print(f"n={n}: {ctx.build_info()['slots']} slots")  # which scene kind (slots in LDS or not) the size took
        gt, gp, gn = ctx.closest_hit(rays, tmin=tpair[0], tmax=tpair[1])
    bad = np.flatnonzero(gp != op)
    assert len(bad) == 0, f"prim mismatch on {len(bad)} rays, classes {np.bincount(cls[bad], minlength=7).tolist()}"
    assert np.array_equal(gt, ot), f"t mismatch, classes {np.bincount(cls[gt != ot], minlength=7).tolist()}"
    assert np.array_equal(gn, on), f"normal mismatch, classes {np.bincount(cls[np.any(gn != on, axis=1)], minlength=7).tolist()}"


@pytest.mark.parametrize("n,nmat", QUERY_SOUPS)
def test_any_hit_exact(gpu, oracle, n, nmat):
    """Occlusion with random tmax, and with tmax at, one ulp around and 1e-12 around the closest hit's t:
    a sphere's strict t < tMax beside triangles that ignore tMax."""
    a, rays, cls = query_case(n, nmat)
    with _ctx(a) as ctx:
        for name, rr, tm, want in any_hit_sets(oracle, n, nmat):
            got = ctx.any_hit(rr, tm)
            assert np.array_equal(got, want), f"{name}: occlusion mismatch on {(got != want).sum()} rays"


def test_leaf_entered_before_tmax_with_every_primitive_hit_beyond_it(gpu, oracle):
    """Two triangles of one reference leaf whose own boxes the ray enters only after tMax while the leaf's
    box is entered before it: Bvh.Hit reports the nearer hit (soup_helpers.beyond_tmax_case)."""
    a, rays, tmax = beyond_tmax_case()
    o = oracle.OracleScene(a)
    with _ctx(a) as ctx:
        assert np.array_equal(ctx.any_hit(rays, tmax), o.any_hit(rays, tmax))
        for tm in sorted(set(tmax.tolist())):
            sel = tmax == tm
            for got, want in zip(ctx.closest_hit(rays[sel], tmax=tm), o.closest_hit(rays[sel], tmax=tm)):
                assert np.array_equal(got, want), tm


@pytest.mark.parametrize("mode", ["wavefront", "megakernel"])
def test_shadow_rays_occluded_beyond_the_light(gpu, oracle, mode):
    """The same rule through k_shadow and the megakernel's shadow rays (soup_helpers.beyond_light_scene):
    floor points whose shadow ray the reference calls occluded by two triangles behind the light."""
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    a = beyond_light_scene()
    o = oracle.OracleScene(a)
    rays, tmax = floor_shadow_rays(a)
    spp = 1 if mode == "megakernel" else SPP
    ref, st = o.sample(spp, SEED, with_stats=True)
    with _ctx(a, flags=MFX_F_MEGAKERNEL if mode == "megakernel" else 0) as ctx:
        assert np.array_equal(ctx.any_hit(rays, tmax), o.any_hit(rays, tmax))
        _image_exact(ctx, ref, st, spp=spp)


# ---- the BVH build ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BUILD_NS)
def test_gpu_bvh_equals_host_bvh_on_mixed_soup(gpu, n):
    bg, bh = both(soup_case(n, 3))
    assert bg["gpu_bvh"] and not bh["gpu_bvh"]
    for k in ("nodes2", "nodes4", "slots"):
        assert bg[k] == bh[k], (k, bg[k], bh[k])
    assert bg["digest"] == bh["digest"], (bg, bh)


def test_ref_leaf_grouping_identical(gpu, oracle):
    a = soup_case(777, 40000)
    with _ctx(a) as ctx:
        gi, gf, gc = ctx.ref_leaves()
    oi, of, oc = oracle_scene(oracle, a).bvh_leaves()
    assert np.array_equal(gi, oi) and np.array_equal(gf, of) and np.array_equal(gc, oc)


# ---- images and counters ----------------------------------------------------------------------------
def _image_exact(ctx, ref, st, spp=SPP):
    img = ctx.sample(spp)
    counts = ctx.ray_counts()
    assert tuple(counts[:3]) == tuple(st[:3]), (counts[:3], st[:3])
    assert np.array_equal(img, ref), np.abs(img - ref).max()  # bit for bit


VARIANTS = {"default": {}, "no camera packets": {"MFX_CAMERA_PACKETS": "0"}, "f32 nodes": {"MFX_NODE_F32": "1"},
            "pool 256": {"MFX_POOL": "256"}}


@pytest.mark.parametrize("key", IMAGE_SOUPS, ids=_ids)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_wavefront_image_exact(gpu, oracle, key, depth, variant):
    ref, st = image_answer(oracle, key, depth)
    with _ctx(with_depth(soup_case(*key), depth), VARIANTS[variant]) as ctx:
        _image_exact(ctx, ref, st)
        if variant == "pool 256":
            assert ctx.trace_timing()["generations"] > 1


@pytest.mark.parametrize("key", IMAGE_SOUPS, ids=_ids)
@pytest.mark.parametrize("depth", DEPTHS)
def test_megakernel_image(gpu, oracle, key, depth):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    a = with_depth(soup_case(*key), depth)
    ref1, st1 = image_answer(oracle, key, depth, spp=1)
    with _ctx(a, flags=MFX_F_MEGAKERNEL) as ctx:
        _image_exact(ctx, ref1, st1, spp=1)  # one path per pixel: bit for bit
    ref, st = image_answer(oracle, key, depth)
    with _ctx(a, flags=MFX_F_MEGAKERNEL) as ctx:
        img = ctx.sample(SPP)
        counts = ctx.ray_counts()
    assert tuple(counts[:3]) == tuple(st[:3]), (counts[:3], st[:3])
    diff = np.abs(img[:, :3] - ref[:, :3])  # FP64 atomics add a pixel's paths in arrival order
    assert diff.max() <= 1e-12 * max(1.0, np.abs(ref).max()), diff.max()
    assert np.all(img[:, 3] == 1.0)


# ---- materials --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MATERIAL_SOUPS, ids=_ids)
@pytest.mark.parametrize("depth", DEPTHS)
def test_material_index_width_image_exact(gpu, oracle, key, depth):
    """nmat 3 and 257 around the 256 albedo rows k_resolve keeps in LDS, 40000 and 65536 beyond 15 bits,
    and every material >= 32768; depth 5 folds vertices 4 and 5 in fold_path's loop over vmat."""
    ref, st = image_answer(oracle, key, depth)
    with _ctx(with_depth(soup_case(*key), depth)) as ctx:
        _image_exact(ctx, ref, st)


def test_render_ahead_frames_with_high_materials(gpu, oracle):
    """k_resolve's frames instance: four one-sample render calls served from batches of 3 equal the
    one-sample-per-call context's and the oracle's film and post (Film.AddSample + PostProcess)."""
    from mafrixraytracing_amd.abi import dptr
    a = soup_case(*HIGH_MAT)
    o = oracle_scene(oracle, a)
    npix = W * H
    accum, target, fc = np.zeros((npix, 4)), np.zeros((npix, 4)), np.zeros(1)
    with _ctx(a) as c1, _ctx(a, render_ahead=3) as c2:
        for k in range(4):
            r1, r2 = c1.render_rgba8(1), c2.render_rgba8(1)
            fr = o.sample(1, SEED, sample_base=k)
            oracle.lib().oracle_film_add(dptr(accum), dptr(target), dptr(fc), dptr(fr), npix)
            ref = oracle.post_rgba8(target, W, H)
            assert np.array_equal(r1, ref), (k, (r1 != ref).sum())
            assert np.array_equal(r2, ref), (k, (r2 != ref).sum())
        m1, m2 = c1.film_mean(), c2.film_mean()
    assert np.array_equal(m1, m2)
    assert np.array_equal(m2[:, :3], target[:, :3])


def test_adaptive_with_high_materials(gpu, oracle):
    """k_resolve's moments instance: tile counts, image, RGBA8 and ray counts of the host rule over the
    oracle's one-sample frames."""
    spp, mean, rgba, st, gap = adaptive_answer(oracle, HIGH_MAT)
    assert len(set(spp.ravel().tolist())) > 1 and gap > 1e-6
    with _ctx(soup_case(*HIGH_MAT)) as ctx:
        frame, tiles, out8 = ctx.sample_adaptive(*ADAPTIVE, want_rgba=True)
        c = ctx.ray_counts()
    assert np.array_equal(tiles, spp), (tiles.tolist(), spp.tolist())
    assert np.array_equal(frame, mean), np.abs(frame - mean).max()
    assert np.array_equal(out8, rgba)
    assert (c[0], c[1], c[2]) == (st[0], st[1], st[2]), (c[:3], st)


def test_material_count_limit(gpu):
    """65,536 materials is the documented limit (a path vertex keeps its material in 16 bits): one more
    is refused with MFX_E_INVALID."""
    from mafrixraytracing_amd.abi import MfxOptions, SceneArrays
    a = soup_case(12, 3)
    rng = np.random.default_rng(1)
    for nmat, want in ((65536, 0), (65537, -1)):
        b = SceneArrays(a.prims, rng.uniform(0.05, 0.95, size=(nmat, 3)), a.light, a.camera, W, H)
        d = b.desc()
        opt = MfxOptions(seed=SEED, device=0, flags=0, part_index=0, part_count=1, ndevices=0, render_ahead=0, devices=None)
        h = C.c_void_p()
        rc = gpu.mfx_create(C.byref(d), C.byref(opt), C.byref(h))
        assert rc == want, (nmat, rc, gpu.mfx_last_error())
        if rc == 0:
            gpu.mfx_destroy(h)
        else:
            assert not h.value and b"materials" in gpu.mfx_last_error()


# ---- feature buffers --------------------------------------------------------------------------------
def test_aov_and_denoise_with_spheres_and_high_materials(gpu, oracle):
    from denoise_helpers import scene_features
    from mafrixraytracing_amd.denoise import DenoiseConfig, reference_denoise
    a = soup_case(*HIGH_MAT)
    ref = scene_features(oracle, a, 3, 5)
    frac = ref[:, 7]
    assert ((frac > 0) & (frac < 1)).any() and (frac == 0).any() and (frac == 1).any()
    with _ctx(a) as ctx:
        got = ctx.aov(3, sample_base=5)
        assert np.array_equal(got, ref), np.abs(got - ref).max(axis=0)
        feat = ctx.aov(SPP)
        frame = ctx.sample(SPP)
        out = ctx.denoise(frame)
    assert np.array_equal(feat, scene_features(oracle, a, SPP, 0))
    assert np.array_equal(frame, image_answer(oracle, HIGH_MAT, 3)[0])
    assert np.array_equal(out, reference_denoise(frame, feat, W, H, DenoiseConfig()))
    assert not np.array_equal(out, frame)


# ---- away from unit scale, with spheres -------------------------------------------------------------
@pytest.mark.parametrize("s,offset", FAR)
def test_mixed_soup_far_from_unit_scale_exact(gpu, oracle, s, offset):
    a, b, rr, tmax = far_case(s, offset)
    o = oracle.OracleScene(b)
    ot, op, on = o.closest_hit(rr)
    occ_o = o.any_hit(rr, tmax)
    with _ctx(b) as ctx:
        gt, gp, gn = ctx.closest_hit(rr)
        occ_g = ctx.any_hit(rr, tmax)
    assert np.array_equal(gp, op), f"prim mismatch on {(gp != op).sum()} rays"
    assert np.array_equal(gt, ot)
    assert np.array_equal(gn, on)
    assert np.array_equal(occ_g, occ_o), f"occlusion mismatch on {(occ_g != occ_o).sum()} rays"
    assert (op >= 0).mean() > 0.01
    assert (a.prims["kind"][op[op >= 0]] == 2).any()


def test_sphere_scene_moved_far_from_origin_image_exact(gpu, oracle):
    """two_spheres_plane moved (1e4, -3e3, 2e4) away, geometry, light and camera together (a sphere's
    centre moves, its radius in p[1] does not): the 4-spp image and the ray counts are the oracle's."""
    b = moved_two_spheres_plane()
    ref, st = oracle.OracleScene(b).sample(4, SEED, with_stats=True)
    with _ctx(b) as ctx:
        _image_exact(ctx, ref, st)
    assert (ref[:, :3].sum(1) != 0).mean() > 0.05 and st[1] > 0 and st[2] > 0
