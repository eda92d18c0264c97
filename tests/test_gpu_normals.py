"""Smooth shading on the GPU (mfx_set_normals): every image, feature buffer and ray count equals the restatement of
the oracle's path trace with the shading normal (tests/normals_helpers.py, pinned to the oracle by
tests/test_normals_reference.py), bit for bit, through every kernel kind; a context whose every primitive keeps its
face normal runs the SN instances and changes no bit; and removing the normals gives the context back."""
import os

import numpy as np
import pytest

from conftest import SEED, scene
from lights_helpers import film_paths, frame_of, light_sets
from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL, PRIM_NORMALS_DTYPE, MfxError
from mafrixraytracing_amd.normals import smooth_normals
from normals_helpers import NormalSet, random_prim_normals, reference_paths, unsmooth
from texture_helpers import TexSet, random_prim_uv, soup_scene, soup_textures

pytestmark = pytest.mark.gpu

W, H = 24, 20  # partial 8x8 tiles in both directions
_cache = {}


def _ctx(a, env=None, **kw):
    from mafrixraytracing_amd.native import NativeContext
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:  # the library reads these at context creation
        return NativeContext(a, seed=SEED, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _shapes(ctx, pool_max=True):
    return {k: v for k, v in ctx.launch_info().items() if pool_max or k != "pool_max"}  # (pool_max: free memory at creation)


def restated(w=W, h=H, spp=4, depth=3, lights=None, textured=False, camera=None):
    """(arrays, normals, lights, textures, maps, radiance (w*h*spp, 3), ray counts, first-hit shading normal
    (w*h*spp, 3), first-hit albedo and hit flag (w*h*spp, 4)) of the mixed soup with random corner normals: computed
    once per shape."""
    key = (w, h, spp, depth, lights, textured, None if camera is None else tuple(camera["position"]))
    if key not in _cache:
        a = soup_scene(w, h, max_depth=depth)
        if camera is not None:
            a.camera = camera
        pn = random_prim_normals(a.prims, seed=31)
        tex = soup_textures() if textured else None
        maps = random_prim_uv(a.prims, len(tex), seed=21) if textured else None
        ls = [a.light] if lights is None else light_sets(a.light)[lights][:3]
        px, py, smp = film_paths(w, h, spp)
        fn, fa = np.zeros((len(px), 3)), np.zeros((len(px), 4))
        rad, counts = reference_paths(a, ls, SEED, px, py, smp, depth, TexSet(a.prims, tex, maps) if textured else None,
                                      NormalSet(a.prims, pn), first_albedo=fa, first_normal=fn)
        _cache[key] = (a, pn, ls, tex, maps, rad, counts, fn, fa)
    return _cache[key]


def _info_on(ctx, nworld, nsmooth=None):
    ni = ctx.normal_info()
    assert ni[1] == 1 and ni[2] == 100 * nworld and ni[3] == 0 and ni[4] >= 1 and ni[5] >= 1 and ni[6] == 0 and ni[7] == 0
    if nsmooth is not None:
        assert ni[0] == nsmooth
    assert ctx.launch_info()["shadow_waves"] == 4


# ---- sampling and ray counts -----------------------------------------------------------------------------------
def test_sampling_equals_the_restatement(gpu, oracle):
    a, pn, _, _, _, rad, counts, _, _ = restated()
    with _ctx(a) as plain, _ctx(a, normals=pn) as ctx:
        frame = ctx.sample(4)
        assert np.array_equal(frame, frame_of(rad, W, H, 4))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert not np.array_equal(frame, plain.sample(4))


def test_deep_paths(gpu, oracle):
    a, pn, _, _, _, rad, counts, _, _ = restated(16, 12, 2, depth=6)
    with _ctx(a, normals=pn) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 12, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_three_lights(gpu, oracle):
    a, pn, ls, _, _, rad, counts, _, _ = restated(spp=2, lights="N5")
    assert len(ls) == 3
    with _ctx(a, lights=ls, normals=pn) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.light_info()[1] == 1 and ctx.normal_info()[1] == 1


def test_textures_and_normals_together(gpu, oracle):
    a, pn, _, tex, maps, rad, counts, fn, fa = restated(spp=2, textured=True)
    with _ctx(a, textures=tex, prim_uv=maps, normals=pn) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.texture_info()[1] == 1 and ctx.normal_info()[1] == 1
        f = ctx.aov(1)  # k_aov's TX, SN instance
        assert np.array_equal(f[:, 0:3], fn.reshape(W * H, 2, 3)[:, 0, :] / 1.0)
        assert np.array_equal(f[:, 4:8], fa.reshape(W * H, 2, 4)[:, 0, :] / 1.0)


# ---- mfx_normal_info ---------------------------------------------------------------------------------------------
def test_normal_info(gpu):
    a, pn, _, _, _, _, _, _, _ = restated()
    with _ctx(a) as ctx:
        assert not ctx.normal_info().any()
        before = _shapes(ctx)
        ctx.set_normals(pn)
        _info_on(ctx, len(a.prims), int((pn["smooth"] != 0).sum()))
        assert _shapes(ctx)["pool_max"] == before["pool_max"]  # no pool bytes: the slots the memory allows stay
        ctx.set_normals(None)
        assert not ctx.normal_info().any()


# ---- mfx_aov -------------------------------------------------------------------------------------------------------
def test_feature_buffer_normals(gpu, oracle):
    a, pn, _, _, _, _, _, fn, _ = restated()
    n = fn.reshape(W * H, 4, 3)
    with _ctx(a) as plain, _ctx(a, normals=pn) as ctx:
        for spp in (1, 2):
            f, g = ctx.aov(spp), plain.aov(spp)
            want = n[:, 0, :] if spp == 1 else n[:, 0, :] + n[:, 1, :]
            assert np.array_equal(f[:, 0:3], want / float(spp))
            assert np.array_equal(f[:, 3:8], g[:, 3:8])  # depth, albedo, hit fraction: unchanged
            assert not np.array_equal(f[:, 0:3], g[:, 0:3])


# ---- identity: every smooth == 0 -----------------------------------------------------------------------------------
def _identity(a, pn, run, **kw):
    """A context with normals none of which is smooth against the context without: `run` gives what to compare."""
    with _ctx(a, **kw) as base, _ctx(a, normals=unsmooth(pn), **kw) as sn:
        assert sn.normal_info()[1] == 1 and sn.normal_info()[0] == 0 and not base.normal_info().any()
        want, got = run(base), run(sn)
        assert len(want) == len(got)
        for x, y in zip(want, got):
            assert np.array_equal(x, y)
        assert np.array_equal(base.ray_counts()[:3], sn.ray_counts()[:3])
        assert base.build_info()["digest"] == sn.build_info()["digest"]


def _sky():
    from mafrixraytracing_amd.environment import gradient
    return gradient(4, (0.2, 0.4, 1.0), (0.9, 0.8, 0.7), (0.1, 0.1, 0.05))


IDENTITY = {
    "one_light": dict(),
    "three_lights": dict(lights="N5"),
    "textures": dict(textured=True),
    "sampled_sky": dict(environment=True, sample_sky=True),
    "unsampled_sky": dict(environment=True),
    "lens": dict(lens=(0.05, 3.0)),
    "device_list": dict(devices=[0, 0]),
}


@pytest.mark.parametrize("case", list(IDENTITY))
def test_identity_with_no_smooth_primitive(gpu, case):
    kw = dict(IDENTITY[case])
    if "environment" in kw:  # an open scene: the sky is seen and lights
        a = scene("spot", W, H)
        pn = smooth_normals(a.prims)
    else:
        a = soup_scene(W, H)
        pn = random_prim_normals(a.prims, seed=31)
    if kw.pop("textured", False):
        tex = soup_textures()
        kw.update(textures=tex, prim_uv=random_prim_uv(a.prims, len(tex), seed=21))
    if "lights" in kw:
        kw["lights"] = light_sets(a.light)[kw["lights"]][:3]
    if kw.pop("environment", False):
        kw["environment"] = _sky()
    _identity(a, pn, lambda c: (c.sample(3),), **kw)


def test_identity_adaptive(gpu):
    """The LIST instances: a listed trace and the resume's per-tile counts."""
    a = soup_scene(W, H)
    pn = random_prim_normals(a.prims, seed=31)

    def run(c):
        f, t = c.sample_adaptive(2, 6, 2, 0.7, 1e-3)
        f2, t2, _ = c.sample_adaptive_resume(8, 2, 0.5, 1e-3)
        return f, t, f2, t2
    _identity(a, pn, run)


def test_identity_render_ahead(gpu):
    a = soup_scene(W, H)
    pn = random_prim_normals(a.prims, seed=31)
    _identity(a, pn, lambda c: tuple(c.render_rgba8(1) for _ in range(6)), render_ahead=4)


def test_removing_the_normals_restores_the_context(gpu, oracle):
    a, pn, _, _, _, rad, _, _, _ = restated()
    with _ctx(a) as ctx, _ctx(a) as never:
        shapes, digest = _shapes(ctx), ctx.build_info()["digest"]
        want = never.sample(4)
        ctx.set_normals(pn)
        assert np.array_equal(ctx.sample(4), frame_of(rad, W, H, 4))
        assert ctx.build_info()["digest"] == digest  # the digest does not cover the normals
        ctx.set_normals(None)
        assert not ctx.normal_info().any()
        assert _shapes(ctx) == shapes and _shapes(ctx, False) == _shapes(never, False)
        assert ctx.build_info()["digest"] == digest
        ctx.accum_clear()
        ctx.trace_accumulate(4, 0)
        assert np.array_equal(ctx.accum_read_mean(4.0), want)
        ctx.set_normals(None)  # none before, none now


# ---- every kernel kind ---------------------------------------------------------------------------------------------
KINDS = {
    "slots_in_lds": ("cornell", {}, lambda li: li["nslot_shd"] > 0 and li["ninst_lds"] == 0),
    "flat": ("spot", {}, lambda li: li["nslot_shd"] == 0 and li["ninst_lds"] == 0),
    "flat_no_spill": ("cornell", {"MFX_SLOT_LDS": "0"}, lambda li: li["nslot_shd"] == 0 and not li["spill_shd"]),
    "two_level": ("spot16_instanced@2l", {}, lambda li: li["ninst_lds"] > 0),
    "spill": ("spot", {"MFX_STACK_LDS": "2"}, lambda li: li["spill_shd"] and li["stack_lds_shd"] == 2),
    "queues_on": ("spot", {"MFX_QUEUE_FROM": "1"}, lambda li: li["queue_from"] == 1),
    "queues_off": ("spot", {"MFX_QUEUE_FROM": "-1"}, lambda li: li["queue_from"] == -1),
    # (the node format has no entry in mfx_launch_info: the predicate shows the scene kind with per-format instances)
    "fp32_nodes": ("spot", {"MFX_NODE_F32": "1"}, lambda li: li["nslot_shd"] == 0 and li["ninst_lds"] == 0),
}


def _world_normals(a, tn):
    """The world primitives' normals of an instanced scene from its templates' (the expansion in entry order)."""
    rows = a.instancing[1]
    return np.concatenate([tn[int(r["first"]):int(r["first"]) + int(r["count"])] for r in rows])


def kind_restated(name):
    """(arrays, the normals the context takes, radiance, counts) of smooth_normals on scene `name` at 16x16x2."""
    if ("kind", name) not in _cache:
        a = scene(name, 16, 16)
        if a.instancing is not None:
            tn = smooth_normals(a.instancing[0])
            wn = _world_normals(a, tn)
            assert len(wn) == len(a.prims)
        else:
            tn = wn = smooth_normals(a.prims)
        px, py, smp = film_paths(16, 16, 2)
        rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 3, None, NormalSet(a.prims, wn))
        plain, _ = reference_paths(a, [a.light], SEED, px, py, smp, 3, None, None)
        assert name == "cornell" or not np.array_equal(rad, plain)  # (a box's edges are creases: its normals stay)
        _cache[("kind", name)] = (a, tn, rad, counts)
    return _cache[("kind", name)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_kernel_kind(gpu, oracle, kind):
    name, env, ran = KINDS[kind]
    a, tn, rad, counts = kind_restated(name)
    with _ctx(a, env, normals=tn) as ctx:
        li = ctx.launch_info()
        assert ran(li), li
        _info_on(ctx, len(a.prims))
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 16, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


# ---- instancing ----------------------------------------------------------------------------------------------------
def test_instanced_flattened_and_expanded_give_one_image(gpu, oracle):
    from mafrixraytracing_amd.abi import MFX_F_FLATTEN
    a, tn, rad, _ = kind_restated("spot16_instanced@2l")
    wn = _world_normals(a, tn)
    free = scene("spot16_instanced", 16, 16)  # (no MFX_F_TWO_LEVEL: it excludes MFX_F_FLATTEN)
    with _ctx(a, normals=tn) as two, _ctx(free, flags=MFX_F_FLATTEN, normals=tn) as flat, \
            _ctx(a, instancing=False, normals=wn) as world:
        assert two.launch_info()["ninst_lds"] > 0 and flat.launch_info()["ninst_lds"] == 0
        f = two.sample(2)
        assert np.array_equal(f, flat.sample(2)) and np.array_equal(f, world.sample(2))
        assert np.array_equal(f, frame_of(rad, 16, 16, 2))
        assert np.array_equal(two.ray_counts()[:3], world.ray_counts()[:3])
        assert np.array_equal(two.aov(1), world.aov(1)) and np.array_equal(flat.aov(1), world.aov(1))
        assert two.normal_info()[2] == 100 * len(a.prims)  # every instance has its own records
        assert np.array_equal(two.normal_info()[:4], world.normal_info()[:4])


# ---- rebuild -------------------------------------------------------------------------------------------------------
def test_set_camera_rebuild_keeps_the_normals(gpu, oracle):
    a0 = soup_scene(W, H)
    cam = dict(a0.camera, position=tuple(p + d for p, d in zip(a0.camera["position"], (0.5, 0.5, 5.0))))
    b, pn, _, _, _, rad, counts, _, _ = restated(spp=2, camera=cam)
    with _ctx(a0, normals=pn) as m, _ctx(b, normals=pn) as f:
        m.sample(1)
        m.set_camera(cam)
        assert m.camera_info()["rebuilds"] == 1
        assert m.build_info()["digest"] == f.build_info()["digest"]
        assert np.array_equal(m.normal_info(), f.normal_info()) and _shapes(m, False) == _shapes(f, False)
        m.accum_clear()
        m.trace_accumulate(2, 0)
        got = m.accum_read_mean(2.0)
        assert np.array_equal(got, f.sample(2))
        assert np.array_equal(got, frame_of(rad, W, H, 2))
        assert np.array_equal(m.ray_counts()[:3], counts)
        assert np.array_equal(m.aov(1), f.aov(1))


# ---- refusals and invalidations ------------------------------------------------------------------------------------
def test_refusals(gpu):
    a = soup_scene(W, H)
    pn = random_prim_normals(a.prims, seed=31)
    for flag in (MFX_F_MEGAKERNEL, MFX_F_COUNT_STATS):
        with _ctx(a, flags=flag) as ctx:
            with pytest.raises(MfxError, match=r"\(-4\).*MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS"):
                ctx.set_normals(pn)
            ctx.set_normals(None)  # nothing to remove: fine
            assert not ctx.normal_info().any()
    sphere = int(np.flatnonzero(a.prims["kind"] == 2)[0])
    flat = int(np.flatnonzero((a.prims["kind"] != 2) & (pn["smooth"] != 0))[0])
    with _ctx(a) as ctx:
        want = ctx.sample(2)
        shapes = _shapes(ctx)
        with pytest.raises(MfxError, match=rf"\(-1\).*nprims {len(pn) - 1} differs"):
            ctx.set_normals(pn[:-1])
        bad = pn.copy()
        bad[sphere]["smooth"] = 1
        with pytest.raises(MfxError, match=rf"\(-1\).*primitive {sphere} is a smooth sphere"):
            ctx.set_normals(bad)
        bad = pn.copy()
        bad[flat]["n"][1][2] = np.inf
        bad[-1]["n"][0][0] = np.nan  # the first offender is named
        with pytest.raises(MfxError, match=rf"\(-1\).*primitive {flat} normal of corner 1 is not finite"):
            ctx.set_normals(bad)
        ok = unsmooth(pn)
        ok["n"] = np.nan  # an unsmooth primitive's normals are not looked at
        ctx.set_normals(ok)
        ctx.set_normals(None)
        # a refused call changes nothing
        assert not ctx.normal_info().any() and _shapes(ctx) == shapes
        ctx.accum_clear()
        ctx.trace_accumulate(2, 0)
        assert np.array_equal(ctx.accum_read_mean(2.0), want)


def test_invalidations(gpu):
    from mafrixraytracing_amd.denoise import DenoiseConfig
    a = soup_scene(W, H)
    pn = random_prim_normals(a.prims, seed=31)
    with _ctx(a) as ctx:
        frame = ctx.sample(2)
        ctx.aov(1)
        ctx.denoise(frame, cfg=DenoiseConfig())
        ctx.sample_adaptive(2, 4, 2, 0.7, 1e-3)
        ctx.set_normals(pn)
        with pytest.raises(MfxError, match=r"\(-4\)"):  # the feature buffers are the old normals'
            ctx.denoise(frame, cfg=DenoiseConfig())
        with pytest.raises(MfxError, match=r"\(-4\)"):  # and so is the adaptive result
            ctx.sample_adaptive_resume(6, 2, 0.7, 1e-3)
        ctx.aov(1)
        ctx.denoise(frame, cfg=DenoiseConfig())
        ctx.sample_adaptive(2, 4, 2, 0.7, 1e-3)
        ctx.set_normals(None)
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.denoise(frame, cfg=DenoiseConfig())
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.sample_adaptive_resume(6, 2, 0.7, 1e-3)
