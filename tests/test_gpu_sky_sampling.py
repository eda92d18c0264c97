"""The sky as a light on the GPU (mfx_set_environment_sampled): every image and ray count equals the restatement
of the rule (tests/sky_sampling_helpers.py, pinned on the CPU by tests/test_sky_sampling_reference.py), bit for
bit, through every kernel kind, depth, light count, map size and sampling call; switching between none,
unsampled and sampled; what is refused; the info call; and the furnace."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED, scene
from env_helpers import FURNACE_SPP, distinct_map, furnace_scene
from env_helpers import reference_paths as unsampled_paths
from gpu_helpers import ctx_env
from lights_helpers import film_paths, frame_of, light_sets
from mafrixraytracing_amd import environment
from mafrixraytracing_amd.abi import (MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL, MFX_F_ROW_PARTITION, MfxEnvironment, MfxError)
from mafrixraytracing_amd.lights import strips
from sky_sampling_helpers import reference_paths
from temporal_helpers import with_camera
from test_gpu_camera_cuts_cull import OFF, ON
from test_gpu_lights import KINDS

pytestmark = pytest.mark.gpu

W, H = 24, 20  # partial 8x8 tiles in both directions
MAPS = {"m5": distinct_map(5, 5), "m7": distinct_map(7, 9), "m64": distinct_map(64, 3), "zero": np.zeros((5, 5, 3), np.float32),
        "c1": environment.constant((0.7, 0.4, 1.3)),
        "sun": environment.sun_map(16, 16 * 6 + 9, (2000.0, 1500.0, 900.0), (0.3, 0.3, 0.4))}
_cache = {}


def _lights(a, which):
    if which is None:
        return [a.light]
    if which == "N63":
        return strips(a.light, 63)
    return light_sets(a.light)[which][:3]


def restated(name, w, h, spp, depth=3, env="m5", lights=None, camera=None, base=0, sampled=True):
    """(arrays, lights, per-path radiance, ray counts, info) of scene `name` under the sampled sky MAPS[env] (or,
    sampled=False, the unsampled one): computed once."""
    key = (name, w, h, spp, depth, env, lights, None if camera is None else tuple(camera["position"]), base, sampled)
    if key not in _cache:
        a = scene(name, w, h, max_depth=depth)
        if camera is not None:
            a = with_camera(a, dict(a.camera, **camera))
        ls = _lights(a, lights)
        px, py, smp = film_paths(w, h, spp, base)
        info = {}
        fn = reference_paths if sampled else unsampled_paths
        rad, counts = fn(a, ls, SEED, px, py, smp, depth, env=MAPS[env], info=info)
        rad.setflags(write=False)
        _cache[key] = (a, ls, rad, counts, info)
    return _cache[key]


def _info_on(ctx, size, nlights=1, depth=3):
    si = ctx.sky_sampling_info()
    per_vertex = 4 + (1 if nlights == 1 else 0)
    assert si[0] == 1 and si[1] == nlights + 1 and si[2] == 16 * size * size and si[3] == per_vertex * (depth + 1), si
    assert si[4] >= 1 and si[5] >= 1 and si[6] == 0 and si[7] == 0, si
    ei = ctx.environment_info()  # the sky itself is reported as ever
    assert ei[0] == size and ei[1] == 1 and ei[2] == 12 * size * size and ei[3] == 4 and ei[6] == 0 and ei[7] == 0, ei
    li = ctx.light_info()
    assert li[0] == nlights and li[1] == 1  # the several-light instances run, with one area light too


def _shapes(ctx):
    return {k: v for k, v in ctx.launch_info().items() if k != "pool_max"}  # (pool_max: free memory)


@pytest.mark.parametrize("name,w,h,spp", [("spot", W, H, 2), ("cornell", 16, 12, 3)])
def test_sample_equals_the_restatement(gpu, oracle, name, w, h, spp):
    a, _, rad, counts, info = restated(name, w, h, spp)
    assert info["sky_lit"] >= 1 and info["sky_occluded"] >= 1 and info["sky_back"] >= 1, info
    with ctx_env(a, environment=MAPS["m5"], sample_sky=True) as ctx, ctx_env(a, environment=MAPS["zero"], sample_sky=True) as black:
        frame = ctx.sample(spp)
        assert np.array_equal(frame, frame_of(rad, w, h, spp))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert not np.array_equal(frame, black.sample(spp))
        assert np.array_equal(ctx.ray_counts()[:3], black.ray_counts()[:3])  # the black-sky context's counts
        _info_on(ctx, 5)
        assert ctx.launch_info()["gray_light"] is False


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_kernel_kind(gpu, oracle, kind):
    name, env, ran = KINDS[kind]
    a, _, rad, counts, _ = restated(name, 16, 16, 2)
    with ctx_env(a, env, environment=MAPS["m5"], sample_sky=True) as ctx:
        li = ctx.launch_info()
        assert ran(li), li
        _info_on(ctx, 5)
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 16, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


@pytest.mark.parametrize("cuts", ["on", "off"])
def test_camera_cuts_on_and_off(gpu, oracle, cuts):
    a, _, rad, counts, _ = restated("spot", W, H, 2)
    with ctx_env(a, ON if cuts == "on" else OFF, environment=MAPS["m5"], sample_sky=True) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.launch_info()["camera_cuts"] is (cuts == "on")


@pytest.mark.parametrize("name,w,h,spp,depth", [("spot", W, H, 2, 0), ("cornell", 16, 12, 2, 6), ("cornell", 16, 12, 1, 15)])
def test_depths(gpu, oracle, name, w, h, spp, depth):
    """depth 0: the one vertex is lit by the pick; 6 and 15: fold_path's loop past WF_RES_VERTS reads the sky plane."""
    a, _, rad, counts, info = restated(name, w, h, spp, depth)
    assert info["sky_lit"] >= 1
    with ctx_env(a, environment=MAPS["m5"], sample_sky=True) as ctx:
        assert np.array_equal(ctx.sample(spp), frame_of(rad, w, h, spp))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        _info_on(ctx, 5, depth=depth)


@pytest.mark.parametrize("which,n,spp", [(None, 1, 3), ("N5", 3, 3), ("N63", 63, 1)])
def test_light_counts(gpu, oracle, which, n, spp):
    a, ls, rad, counts, info = restated("cornell", 16, 12, spp, lights=which)
    assert len(ls) == n and info["sky_picked"] >= 1
    with ctx_env(a, lights=ls, environment=MAPS["m5"], sample_sky=True) as ctx:
        assert np.array_equal(ctx.sample(spp), frame_of(rad, 16, 12, spp))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        _info_on(ctx, 5, nlights=n)


def test_64_lights_are_refused(gpu):
    a = scene("cornell", 16, 12)
    with ctx_env(a, lights=strips(a.light, 64)) as ctx:
        want = ctx.sample(1)
        with pytest.raises(MfxError, match=r"\(-4\).*64 lights"):
            ctx.set_environment(MAPS["m5"], sampled=True)
        assert not ctx.sky_sampling_info().any() and not ctx.environment_info().any()
        ctx.accum_clear()
        ctx.trace_accumulate(1, 0)
        assert np.array_equal(ctx.accum_read_mean(1.0), want)  # a refused call changes nothing
        ctx.set_environment(MAPS["m5"])  # unsampled: 64 lights will do


@pytest.mark.parametrize("env", ["c1", "m64", "sun"])
def test_map_sizes(gpu, oracle, env):
    a, _, rad, counts, info = restated("spot", W, H, 2, env=env)
    assert info["sky_lit"] >= 1
    with ctx_env(a, environment=MAPS[env], sample_sky=True) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        _info_on(ctx, MAPS[env].shape[0])


def test_a_4096_map(gpu, oracle):
    """Texel ids up to 2^24 - 1 fit the plane and the table: a constant 4096 x 4096 map, sampled."""
    big = np.empty((4096, 4096, 3), dtype=np.float32)
    big[:] = MAPS["c1"].reshape(3)
    a = scene("spot", W, H)
    px, py, smp = film_paths(W, H, 1)
    info = {}
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 3, env=big, info=info)
    assert info["sky_lit"] >= 1
    with ctx_env(a, environment=big, sample_sky=True) as ctx:
        assert ctx.sky_sampling_info()[2] == 16.0 * 4096 * 4096
        assert np.array_equal(ctx.sample(1), frame_of(rad, W, H, 1))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_textures(gpu, oracle):
    from texture_helpers import TexSet, random_prim_uv, soup_scene, soup_textures
    w, h, spp = 16, 12, 2
    a = soup_scene(w, h)
    tex = soup_textures()
    maps = random_prim_uv(a.prims, len(tex), seed=21)
    px, py, smp = film_paths(w, h, spp)
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 3, TexSet(a.prims, tex, maps), env=MAPS["m5"])
    with ctx_env(a, textures=tex, prim_uv=maps, environment=MAPS["m5"], sample_sky=True) as ctx:
        assert ctx.texture_info()[1] == 1
        _info_on(ctx, 5)
        assert np.array_equal(ctx.sample(spp), frame_of(rad, w, h, spp))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


@pytest.mark.parametrize("name", ["spot16_instanced", "spot16_instanced@2l"])
def test_instanced(gpu, oracle, name):
    a, _, rad, counts, _ = restated(name, 16, 16, 2)
    with ctx_env(a, environment=MAPS["m5"], sample_sky=True) as ctx:
        assert (ctx.launch_info()["ninst_lds"] > 0) == name.endswith("@2l")
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 16, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_device_list_and_row_partition(gpu, oracle):
    a, _, rad, counts, _ = restated("spot", W, H, 2)
    want = frame_of(rad, W, H, 2)
    with ctx_env(a, devices=[0, 0], environment=MAPS["m5"], sample_sky=True) as ctx:
        assert np.array_equal(ctx.sample(2), want)
        _info_on(ctx, 5)
    total, ct = np.zeros((W * H, 3)), np.zeros(3)
    for p in range(2):
        with ctx_env(a, flags=MFX_F_ROW_PARTITION, part_index=p, part_count=2, environment=MAPS["m5"], sample_sky=True) as ctx:
            ctx.trace_accumulate(2, 0)
            total += ctx.accum_read_mean(2.0)[:, :3]
            ct += ctx.ray_counts()[:3]
    assert np.array_equal(total, want[:, :3]) and np.array_equal(ct, counts)


def test_render_ahead_frames(gpu, oracle):
    a, _, rad, _, _ = restated("cornell", 16, 12, 6)
    w, h = 16, 12
    r = rad.reshape(w * h, 6, 3)
    with ctx_env(a, render_ahead=4, environment=MAPS["m5"], sample_sky=True) as ah, \
            ctx_env(a, environment=MAPS["m5"], sample_sky=True) as plain:
        film = np.zeros((w * h, 3))
        for k in range(6):
            got, want = ah.render_rgba8(1), plain.render_rgba8(1)
            assert np.array_equal(got, want)
            film = film + (0.0 + r[:, k, :]) / 1.0  # Film.AddSample of a one-sample frame
            mean = np.ones((w * h, 4))
            mean[:, :3] = film / float(k + 1)
            assert np.array_equal(got, oracle.post_rgba8(mean, w, h))  # the one-sample call's RGBA8
        assert np.array_equal(ah.film_mean(), plain.film_mean())


def _prefix_mean(rad, w, h, spp, tile_spp):
    """Every pixel's first n_T samples summed in order from +0.0 and divided by n_T (its tile's count)."""
    r = rad.reshape(w * h, spp, 3)
    out = np.ones((w * h, 4))
    for q in range(w * h):
        n = int(tile_spp[(q % h) // 8, (q // h) // 8])
        s = np.zeros(3)
        for k in range(n):
            s = s + r[q, k]
        out[q, :3] = s / float(n)
    return out


def test_adaptive_and_resume(gpu, oracle):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, luminance, reference_tile_spp
    w, h = 24, 12
    a, _, rad, _, _ = restated("cornell", w, h, 8)
    Y = luminance(rad.reshape(w * h, 8, 3).transpose(1, 0, 2))
    cfg = None
    for rel in (1.0, 0.7, 1.5, 0.5, 0.35, 2.0, 0.25, 3.0, 0.15):  # a threshold that stops some tiles and not others
        c = AdaptiveConfig(2, 6, 2, rel, 1e-3)
        spp, gap = reference_tile_spp(Y[:6], w, h, c)
        if spp.min() < 6 and (spp == 6).any() and gap > 1e-6:
            cfg, want_spp = c, spp
            break
    assert cfg is not None
    with ctx_env(a, environment=MAPS["m5"], sample_sky=True) as ctx:
        frame, tiles = ctx.sample_adaptive(2, 6, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(tiles, want_spp)
        assert np.array_equal(frame, _prefix_mean(rad, w, h, 8, tiles))
        frame8, tiles8, _ = ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(frame8, _prefix_mean(rad, w, h, 8, tiles8))
        ctx.set_environment(MAPS["m5"])  # unsampled now: the adaptive result is gone
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)


def test_sampled_unsampled_sampled_and_removed(gpu, oracle):
    """Each state equals its restatement (next_sample is left alone: samples 0-1, 2-3, 4-5), and a removed sky
    leaves the context that never had one."""
    a, _, rad0, c0, _ = restated("spot", W, H, 2)
    _, _, rad1, c1, _ = restated("spot", W, H, 2, base=2, sampled=False)
    _, _, rad2, c2, _ = restated("spot", W, H, 2, env="m7", base=4)
    with ctx_env(a) as base:
        want = base.sample(3)
        shapes, digest = _shapes(base), base.build_info()["digest"]
        none_info = base.light_info().copy()
    with ctx_env(a, environment=MAPS["m5"], sample_sky=True) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad0, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], c0)
        ctx.set_environment(MAPS["m5"])
        assert not ctx.sky_sampling_info().any() and ctx.environment_info()[1] == 1
        assert np.array_equal(ctx.light_info(), none_info) and _shapes(ctx) == shapes
        assert np.array_equal(ctx.sample(2), frame_of(rad1, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], c1)
        ctx.set_environment(MAPS["m7"], sampled=True)
        _info_on(ctx, 7)
        assert np.array_equal(ctx.sample(2), frame_of(rad2, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], c2)
        ctx.set_environment(None, sampled=True)
        assert not ctx.sky_sampling_info().any() and not ctx.environment_info().any()
        assert np.array_equal(ctx.light_info(), none_info)
        assert _shapes(ctx) == shapes and ctx.build_info()["digest"] == digest
        ctx.accum_clear()
        ctx.trace_accumulate(3, 0)
        assert np.array_equal(ctx.accum_read_mean(3.0), want)  # the image of a context that never had a sky


def test_set_camera_rebuild_keeps_the_sampling(gpu, oracle):
    a = scene("cornell", 16, 12)
    cam = dict(a.camera, position=tuple(p + d for p, d in zip(a.camera["position"], (0.5, 0.5, 5.0))))
    _, _, rad, counts, _ = restated("cornell", 16, 12, 3, camera=cam)
    with ctx_env(a, environment=MAPS["m5"], sample_sky=True) as m:
        m.sample(1)
        m.set_camera(cam)
        assert m.camera_info()["rebuilds"] == 1
        _info_on(m, 5)
        m.accum_clear()
        m.trace_accumulate(3, 0)
        assert np.array_equal(m.accum_read_mean(3.0), frame_of(rad, 16, 12, 3))
        assert np.array_equal(m.ray_counts()[:3], counts)
        m.set_environment(None)  # and the lights' pdf is the one-light context's again after the rebuild
        m.accum_clear()
        m.trace_accumulate(1, 0)
        with ctx_env(with_camera(a, cam)) as plain:
            assert np.array_equal(m.accum_read_mean(1.0), plain.sample(1))


def _refused(ctx, code, env_struct, what):
    rc = ctx.lib.mfx_set_environment_sampled(ctx._h, C.byref(env_struct) if env_struct is not None else None)
    msg = ctx.lib.mfx_last_error().decode()
    assert rc == code, (rc, msg)
    assert what in msg, msg


def test_refusals(gpu):
    a = scene("cornell", 16, 12)
    good = np.ascontiguousarray(MAPS["m5"])
    ptr = good.ctypes.data_as(C.POINTER(C.c_float))
    for flags in (MFX_F_MEGAKERNEL, MFX_F_COUNT_STATS):
        with ctx_env(a, flags=flags) as ctx:
            _refused(ctx, -4, MfxEnvironment(ptr, 5, 0), "MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS")
            assert not ctx.sky_sampling_info().any() and not ctx.environment_info().any()
    with ctx_env(a) as ctx:
        want = ctx.sample(1)
        _refused(ctx, -1, MfxEnvironment(ptr, 0, 0), "size 0")
        _refused(ctx, -1, MfxEnvironment(ptr, 4097, 0), "size 4097")
        _refused(ctx, -1, MfxEnvironment(None, 5, 0), "rgb is NULL")
        for bad, why in ((np.nan, "not finite"), (np.inf, "not finite"), (-1e-30, "negative")):
            m = good.copy()
            m[3, 2, 1] = bad  # texel 17: x 2, y 3, channel 1
            _refused(ctx, -1, MfxEnvironment(m.ctypes.data_as(C.POINTER(C.c_float)), 5, 0), "texel 17 (x 2, y 3) channel 1 is " + why)
        assert not ctx.sky_sampling_info().any() and not ctx.environment_info().any()  # a refused call changes nothing
        ctx.accum_clear()
        ctx.trace_accumulate(1, 0)
        assert np.array_equal(ctx.accum_read_mean(1.0), want)
    with ctx_env(a, environment=good, sample_sky=True) as ctx:  # a refused call leaves a sampled sky sampled
        _refused(ctx, -1, MfxEnvironment(ptr, 0, 0), "size 0")
        _info_on(ctx, 5)


def test_furnace(gpu):
    """One floor under a constant sky of 1, depth 0: the one vertex is lit by the pick alone, and the film mean is
    the albedo within five standard errors taken from the frame's own pixels."""
    a = furnace_scene()
    a = type(a)(a.prims, a.albedo, a.light, a.camera, a.width, a.height, 0)
    with ctx_env(a, environment=environment.constant((1.0, 1.0, 1.0)), sample_sky=True) as ctx:
        frame = ctx.sample(FURNACE_SPP)
        K = a.width * a.height * FURNACE_SPP
        assert tuple(ctx.ray_counts()[:3]) == (K, 0, K)
    f = np.asarray(frame, dtype=np.float64)[:, :3]
    mean, se = f.mean(axis=0), f.std(axis=0, ddof=1) / np.sqrt(len(f))
    print("furnace mean", mean, "standard error", se)
    assert np.all(se > 0.0) and np.all(np.abs(mean - np.array((0.2, 0.5, 0.8))) <= 5.0 * se)
