"""The sky on the GPU (mfx_set_environment): every image and ray count equals the restatement of the oracle's
path trace with the miss term (tests/env_helpers.py, pinned to the oracle by
tests/test_environment_reference.py), bit for bit, through every kernel kind, depth and sampling call; a black
sky and a removed one change nothing; what a change of sky invalidates; what is refused; and the furnace."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED, scene
from env_helpers import (FURNACE_SPP, distinct_map, furnace_check, furnace_scene, reference_paths)
from gpu_helpers import ctx_env
from lights_helpers import film_paths, frame_of, light_sets
from mafrixraytracing_amd import environment
from mafrixraytracing_amd.abi import (MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL, MFX_F_ROW_PARTITION, MfxEnvironment, MfxError)
from temporal_helpers import with_camera
from test_gpu_camera_cuts_cull import NOTHING, OFF, ON
from test_gpu_lights import KINDS

pytestmark = pytest.mark.gpu

W, H = 24, 20  # partial 8x8 tiles in both directions
MAPS = {"m5": distinct_map(5, 5), "m7": distinct_map(7, 9), "m64": distinct_map(64, 3), "zero": np.zeros((5, 5, 3), np.float32),
        "c1": environment.constant((0.7, 0.4, 1.3)), None: None}
_cache = {}


def restated(name, w, h, spp, depth=3, env="m5", lights=None, camera=None, base=0):
    """(arrays, lights, per-path radiance, ray counts, info) of scene `name` under MAPS[env]: computed once."""
    key = (name, w, h, spp, depth, env, lights, None if camera is None else tuple(camera["position"]), base)
    if key not in _cache:
        a = scene(name, w, h, max_depth=depth)
        if camera is not None:
            a = with_camera(a, dict(a.camera, **camera))
        ls = [a.light] if lights is None else light_sets(a.light)[lights][:3]
        px, py, smp = film_paths(w, h, spp, base)
        info = {}
        rad, counts = reference_paths(a, ls, SEED, px, py, smp, depth, env=MAPS[env], info=info)
        rad.setflags(write=False)
        _cache[key] = (a, ls, rad, counts, info)
    return _cache[key]


def _info_on(ctx, size):
    ei = ctx.environment_info()
    assert ei[0] == size and ei[1] == 1 and ei[2] == 12 * size * size and ei[3] == 4, ei
    assert ei[4] >= 1 and ei[5] >= 1 and ei[6] == 0 and ei[7] == 0, ei


def _shapes(ctx):
    return {k: v for k, v in ctx.launch_info().items() if k != "pool_max"}  # (pool_max: free memory)


@pytest.mark.parametrize("name,w,h,spp", [("spot", W, H, 2), ("cornell", 16, 12, 3)])
def test_sample_equals_the_restatement(gpu, oracle, name, w, h, spp):
    a, _, rad, counts, info = restated(name, w, h, spp)
    assert all(m >= 1 for m in info["misses"])
    with ctx_env(a, environment=MAPS["m5"]) as ctx, ctx_env(a) as plain:
        frame = ctx.sample(spp)
        assert np.array_equal(frame, frame_of(rad, w, h, spp))
        black = plain.sample(spp)
        assert not np.array_equal(frame, black)
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert np.array_equal(ctx.ray_counts()[:3], plain.ray_counts()[:3])
        _info_on(ctx, 5)
        assert not plain.environment_info().any()
        assert _shapes(ctx) == _shapes(plain) and ctx.build_info()["digest"] == plain.build_info()["digest"]


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_kernel_kind(gpu, oracle, kind):
    name, env, ran = KINDS[kind]
    a, _, rad, counts, _ = restated(name, 16, 16, 2)
    with ctx_env(a, env, environment=MAPS["m5"]) as ctx:
        li = ctx.launch_info()
        assert ran(li), li
        _info_on(ctx, 5)
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 16, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


@pytest.mark.parametrize("cuts", ["on", "off"])
def test_camera_cuts_on_and_off(gpu, oracle, cuts):
    a, _, rad, counts, _ = restated("spot", W, H, 2)
    with ctx_env(a, ON if cuts == "on" else OFF, environment=MAPS["m5"]) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.launch_info()["camera_cuts"] is (cuts == "on")
        if cuts == "on":
            assert ctx.camera_cut_info()["builds"] >= 1


# (64 x 64: the 40-degree view crosses many texels; a one-texel map: the empty tiles' lanes derive no direction)
@pytest.mark.parametrize("env", ["m64", "c1"])
def test_a_camera_that_sees_nothing(gpu, oracle, env):
    """Every tile's cut is empty, no window makes a ray: each pixel is the mean of its samples' texels."""
    a, _, rad, counts, info = restated("spot", W, H, 3, env=env, camera=NOTHING)
    assert info["misses"][0] == W * H * 3 and tuple(counts) == (W * H * 3, 0, 0)
    with ctx_env(a, ON, environment=MAPS[env]) as ctx:
        frame = ctx.sample(3)
        ci = ctx.camera_cut_info()
        assert ci["builds"] >= 1 and ci["empty_tiles"] == ci["tiles"]
        assert np.array_equal(frame, frame_of(rad, W, H, 3))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        if env == "m64":
            assert len(np.unique(frame[:, 0])) > 3  # the background shows the map


@pytest.mark.parametrize("name,w,h,spp,depth", [("spot", W, H, 2, 0), ("cornell", 16, 12, 2, 6), ("cornell", 16, 12, 1, 15)])
def test_depths(gpu, oracle, name, w, h, spp, depth):
    """depth 0: only camera misses contribute; 6 and 15: fold_path's loop past WF_RES_VERTS."""
    a, _, rad, counts, info = restated(name, w, h, spp, depth)
    if depth == 6:
        assert all(m >= 1 for m in info["misses"]), info["misses"]
    with ctx_env(a, environment=MAPS["m5"]) as ctx:
        assert np.array_equal(ctx.sample(spp), frame_of(rad, w, h, spp))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_a_black_sky_and_a_removed_one_change_nothing(gpu, oracle):
    a = scene("spot", W, H)
    ref, st = oracle.OracleScene(a).sample(3, SEED, with_stats=True)
    with ctx_env(a) as base:
        want = base.sample(3)
        assert np.array_equal(want, ref)
        shapes = _shapes(base)
        with ctx_env(a, environment=MAPS["zero"]) as z:
            assert z.environment_info()[1] == 1  # the ENV instances run
            assert np.array_equal(z.sample(3), want)
            assert tuple(z.ray_counts()[:3]) == tuple(st[:3])
        with ctx_env(a, environment=MAPS["m5"]) as c:
            assert not np.array_equal(c.sample(3), want)
            c.set_environment(None)
            assert not c.environment_info().any()
            assert _shapes(c) == shapes
            c.accum_clear()
            c.trace_accumulate(3, 0)
            assert np.array_equal(c.accum_read_mean(3.0), want)
            c.set_environment(None)  # none before, none now
            c.set_environment(MAPS["m5"])
            _info_on(c, 5)


def test_a_4096_map(gpu, oracle):
    """Texel ids up to 2^24 - 1 fit the record: a constant 4096 x 4096 map is the one-texel map's image."""
    a, _, rad, counts, _ = restated("spot", W, H, 2, env="c1")
    big = np.empty((4096, 4096, 3), dtype=np.float32)
    big[:] = MAPS["c1"].reshape(3)
    dirs = environment.texel_direction(64).reshape(-1, 3)
    from mafrixraytracing_amd.abi import env_texel_index
    assert int(env_texel_index(dirs, 4096).max()) > (1 << 24) - 4096 * 64  # (the last rows are reached)
    with ctx_env(a, environment=big) as ctx:
        ei = ctx.environment_info()
        assert ei[0] == 4096 and ei[2] == 12.0 * 4096 * 4096
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_three_lights(gpu, oracle):
    a, ls, rad, counts, _ = restated("cornell", 16, 12, 3, lights="N5")
    assert len(ls) == 3
    with ctx_env(a, lights=ls, environment=MAPS["m5"]) as ctx:
        assert np.array_equal(ctx.sample(3), frame_of(rad, 16, 12, 3))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.light_info()[1] == 1
        _info_on(ctx, 5)


def test_textures(gpu, oracle):
    from texture_helpers import TexSet, random_prim_uv, soup_scene, soup_textures
    w, h, spp = 16, 12, 2
    a = soup_scene(w, h)
    tex = soup_textures()
    maps = random_prim_uv(a.prims, len(tex), seed=21)
    px, py, smp = film_paths(w, h, spp)
    info = {}
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 3, TexSet(a.prims, tex, maps), env=MAPS["m5"], info=info)
    with ctx_env(a, textures=tex, prim_uv=maps, environment=MAPS["m5"]) as ctx:
        assert ctx.texture_info()[1] == 1
        _info_on(ctx, 5)
        assert np.array_equal(ctx.sample(spp), frame_of(rad, w, h, spp))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_instanced_flattened(gpu, oracle):
    a, _, rad, counts, _ = restated("spot16_instanced", 16, 16, 2)
    with ctx_env(a, environment=MAPS["m5"]) as ctx:
        assert ctx.launch_info()["ninst_lds"] == 0
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 16, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_device_list_and_row_partition(gpu, oracle):
    a, _, rad, counts, _ = restated("spot", W, H, 2)
    want = frame_of(rad, W, H, 2)
    with ctx_env(a, devices=[0, 0], environment=MAPS["m5"]) as ctx:
        assert np.array_equal(ctx.sample(2), want)
        _info_on(ctx, 5)
        ctx.set_environment(MAPS["zero"])  # every device of the list gets the new map
        with ctx_env(a) as plain:  # (the second call's paths are samples 2 and 3 on both)
            plain.sample(2)
            assert np.array_equal(ctx.sample(2), plain.sample(2))
    total, ct = np.zeros((W * H, 3)), np.zeros(3)
    for p in range(2):
        with ctx_env(a, flags=MFX_F_ROW_PARTITION, part_index=p, part_count=2, environment=MAPS["m5"]) as ctx:
            ctx.trace_accumulate(2, 0)
            total += ctx.accum_read_mean(2.0)[:, :3]
            ct += ctx.ray_counts()[:3]
    assert np.array_equal(total, want[:, :3]) and np.array_equal(ct, counts)


def test_render_ahead_frames(gpu, oracle):
    a, _, rad, _, _ = restated("cornell", 16, 12, 6)
    w, h = 16, 12
    r = rad.reshape(w * h, 6, 3)
    with ctx_env(a, render_ahead=4, environment=MAPS["m5"]) as ah, ctx_env(a, environment=MAPS["m5"]) as plain:
        film = np.zeros((w * h, 3))
        for k in range(6):
            got, want = ah.render_rgba8(1), plain.render_rgba8(1)
            assert np.array_equal(got, want)
            film = film + (0.0 + r[:, k, :]) / 1.0  # Film.AddSample of a one-sample frame
            mean = np.ones((w * h, 4))
            mean[:, :3] = film / float(k + 1)
            assert np.array_equal(got, oracle.post_rgba8(mean, w, h))  # the one-sample call's RGBA8
        assert np.array_equal(ah.film_mean(), plain.film_mean())


def test_held_frames_are_not_served_after_a_change(gpu, oracle):
    a = scene("cornell", 16, 12)
    with ctx_env(a, render_ahead=4, environment=MAPS["m5"]) as ah, ctx_env(a, environment=MAPS["m5"]) as plain, \
            ctx_env(a, render_ahead=4, environment=MAPS["m5"]) as stay:
        for _ in range(2):
            assert np.array_equal(ah.render_rgba8(1), plain.render_rgba8(1))
            stay.render_rgba8(1)
        ah.set_environment(MAPS["m7"])  # two frames of the batch are still held
        plain.set_environment(MAPS["m7"])
        for _ in range(3):
            got = ah.render_rgba8(1)
            assert np.array_equal(got, plain.render_rgba8(1))
            assert not np.array_equal(got, stay.render_rgba8(1))
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


def test_adaptive_resume_and_state(gpu, oracle):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, luminance, reference_tile_spp
    w, h = 24, 12
    a, _, rad, _, _ = restated("cornell", w, h, 8)
    Y = luminance(rad.reshape(w * h, 8, 3).transpose(1, 0, 2))
    cfg = None
    for rel in (1.0, 0.7, 1.5, 0.5, 0.35, 2.0, 0.25):  # a threshold that stops some tiles and not others
        c = AdaptiveConfig(2, 6, 2, rel, 1e-3)
        spp, gap = reference_tile_spp(Y[:6], w, h, c)
        if spp.min() < 6 and (spp == 6).any() and gap > 1e-6:
            cfg, want_spp = c, spp
            break
    assert cfg is not None
    with ctx_env(a, environment=MAPS["m5"]) as ctx:
        frame, tiles = ctx.sample_adaptive(2, 6, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(tiles, want_spp)
        assert np.array_equal(frame, _prefix_mean(rad, w, h, 8, tiles))
        ctx.aov(1)
        out = ctx.denoise_var()  # the adaptive source: the moments of the paths that ended in the sky are in it
        assert np.all(np.isfinite(out))
        frame8, tiles8, _ = ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(frame8, _prefix_mean(rad, w, h, 8, tiles8))
        # a change of sky: the adaptive result is gone, the feature buffers stay
        ctx.set_environment(MAPS["m7"])
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.denoise_var()
        filtered = ctx.denoise(frame8)  # after aov, then set_environment: still runs
        assert np.all(np.isfinite(filtered))
        ctx.set_environment(None)
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)
        assert np.all(np.isfinite(ctx.denoise(frame8)))


def test_set_camera_rebuild_keeps_the_sky(gpu, oracle):
    a = scene("cornell", 16, 12)
    cam = dict(a.camera, position=tuple(p + d for p, d in zip(a.camera["position"], (0.5, 0.5, 5.0))))
    b, _, rad, counts, _ = restated("cornell", 16, 12, 3, camera=cam)
    with ctx_env(a, environment=MAPS["m5"]) as m:
        m.sample(1)
        m.set_camera(cam)
        assert m.camera_info()["rebuilds"] == 1
        _info_on(m, 5)
        m.accum_clear()
        m.trace_accumulate(3, 0)
        assert np.array_equal(m.accum_read_mean(3.0), frame_of(rad, 16, 12, 3))
        assert np.array_equal(m.ray_counts()[:3], counts)


def test_the_map_changes_between_two_sample_calls(gpu, oracle):
    """next_sample is left alone: the second call's paths are samples 2 and 3, under the second map."""
    a, _, rad0, _, _ = restated("spot", W, H, 2)
    _, _, rad1, counts1, _ = restated("spot", W, H, 2, env="m7", base=2)
    with ctx_env(a, environment=MAPS["m5"]) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad0, W, H, 2))
        before = ctx.ray_counts()[:3].copy()
        ctx.set_environment(MAPS["m7"])
        assert np.array_equal(ctx.ray_counts()[:3], before)  # the ray counters are left alone
        _info_on(ctx, 7)
        assert np.array_equal(ctx.sample(2), frame_of(rad1, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts1)


def _refused(ctx, code, env_struct, what):
    rc = ctx.lib.mfx_set_environment(ctx._h, C.byref(env_struct) if env_struct is not None else None)
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
            with pytest.raises(MfxError, match=r"\(-4\)"):
                ctx.set_environment(good)
            assert not ctx.environment_info().any()
    with ctx_env(a) as ctx:
        want = ctx.sample(1)
        _refused(ctx, -1, MfxEnvironment(ptr, 0, 0), "size 0")
        _refused(ctx, -1, MfxEnvironment(ptr, 4097, 0), "size 4097")
        _refused(ctx, -1, MfxEnvironment(None, 5, 0), "rgb is NULL")
        for bad, why in ((np.nan, "not finite"), (np.inf, "not finite"), (-1e-30, "negative")):
            m = good.copy()
            m[3, 2, 1] = bad  # texel 17: x 2, y 3, channel 1
            _refused(ctx, -1, MfxEnvironment(m.ctypes.data_as(C.POINTER(C.c_float)), 5, 0), "texel 17 (x 2, y 3) channel 1 is " + why)
        assert not ctx.environment_info().any()  # a refused call changes nothing
        ctx.accum_clear()
        ctx.trace_accumulate(1, 0)
        assert np.array_equal(ctx.accum_read_mean(1.0), want)


def test_furnace(gpu):
    a = furnace_scene()
    with ctx_env(a, environment=environment.constant((1.0, 1.0, 1.0))) as ctx:
        frame = ctx.sample(FURNACE_SPP)
        K = a.width * a.height * FURNACE_SPP
        assert tuple(ctx.ray_counts()[:3]) == (K, K, K)
    mean, bound = furnace_check(frame)
    print("furnace mean", mean, "bound", bound)
    assert np.all(np.abs(mean - np.array((0.2, 0.5, 0.8))) <= bound)
