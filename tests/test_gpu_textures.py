"""Albedo textures on the GPU (mfx_create_textured): every image, feature buffer and ray count equals the
restatement of the oracle's path trace with the texel lookup (tests/texture_helpers.py, pinned to the oracle
by tests/test_textures_reference.py), bit for bit, through every sampling call; and a context without a
textured primitive is the untextured one."""
import numpy as np
import pytest

from conftest import SEED, scene
from mafrixraytracing_amd.abi import PRIM_UV_DTYPE
from lights_helpers import film_paths, frame_of, light_sets
from texture_helpers import TexSet, random_prim_uv, reference_paths, soup_scene, soup_textures

pytestmark = pytest.mark.gpu

W, H = 24, 20  # partial 8x8 tiles in both directions
_cache = {}


def _ctx(a, **kw):
    from mafrixraytracing_amd.native import NativeContext
    return NativeContext(a, seed=SEED, **kw)


def restated(w, h, spp, depth=3, nmat=5, lights=None, camera=None):
    """(arrays, textures, maps, radiance (w*h*spp, 3), ray counts, first-hit albedo (w*h*spp, 4)) of the mixed
    soup with the three procedural textures: computed once per shape."""
    key = (w, h, spp, depth, nmat, lights, None if camera is None else tuple(camera["position"]))
    if key not in _cache:
        a = soup_scene(w, h, max_depth=depth, nmat=nmat)
        if camera is not None:
            a.camera = camera
        tex = soup_textures()
        maps = random_prim_uv(a.prims, len(tex), seed=21)
        ls = [a.light] if lights is None else light_sets(a.light)[lights][:3]
        px, py, smp = film_paths(w, h, spp)
        first = np.zeros((len(px), 4))
        rad, counts = reference_paths(a, ls, SEED, px, py, smp, depth, TexSet(a.prims, tex, maps), first_albedo=first)
        _cache[key] = (a, tex, maps, ls, rad, counts, first)
    return _cache[key]


def test_feature_buffer_albedo(gpu, oracle):
    a, tex, maps, _, _, _, first = restated(W, H, 4)
    want = first.reshape(W * H, 4, 4)[:, 0, :]  # sample 0 of every pixel
    with _ctx(a, textures=tex, prim_uv=maps) as ctx:
        f = ctx.aov(1)
        assert np.array_equal(f[:, 4:8].view(np.uint64), (want / 1.0).view(np.uint64))
        plain = _ctx(a)
        with plain:
            g = plain.aov(1)
        assert np.array_equal(f[:, :4], g[:, :4]) and np.array_equal(f[:, 7], g[:, 7])  # geometry: unchanged
        assert not np.array_equal(f[:, 4:7], g[:, 4:7])
        # two samples: summed in sample order, divided once
        want2 = (first.reshape(W * H, 4, 4)[:, 0, :] + first.reshape(W * H, 4, 4)[:, 1, :]) / 2.0
        assert np.array_equal(ctx.aov(2)[:, 4:8], want2)


def test_sampling_equals_the_restatement(gpu, oracle):
    a, tex, maps, _, rad, counts, _ = restated(W, H, 4)
    with _ctx(a, textures=tex, prim_uv=maps) as ctx:
        frame = ctx.sample(4)
        assert np.array_equal(frame, frame_of(rad, W, H, 4))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        ti = ctx.texture_info()
        nw = len(a.prims)
        assert ti[0] == 3 and ti[1] == 1 and ti[2] == 4 * (1 + 15 + 64 * 64) and ti[3] == 68 * nw
        assert ti[4] == 4 * (a.max_depth + 1) and ti[5] >= 1 and ti[6] >= 1 and ti[7] == 0
        assert ctx.launch_info()["shadow_waves"] == 4


def test_deep_paths(gpu, oracle):
    """max_depth 6: vertices 4 to 6 go through fold_path's loop, past WF_RES_VERTS."""
    a, tex, maps, _, rad, counts, _ = restated(16, 12, 2, depth=6)
    with _ctx(a, textures=tex, prim_uv=maps) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, 16, 12, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.texture_info()[4] == 28


def test_materials_past_lds(gpu, oracle):
    """300 materials: the walls' albedos are read from global memory (past WF_RES_MAT_LDS), then textured."""
    a, tex, maps, _, rad, counts, _ = restated(W, H, 2, nmat=300)
    assert len(a.albedo) == 300 and (a.prims["material"] >= 256).sum() > 10
    with _ctx(a, textures=tex, prim_uv=maps) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)


def test_no_change_without_textures(gpu, oracle):
    a = soup_scene(W, H)
    tex = soup_textures()
    none = np.zeros(len(a.prims), dtype=PRIM_UV_DTYPE)
    none["texture"] = -1
    white = [np.full((5, 3, 4), 255, np.uint8)]
    maps = random_prim_uv(a.prims, 1, seed=21)
    with _ctx(a, lights=[a.light]) as base:
        want = base.sample(3)
        shapes = {k: v for k, v in base.launch_info().items() if k != "pool_max"}  # (pool_max: free memory)
        digest = base.build_info()["digest"]
        with _ctx(a, textures=[], prim_uv=None) as c0, _ctx(a, textures=tex, prim_uv=none) as c1:
            for c in (c0, c1):  # no texture at all, and textures that no primitive uses
                assert np.array_equal(c.sample(3), want)
                assert {k: v for k, v in c.launch_info().items() if k != "pool_max"} == shapes
                assert c.build_info()["digest"] == digest
                assert tuple(c.texture_info()[:5]) == (0, 0, 0, 0, 0)
                assert np.array_equal(c.texture_info(), base.texture_info())
                assert np.array_equal(c.ray_counts(), base.ray_counts())
        with _ctx(a, textures=white, prim_uv=maps) as cw:  # an all-white texture: the textured kernels, the same bits
            assert cw.texture_info()[1] == 1
            assert np.array_equal(cw.sample(3), want)
            assert cw.build_info()["digest"] == digest  # the digest does not cover the textures
    ref, _ = oracle.OracleScene(a).sample(3, SEED, with_stats=True)
    assert np.array_equal(want, ref)


def test_three_lights(gpu, oracle):
    a, tex, maps, ls, rad, counts, _ = restated(W, H, 2, lights="N5")
    assert len(ls) == 3
    with _ctx(a, lights=ls, textures=tex, prim_uv=maps) as ctx:
        assert np.array_equal(ctx.sample(2), frame_of(rad, W, H, 2))
        assert np.array_equal(ctx.ray_counts()[:3], counts)
        assert ctx.light_info()[1] == 1 and ctx.texture_info()[1] == 1


def test_instanced_flattened_and_expanded_give_one_image(gpu, oracle):
    from mafrixraytracing_amd.abi import MFX_F_FLATTEN
    from mafrixraytracing_amd.textures import planar_prim_uv
    a = scene("spot16_instanced@2l", 16, 16)
    tmpl, rows = a.instancing
    tex = soup_textures()
    tuv = planar_prim_uv(tmpl, 2, axes=(0, 1), scale=3.0)
    tuv["texture"][::3] = -1  # textured and untextured primitives side by side
    tuv["texture"][1::3] = 1
    wuv = np.concatenate([tuv[int(r["first"]):int(r["first"]) + int(r["count"])] for r in rows])
    assert len(wuv) == len(a.prims)
    free = scene("spot16_instanced", 16, 16)  # (no MFX_F_TWO_LEVEL: it excludes MFX_F_FLATTEN)
    with _ctx(a, textures=tex, prim_uv=tuv) as two, _ctx(free, flags=MFX_F_FLATTEN, textures=tex, prim_uv=tuv) as flat, \
            _ctx(a, instancing=False, textures=tex, prim_uv=wuv) as world, _ctx(a) as plain:
        assert two.launch_info()["ninst_lds"] > 0 and flat.launch_info()["ninst_lds"] == 0
        f = two.sample(2)
        assert np.array_equal(f, flat.sample(2)) and np.array_equal(f, world.sample(2))
        assert np.array_equal(two.ray_counts()[:3], world.ray_counts()[:3])
        assert not np.array_equal(f, plain.sample(2))
        assert np.array_equal(two.aov(1), world.aov(1)) and np.array_equal(flat.aov(1), world.aov(1))
        assert two.texture_info()[3] == 68 * len(a.prims)  # every instance has its own records


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


def test_adaptive(gpu, oracle):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, luminance, reference_tile_spp
    a, tex, maps, _, rad, _, _ = restated(W, H, 6)
    Y = luminance(rad.reshape(W * H, 6, 3).transpose(1, 0, 2))
    cfg = None
    for rel in (1.0, 0.7, 1.5, 0.5, 2.0, 0.3):  # a threshold that stops some tiles and not others, found on the restatement
        c = AdaptiveConfig(2, 6, 2, rel, 1e-3)
        spp, gap = reference_tile_spp(Y, W, H, c)
        if spp.min() < 6 and (spp == 6).any() and gap > 1e-6:
            cfg, want_spp = c, spp
            break
    assert cfg is not None
    with _ctx(a, textures=tex, prim_uv=maps) as ctx:
        frame, tiles = ctx.sample_adaptive(2, 6, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(tiles, want_spp)
        assert np.array_equal(frame, _prefix_mean(rad, W, H, 6, tiles))


def test_render_ahead_frames(gpu, oracle):
    a, tex, maps, _, rad, _, _ = restated(W, H, 6)
    r = rad.reshape(W * H, 6, 3)
    with _ctx(a, textures=tex, prim_uv=maps, render_ahead=4) as ah, _ctx(a, textures=tex, prim_uv=maps) as plain:
        film = np.zeros((W * H, 3))
        for k in range(6):  # one whole batch and half of the next
            got, want = ah.render_rgba8(1), plain.render_rgba8(1)
            assert np.array_equal(got, want)
            film = film + (0.0 + r[:, k, :]) / 1.0  # Film.AddSample of a one-sample frame
            mean = np.ones((W * H, 4))
            mean[:, :3] = film / float(k + 1)
            assert np.array_equal(got, oracle.post_rgba8(mean, W, H))


def test_device_list(gpu, oracle):
    a, tex, maps, _, rad, _, _ = restated(W, H, 4)
    with _ctx(a, textures=tex, prim_uv=maps, devices=[0, 0]) as two:
        assert np.array_equal(two.sample(4), frame_of(rad, W, H, 4))
        assert two.texture_info()[1] == 1


def test_set_camera_rebuild(gpu, oracle):
    a0 = soup_scene(W, H)
    cam = dict(a0.camera, position=tuple(p + d for p, d in zip(a0.camera["position"], (0.5, 0.5, 5.0))))
    b, tex, maps, _, rad, counts, _ = restated(W, H, 2, camera=cam)
    with _ctx(a0, textures=tex, prim_uv=maps) as m, _ctx(b, textures=tex, prim_uv=maps) as f:
        m.sample(1)
        m.set_camera(cam)
        assert m.camera_info()["rebuilds"] == 1
        assert m.build_info()["digest"] == f.build_info()["digest"]
        assert np.array_equal(m.texture_info(), f.texture_info())
        m.accum_clear()
        m.trace_accumulate(2, 0)
        got = m.accum_read_mean(2.0)
        assert np.array_equal(got, f.sample(2))
        assert np.array_equal(got, frame_of(rad, W, H, 2))
        assert np.array_equal(m.aov(1), f.aov(1))


def test_flags_refused(gpu):
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL, MfxError
    a = soup_scene(W, H)
    tex = soup_textures()
    maps = random_prim_uv(a.prims, len(tex), seed=21)
    for flag in (MFX_F_MEGAKERNEL, MFX_F_COUNT_STATS):
        with pytest.raises(MfxError, match=r"\(-1\).*MFX_F_MEGAKERNEL and MFX_F_COUNT_STATS"):
            _ctx(a, flags=flag, textures=tex, prim_uv=maps)
        none = maps.copy()
        none["texture"] = -1
        with _ctx(a, flags=flag, textures=tex, prim_uv=none) as ok:  # no textured primitive: the flags stand
            assert ok.texture_info()[1] == 0
