"""The thin lens on the GPU (mfx_set_lens): every image, feature buffer and ray count equals the restatement of
the oracle's path trace with the lens ray (tests/lens_helpers.py, pinned by tests/test_lens_reference.py), bit for
bit, through every scene kind, depth, sampling call and light or surface extension; camera moves under a lens;
the widening; removal; what setting a lens invalidates; and what is refused."""
import numpy as np
import pytest

from conftest import SEED, scene
from env_helpers import distinct_map
from gpu_helpers import ctx_env
from lens_helpers import reference_paths, scene_features
from lights_helpers import film_paths, frame_of, light_sets
from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL, MFX_F_ROW_PARTITION, MfxError
from temporal_helpers import moved, with_camera

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 19, 13, 2, 3  # the edge tiles are padded on both axes
# (aperture, focus) per scene: the disk is a few pixels wide on the film, the focus plane cuts the scene
LENS = {"cornell": (0.08, 2.6), "spot": (0.06, 4.2), "spot16_instanced": (0.1, 8.5), "spot16_instanced@2l": (0.1, 8.5)}
MAP = distinct_map(5, 5)
_cache = {}


def restated(name="cornell", w=W, h=H, spp=SPP, depth=DEPTH, lens="own", lights=None, env=False, sampled=False, camera=None,
             base=0):
    """(arrays, lights, per-path radiance, ray counts, info) of scene `name` through its lens: computed once."""
    lens = LENS[name] if lens == "own" else lens
    key = (name, w, h, spp, depth, lens, lights, env, sampled, None if camera is None else tuple(camera["position"]), base)
    if key not in _cache:
        a = scene(name, w, h, max_depth=depth)
        if camera is not None:
            a = with_camera(a, camera)
        ls = [a.light] if lights is None else light_sets(a.light)[lights][:3]
        px, py, smp = film_paths(w, h, spp, base)
        info = {}
        rad, counts = reference_paths(a, ls, SEED, px, py, smp, depth, lens=lens, env=MAP if env else None, sampled=sampled,
                                      info=info)
        rad.setflags(write=False)
        _cache[key] = (a, ls, rad, counts, info)
    return _cache[key]


def _shapes(ctx, pool_max=False):
    return {k: v for k, v in ctx.launch_info().items() if pool_max or k != "pool_max"}  # (pool_max: free memory at creation)


def _exact(ctx, rad, counts, w=W, h=H, spp=SPP):
    assert np.array_equal(ctx.sample(spp), frame_of(rad, w, h, spp))
    assert np.array_equal(ctx.ray_counts()[:3], counts)
    assert counts[0] == w * h * spp  # primary rays are w * h * spp as ever


def _info_on(ctx, lens):
    li = ctx.lens_info()
    assert li[0] == 1 and (li[1], li[2]) == tuple(lens) and li[10] > 0 and li[12] >= 1 and li[13] >= 1 and not li[14:].any(), li
    from mafrixraytracing_amd.abi import lens_derive
    assert np.array_equal(li[3:10], lens_derive(_derived(ctx), lens))  # the record of the context's own camera


def _derived(ctx):
    ci = ctx.camera_info()
    return {k: tuple(ci[k]) for k in ("position", "topleft", "right", "down")}


@pytest.mark.parametrize("depth", [0, 1, 3])
def test_depths(gpu, oracle, depth):
    a, _, rad, counts, _ = restated(depth=depth)
    with ctx_env(a, {"MFX_CAMERA_CUT_MIN_SAMPLES": "1"}, lens=LENS["cornell"]) as ctx:  # (a pinhole context would build)
        _info_on(ctx, LENS["cornell"])
        _exact(ctx, rad, counts)
        assert ctx.camera_cut_info()["builds"] == 0  # no cut table is built or read under a lens
    pin = oracle.OracleScene(a).sample(SPP, SEED)
    assert not np.array_equal(frame_of(rad, W, H, SPP), pin)  # the aperture is large enough to show


@pytest.mark.parametrize("name,ran", [("cornell", lambda li: li["ninst_lds"] == 0 and li["nslot_ext"] > 0),
                                      ("spot", lambda li: li["ninst_lds"] == 0 and li["nslot_ext"] == 0),
                                      ("spot16_instanced@2l", lambda li: li["ninst_lds"] > 0),
                                      ("spot16_instanced", lambda li: li["ninst_lds"] == 0)])
def test_scene_kinds(gpu, oracle, name, ran):
    """Flat with its slots in LDS, flat, two-level instanced and flattened instanced."""
    a, _, rad, counts, _ = restated(name)
    with ctx_env(a, lens=LENS[name]) as ctx:
        assert ran(ctx.launch_info()), ctx.launch_info()
        _info_on(ctx, LENS[name])
        _exact(ctx, rad, counts)


def test_forced_spill(gpu, oracle):
    a, _, rad, counts, _ = restated("spot")
    with ctx_env(a, {"MFX_STACK_LDS": "2"}, lens=LENS["spot"]) as ctx:
        li = ctx.launch_info()
        assert li["spill_ext"] and li["stack_lds_ext"] == 2, li
        _exact(ctx, rad, counts)


def test_one_sample_render_calls_and_render_ahead(gpu, oracle):
    """The one-sample render call runs the wavefront pipeline under a lens; K = 4 serves the same frames."""
    a, _, rad, _, _ = restated(spp=6)
    r = rad.reshape(W * H, 6, 3)
    lens = LENS["cornell"]
    with ctx_env(a, render_ahead=4, lens=lens) as ah, ctx_env(a, lens=lens) as plain, ctx_env(a, lens=lens) as smp:
        film = np.zeros((W * H, 3))
        for k in range(6):
            got, want = ah.render_rgba8(1), plain.render_rgba8(1)
            assert np.array_equal(got, want)
            one = smp.sample(1)  # mfx_sample's sample k: the render call's frame is its post
            assert np.array_equal(one[:, :3], r[:, k, :])
            film = film + (0.0 + r[:, k, :]) / 1.0  # Film.AddSample of a one-sample frame
            mean = np.ones((W * H, 4))
            mean[:, :3] = film / float(k + 1)
            assert np.array_equal(got, oracle.post_rgba8(mean, W, H))
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
    """mfx_sample_adaptive (the tile list) and a resume with differing per-tile counts (the list with counts)."""
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, luminance, reference_tile_spp
    a, _, rad, _, _ = restated(spp=8)
    Y = luminance(rad.reshape(W * H, 8, 3).transpose(1, 0, 2))
    cfg = None
    for rel in (1.0, 0.7, 1.5, 0.5, 0.35, 2.0, 0.25, 3.0, 0.18):  # a threshold that stops some tiles and not others
        c = AdaptiveConfig(2, 6, 2, rel, 1e-3)
        spp, gap = reference_tile_spp(Y[:6], W, H, c)
        if spp.min() < 6 and (spp == 6).any() and gap > 1e-6:
            cfg, want_spp = c, spp
            break
    assert cfg is not None
    with ctx_env(a, lens=LENS["cornell"]) as ctx:
        frame, tiles = ctx.sample_adaptive(2, 6, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(tiles, want_spp) and len(set(tiles.ravel().tolist())) > 1
        assert np.array_equal(frame, _prefix_mean(rad, W, H, 8, tiles))
        frame8, tiles8, _ = ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)
        assert np.array_equal(frame8, _prefix_mean(rad, W, H, 8, tiles8))
        assert (tiles8 > tiles).any()
        # a new lens ends the adaptive result, as a new camera does
        ctx.set_lens((0.05, 2.0))
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.sample_adaptive_resume(8, 2, cfg.rel_error, cfg.abs_floor)


def test_device_list_and_row_partition(gpu, oracle):
    a, _, rad, counts, _ = restated()
    want = frame_of(rad, W, H, SPP)
    with ctx_env(a, devices=[0, 0], lens=LENS["cornell"]) as ctx:
        _info_on(ctx, LENS["cornell"])
        assert np.array_equal(ctx.sample(SPP), want)
        assert np.array_equal(ctx.ray_counts()[:3], counts)
    total, ct = np.zeros((W * H, 3)), np.zeros(3)
    for p in range(2):
        with ctx_env(a, flags=MFX_F_ROW_PARTITION, part_index=p, part_count=2, lens=LENS["cornell"]) as ctx:
            ctx.trace_accumulate(SPP, 0)
            total += ctx.accum_read_mean(float(SPP))[:, :3]
            ct += ctx.ray_counts()[:3]
    assert np.array_equal(total, want[:, :3]) and np.array_equal(ct, counts)


def test_three_lights(gpu, oracle):
    a, ls, rad, counts, _ = restated(lights="N5")
    assert len(ls) == 3
    with ctx_env(a, lights=ls, lens=LENS["cornell"]) as ctx:
        assert ctx.light_info()[1] == 1
        _exact(ctx, rad, counts)


def test_textures(gpu, oracle):
    from texture_helpers import TexSet, random_prim_uv, soup_scene, soup_textures
    a = soup_scene(W, H)
    tex = soup_textures()
    maps = random_prim_uv(a.prims, len(tex), seed=21)
    px, py, smp = film_paths(W, H, SPP)
    lens = (0.05, 3.0)
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 3, lens=lens, tex=TexSet(a.prims, tex, maps))
    pin, _ = reference_paths(a, [a.light], SEED, px, py, smp, 3, tex=TexSet(a.prims, tex, maps))
    assert not np.array_equal(rad, pin)
    with ctx_env(a, textures=tex, prim_uv=maps, lens=lens) as ctx:
        assert ctx.texture_info()[1] == 1
        _exact(ctx, rad, counts)
        feat = ctx.aov(2)  # k_aov's textured LENS instance
        assert np.all(np.isfinite(feat)) and feat[:, 7].max() > 0


def test_an_unsampled_sky_on_an_open_scene(gpu, oracle):
    """A lens ray's miss shows the texel of d, the lens ray's direction."""
    a, _, rad, counts, info = restated("spot", env=True)
    assert info["misses"][0] >= 1
    _, _, pin, _, _ = restated("spot", env=True, lens=None)
    assert not np.array_equal(rad, pin)
    with ctx_env(a, environment=MAP, lens=LENS["spot"]) as ctx:
        assert ctx.environment_info()[1] == 1
        _exact(ctx, rad, counts)


def test_a_sampled_sky(gpu, oracle):
    a, _, rad, counts, _ = restated("spot", env=True, sampled=True)
    with ctx_env(a, environment=MAP, sample_sky=True, lens=LENS["spot"]) as ctx:
        assert ctx.sky_sampling_info()[0] == 1
        _exact(ctx, rad, counts)


def test_aov_and_denoise_var(gpu, oracle):
    """mfx_aov(2): the lens ray composed with the oracle's closest hit; mfx_denoise_var on those features against its
    numpy statement."""
    from denoise_helpers import scene_features as pinhole_features
    from denoise_var_helpers import mean_and_moments
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var, variance_of_mean
    a, _, rad, _, _ = restated(spp=4)
    lens = LENS["cornell"]
    want = scene_features(oracle, a, 2, 0, lens, SEED)
    assert not np.array_equal(want, pinhole_features(oracle, a, 2, 0, SEED))
    frames = np.ones((4, W * H, 4))
    frames[:, :, :3] = rad.reshape(W * H, 4, 3).transpose(1, 0, 2)
    mean, S1, S2 = mean_and_moments(frames, 4)
    var = variance_of_mean(S1, S2, np.full(W * H, 4))
    with ctx_env(a, lens=lens) as ctx:
        feat = ctx.aov(2)
        assert np.array_equal(feat, want)
        cfg = DenoiseVarConfig()
        ref, rvar = reference_denoise_var(mean, var, want, W, H, cfg)
        got, gvar = ctx.denoise_var(mean, variance=var, cfg=cfg, want_variance=True)
        assert np.array_equal(got, ref) and np.array_equal(gvar, rvar)
        # a new lens: the feature buffers are another camera's until mfx_aov runs again
        ctx.set_lens((0.03, 2.0))
        with pytest.raises(MfxError, match=r"\(-4\)"):
            ctx.denoise_var(mean, variance=var, cfg=cfg)
        assert np.array_equal(ctx.aov(2), scene_features(oracle, a, 2, 0, (0.03, 2.0), SEED))


@pytest.mark.parametrize("move,rebuilds", [(dict(dpos=(0.2, 0.1, -0.5), ddir=(0.05, -0.05, 0.0)), 0), (dict(dpos=(0.5, 0.5, 5.0)), 1)])
def test_set_camera_under_a_lens(gpu, oracle, move, rebuilds):
    """One move in place and one that forces a rebuild: aperture and focus are kept, the record is derived again."""
    a = scene("cornell", W, H)
    cam = moved(a.camera, **move)
    lens = LENS["cornell"]
    b, _, rad, counts, _ = restated(camera=cam)
    with ctx_env(a, lens=lens) as m, ctx_env(b, lens=lens) as f:
        before = m.lens_info()
        m.set_camera(cam)
        assert m.camera_info()["rebuilds"] == rebuilds
        li = m.lens_info()
        assert (li[1], li[2]) == lens and li[11] == before[11] == 1  # (the first lens of a fresh context widens)
        assert np.array_equal(li[:11], f.lens_info()[:11])
        _info_on(m, lens)
        ci = m.camera_info()
        assert li[10] <= ci["eps_built"] and ci["eps_needed"] <= li[10]
        if rebuilds:
            assert m.build_info()["digest"] == f.build_info()["digest"]
        _exact(m, rad, counts)
        assert np.array_equal(f.sample(SPP), frame_of(rad, W, H, SPP))


def test_the_widening(gpu, oracle):
    """A lens whose aperture alone forces a rebuild; a smaller one afterwards goes in place."""
    a, _, rad, counts, _ = restated()
    _, _, small, scounts, _ = restated(lens=(0.02, 2.6), base=SPP)
    with ctx_env(a) as ctx:
        ci = ctx.camera_info()
        assert ci["eps_needed"] == ci["eps_built"]
        digest = ctx.build_info()["digest"]
        ctx.set_lens(LENS["cornell"])
        li, after = ctx.lens_info(), ctx.camera_info()
        assert li[11] == 1 and after["rebuilds"] == 0  # the lens's rebuild, not the camera's
        assert li[10] == after["eps_built"] > ci["eps_built"]
        assert ctx.build_info()["digest"] != digest
        _exact(ctx, rad, counts)  # still exact
        ctx.set_lens((0.02, 2.6))
        li2 = ctx.lens_info()
        assert li2[11] == 1 and li2[10] < li[10] and ctx.camera_info()["eps_built"] == after["eps_built"]
        assert np.array_equal(ctx.sample(SPP), frame_of(small, W, H, SPP))  # next_sample is left alone: samples 2, 3
        assert np.array_equal(ctx.ray_counts()[:3], scounts)


@pytest.mark.parametrize("how", ["none", "zero"])
def test_removal(gpu, oracle, how):
    """After set_lens(None) and after aperture = 0 the context is one that never had a lens."""
    a = scene("cornell", W, H)
    want = oracle.OracleScene(a).sample(SPP, SEED)
    with ctx_env(a) as never, ctx_env(a) as ctx:
        shapes, digest = _shapes(ctx, pool_max=True), ctx.build_info()["digest"]
        ctx.set_lens(LENS["cornell"])
        assert ctx.lens_info()[11] == 1 and ctx.build_info()["digest"] != digest
        assert not np.array_equal(ctx.sample(SPP), want)
        ctx.set_lens(None if how == "none" else (0.0, 1.0))
        assert not ctx.lens_info().any()
        # mfx_launch_info (pool_max, the slots the free memory allows for this context's bytes per slot, included)
        assert _shapes(ctx, pool_max=True) == shapes and _shapes(ctx) == _shapes(never)
        assert ctx.build_info()["digest"] == digest == never.build_info()["digest"]
        ci = ctx.camera_info()
        assert ci["eps_built"] == ci["eps_needed"] == never.camera_info()["eps_built"]
        ctx.accum_clear()
        ctx.trace_accumulate(SPP, 0)
        assert np.array_equal(ctx.accum_read_mean(float(SPP)), want)
        assert np.array_equal(never.sample(SPP), want)
        assert np.array_equal(ctx.ray_counts()[:3], never.ray_counts()[:3])
        assert ctx.launch_info()["camera_packets"] == never.launch_info()["camera_packets"]
        assert np.array_equal(ctx.render_rgba8(1), never.render_rgba8(1))  # the one-sample call's own kernel again
        ctx.set_lens(None)  # none before, none now


def test_a_lens_set_while_frames_are_held(gpu, oracle):
    a = scene("cornell", W, H)
    lens = LENS["cornell"]
    with ctx_env(a, render_ahead=4) as ah, ctx_env(a) as plain, ctx_env(a, render_ahead=4) as stay:
        for _ in range(2):
            assert np.array_equal(ah.render_rgba8(1), plain.render_rgba8(1))
            stay.render_rgba8(1)
        ah.set_lens(lens)  # two frames of the batch are still held
        plain.set_lens(lens)
        for _ in range(3):
            got = ah.render_rgba8(1)
            assert np.array_equal(got, plain.render_rgba8(1))  # the lens context's frame
            assert not np.array_equal(got, stay.render_rgba8(1))
        assert np.array_equal(ah.film_mean(), plain.film_mean())


def test_refusals_and_state(gpu, oracle):
    a, _, rad, counts, _ = restated()
    want = oracle.OracleScene(a).sample(1, SEED)
    for flags in (MFX_F_MEGAKERNEL, MFX_F_COUNT_STATS):
        with ctx_env(a, flags=flags) as ctx:
            with pytest.raises(MfxError, match=r"\(-4\).*MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS"):
                ctx.set_lens(LENS["cornell"])
            assert not ctx.lens_info().any()
            ctx.set_lens(None)  # nothing to remove: fine
            assert np.array_equal(ctx.sample(1), want)  # the context still renders
    with ctx_env(a) as ctx:
        digest = ctx.build_info()["digest"]
        for bad, what in (((-1.0, 1.0), "aperture"), ((np.inf, 1.0), "aperture"), ((np.nan, 1.0), "aperture"),
                          ((0.1, 0.0), "focus"), ((0.1, -2.0), "focus"), ((0.1, np.nan), "focus"), ((0.1, np.inf), "focus")):
            with pytest.raises(MfxError, match=r"\(-1\).*" + what):
                ctx.set_lens(bad)
        assert not ctx.lens_info().any() and ctx.build_info()["digest"] == digest  # a refused call changes nothing
        assert np.array_equal(ctx.sample(1), want)
    with ctx_env(a) as ctx:
        # mfx_temporal under a lens: MFX_E_STATE, the history as it is
        ctx.aov(1)
        frame = ctx.sample(2)
        var = np.full(W * H, 0.01)
        cnt = np.full(W * H, 2.0)
        first = ctx.temporal(frame, var, cnt, restart=True)
        ctx.set_lens(LENS["cornell"])
        ctx.aov(1)
        with pytest.raises(MfxError, match=r"\(-4\).*lens"):
            ctx.temporal(frame, var, cnt)
        ctx.accum_clear()
        ctx.trace_accumulate(SPP, 0)
        assert np.array_equal(ctx.accum_read_mean(float(SPP)), frame_of(rad, W, H, SPP))  # it still renders
        ctx.set_lens(None)
        ctx.aov(1)
        again = ctx.temporal(frame, var, cnt)  # the history survived the lens: the same view takes it
        assert first[3] == 0 and again[3] > 0 and np.all(np.isfinite(again[0]))
