"""mfx_aov and mfx_denoise on the GPU, bit for bit (every comparison is array_equal): the feature
buffers are the host composition of the CPU oracle's camera ray, RNG draws and closest hit
(tests/denoise_helpers.py), the filtered image is the numpy statement of the rule
(mafrixraytracing_amd/denoise.py) applied to the same frame and features, and the RGBA8 frame is the
oracle's post of that image."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED, scene
from denoise_helpers import oracle_features, smallest_with_a_square

pytestmark = pytest.mark.gpu

W, H = 44, 36  # both sides leave edge tiles; 1584 pixels: seven blocks, the last one partly filled


def _ctx(a, **kw):
    from mafrixraytracing_amd.native import NativeContext
    return NativeContext(a, seed=SEED, **kw)


def _cfg(**kw):
    from mafrixraytracing_amd.denoise import DenoiseConfig
    return DenoiseConfig(**kw)


PLAIN = dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, sigma_color=0.0)


# ---- feature buffers --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "two_spheres_plane", "spot", "spot16_instanced", "spot16_instanced@2l"])
def test_aov_parity(gpu, oracle, name):
    ref = oracle_features(oracle, name, W, H, 3, 5)
    frac = ref[:, 7]
    assert ((frac > 0) & (frac < 1)).any() and (frac == 0).any()  # silhouettes and full misses are exercised
    assert np.array_equal(ref[frac == 0], np.zeros(((frac == 0).sum(), 8)))
    with _ctx(scene(name, W, H)) as ctx:
        if name.endswith("@2l"):
            assert ctx.instancing_info()["instances"] > 0  # traced two-level
        got = ctx.aov(3, sample_base=5)
        assert ctx.last_aov_ms > 0
    assert got.shape == (W * H, 8)
    assert np.array_equal(got, ref), (name, np.abs(got - ref).max(axis=0))


def test_aov_leaves_the_context_alone(gpu):
    a = scene("cornell", W, H)

    def run(with_aov):
        with _ctx(a) as ctx:
            ctx.render_rgba8(1)
            ctx.render_rgba8(1)
            ctx.sample(2)
            if with_aov:
                ctx.aov(3, sample_base=1)
            return ctx.film_mean(), ctx.ray_counts(), ctx.sample(1)

    for got, want in zip(run(True), run(False)):
        assert np.array_equal(got, want)


# ---- the filter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(W, H), (5, 3), (1, 1)])
def test_denoise_parity(gpu, oracle, w, h):
    from mafrixraytracing_amd.denoise import reference_denoise
    with _ctx(scene("cornell", w, h)) as ctx:
        feat = ctx.aov(4)
        frame = ctx.sample(4)
        # defaults; step 16 past every edge with the colour term on; the plain B3-spline a-trous
        for cfg in (_cfg(), _cfg(iterations=5, sigma_color=1.0), _cfg(**PLAIN)):
            ref = reference_denoise(frame, feat, w, h, cfg)
            got, rgba = ctx.denoise(frame, cfg=cfg, want_rgba=True)
            assert ctx.last_denoise_ms > 0
            assert np.array_equal(got, ref), (cfg, np.abs(got - ref).max())
            assert np.array_equal(got[:, 3], np.ones(w * h))
            assert np.array_equal(rgba, oracle.post_rgba8(ref, w, h)), cfg
        assert not np.array_equal(ctx.denoise(frame), frame) or w * h == 1  # it filters


@pytest.mark.parametrize("name", ["spot", "spot16_instanced@2l"])
def test_denoise_parity_other_scenes(gpu, name):
    """Spheres' and meshes' features (spot), and the features of a two-level scene."""
    from mafrixraytracing_amd.denoise import reference_denoise
    with _ctx(scene(name, W, H)) as ctx:
        feat = ctx.aov(4)
        frame = ctx.sample(4)
        got = ctx.denoise(frame)
    assert np.array_equal(got, reference_denoise(frame, feat, W, H, _cfg()))


def test_sources_agree(gpu):
    from mafrixraytracing_amd.denoise import reference_denoise
    with _ctx(scene("cornell", W, H)) as ctx:
        feat = ctx.aov(4)
        frame = ctx.sample(4)
        from_host = ctx.denoise(frame)
        from_accum, rgba = ctx.denoise(None, count=4, want_rgba=True)
        assert np.array_equal(from_accum, from_host)
        assert np.array_equal(ctx.accum_read_mean(4), frame)  # the accumulator is left as it was
        assert np.array_equal(ctx.denoise(frame, want_rgba=True)[1], rgba)
        # an adaptive frame (per-tile counts) filters like any other host frame
        adaptive, tiles = ctx.sample_adaptive(4, 16, 4, 0.25, 0.01)
        assert len(set(tiles.ravel().tolist())) > 1
        assert np.array_equal(ctx.denoise(adaptive), reference_denoise(adaptive, feat, W, H, _cfg()))


def test_denoise_leaves_the_context_alone(gpu):
    a = scene("cornell", W, H)

    def run(with_denoise):
        with _ctx(a) as ctx:
            ctx.render_rgba8(1)
            frame = ctx.sample(2)
            if with_denoise:
                ctx.aov(2)
                ctx.denoise(frame)
                ctx.denoise(None, count=2)
            return ctx.film_mean(), ctx.ray_counts(), ctx.accum_read_mean(2), ctx.sample(1)

    for got, want in zip(run(True), run(False)):
        assert np.array_equal(got, want)


# ---- refusals ---------------------------------------------------------------------------------------
def test_refusals(gpu):
    from mafrixraytracing_amd.abi import MfxDenoiseCfg, dptr
    a = scene("cornell", 16, 16)
    frame = np.zeros((16 * 16, 4))

    def aov(ctx, spp=2, base=0):
        return ctx.lib.mfx_aov(ctx._h, spp, base, None, None), ctx.lib.mfx_last_error()

    def denoise(ctx, color=frame, **kw):
        d = dict(iterations=3, source=0, count=0.0, sigma_normal=0.1, sigma_depth=0.02, sigma_albedo=0.05, sigma_color=0.0)
        reserved = kw.pop("reserved", (0, 0))
        d.update(kw)
        cfg = MfxDenoiseCfg(**d)
        cfg.reserved[0], cfg.reserved[1] = reserved
        rc = ctx.lib.mfx_denoise(ctx._h, C.byref(cfg), dptr(color) if color is not None else None, None, None, None)
        return rc, ctx.lib.mfx_last_error()

    with _ctx(a) as ctx:
        rc, err = denoise(ctx)
        assert rc == -4 and b"mfx_aov" in err  # MFX_E_STATE: no feature buffers yet
        for bad in (dict(spp=0), dict(spp=-3), dict(base=-1)):
            rc, err = aov(ctx, **bad)
            assert rc == -1 and err, bad  # MFX_E_INVALID
        assert aov(ctx)[0] == 0  # every output pointer may be NULL
        for bad in (dict(iterations=0), dict(iterations=9), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
                    dict(sigma_normal=-0.1), dict(sigma_depth=float("nan")), dict(sigma_albedo=float("inf")),
                    dict(sigma_color=-1.0), dict(sigma_color=float("nan")), dict(color=None),
                    dict(source=1, color=None, count=0.0), dict(source=1, color=None, count=-2.0),
                    dict(source=1, color=None, count=float("nan")), dict(source=2), dict(source=-1)):
            rc, err = denoise(ctx, **bad)
            assert rc == -1 and b"mfx_denoise" in err, bad  # MFX_E_INVALID
        assert ctx.lib.mfx_denoise(ctx._h, None, dptr(frame), None, None, None) == -1
        assert denoise(ctx)[0] == 0  # every output pointer may be NULL
        assert denoise(ctx, source=1, color=None, count=1.0)[0] == 0
    for kw in (dict(devices=[0, 0]), dict(part_index=0, part_count=2)):
        with _ctx(a, **kw) as ctx:
            rc, err = aov(ctx)
            assert rc == -4 and b"mfx_aov" in err, kw  # MFX_E_STATE
            rc, err = denoise(ctx)
            assert rc == -4 and b"mfx_denoise" in err, kw


def test_refusals_of_sigmas_whose_divisor_is_zero(gpu):
    """A sigma > 0 whose square is 0 in FP64, or a sigma_color whose (sc*sc) * 0.25^i reaches 0 at an
    iteration that runs, made every pixel NaN (the centre tap's term was 0/0): MFX_E_INVALID now. Just
    above the limit the call is accepted, finite, and the reference's bits."""
    from mafrixraytracing_amd.abi import MfxDenoiseCfg, dptr
    from mafrixraytracing_amd.denoise import reference_denoise
    w = h = 16
    s_min, s_below = smallest_with_a_square()

    def rc_of(ctx, frame, **kw):
        d = dict(iterations=3, source=0, count=0.0, sigma_normal=0.1, sigma_depth=0.02, sigma_albedo=0.05, sigma_color=0.0)
        d.update(kw)
        cfg = MfxDenoiseCfg(**d)
        out = np.full((w * h, 4), -1.0)
        rc = ctx.lib.mfx_denoise(ctx._h, C.byref(cfg), dptr(frame), dptr(out), None, None)
        return rc, ctx.lib.mfx_last_error(), out

    with _ctx(scene("cornell", w, h)) as ctx:
        feat = ctx.aov(4)
        frame = ctx.sample(4)
        for name in ("sigma_normal", "sigma_depth", "sigma_albedo", "sigma_color"):
            it = 1 if name == "sigma_color" else 3  # (a later iteration's 0.25^i would take sc2 to 0)
            for bad in (1e-163, 1e-170, 5e-324, s_below):
                rc, err, out = rc_of(ctx, frame, iterations=it, **{name: bad})
                assert rc == -1 and b"mfx_denoise" in err, (name, bad)  # MFX_E_INVALID
                assert (out == -1.0).all()  # nothing was written
            rc, err, out = rc_of(ctx, frame, iterations=it, **{name: s_min})
            assert rc == 0, (name, err)
            assert np.isfinite(out).all(), name
            cfg = _cfg(iterations=it, **{name: s_min})
            assert np.array_equal(out, reference_denoise(frame, feat, w, h, cfg)), name
            assert np.array_equal(ctx.denoise(frame, cfg=cfg), out)
        # sc2 = 1e-320 survives the first iteration's 0.25^0 and is 0 by the seventh
        assert rc_of(ctx, frame, iterations=8, sigma_color=1e-160)[0] == -1
        rc, err, out = rc_of(ctx, frame, iterations=1, sigma_color=1e-160)
        assert rc == 0 and np.isfinite(out).all()
        assert np.array_equal(out, reference_denoise(frame, feat, w, h, _cfg(iterations=1, sigma_color=1e-160)))
        # the last iteration at which it is still non-zero, found as the library finds it
        sc2, quarter, last = 1e-160 * 1e-160, 1.0, 0
        while sc2 * quarter != 0.0:
            last += 1
            quarter = quarter * 0.25
        assert 1 < last < 8
        assert rc_of(ctx, frame, iterations=last + 1, sigma_color=1e-160)[0] == -1
        rc, err, out = rc_of(ctx, frame, iterations=last, sigma_color=1e-160)
        assert rc == 0 and np.isfinite(out).all()
        assert np.array_equal(out, reference_denoise(frame, feat, w, h, _cfg(iterations=last, sigma_color=1e-160)))
