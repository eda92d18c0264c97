"""mfx_denoise_var on the GPU, bit for bit (every comparison is array_equal): from the adaptive
sampler's result as it lies on the device, the filtered image and variance are the numpy statement of
the rule (mafrixraytracing_amd/denoise.py, reference_denoise_var) applied to the frame the sampler
returned, the variance of the mean that the CPU oracle's one-sample frames give for the tiles' counts,
and the features mfx_aov returned; the RGBA8 frame is the oracle's post of that image."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED, scene
from denoise_helpers import smallest_with_a_square
from denoise_var_helpers import mean_and_moments, oracle_sample_frames, pixel_counts

pytestmark = pytest.mark.gpu

W, H = 44, 36  # both sides leave edge tiles; 1584 pixels: seven blocks, the last one partly filled
ADAPTIVE = (4, 16, 4, 0.25, 0.01)  # min, max, step, rel_error, abs_floor


def _ctx(a, **kw):
    from mafrixraytracing_amd.native import NativeContext
    return NativeContext(a, seed=SEED, **kw)


def _cfg(**kw):
    from mafrixraytracing_amd.denoise import DenoiseVarConfig
    return DenoiseVarConfig(**kw)


def _sampled(ctx, oracle, name, w, h):
    """aov(4) and the adaptive frame of a fresh context (samples 0...), with the variance of the mean the
    oracle's one-sample frames give for the counts the tiles got."""
    from mafrixraytracing_amd.denoise import variance_of_mean
    feat = ctx.aov(4)
    frame, tiles = ctx.sample_adaptive(*ADAPTIVE)
    n = pixel_counts(tiles, w, h)
    mean, S1, S2 = mean_and_moments(oracle_sample_frames(oracle, name, w, h, ADAPTIVE[1]), n)
    assert np.array_equal(frame, mean)  # the inputs are the oracle's
    return feat, frame, tiles, variance_of_mean(S1, S2, n)


@pytest.mark.parametrize("w,h", [(W, H), (5, 3), (1, 1)])
def test_parity_from_the_device(gpu, oracle, w, h):
    from mafrixraytracing_amd.denoise import reference_denoise_var
    with _ctx(scene("cornell", w, h)) as ctx:
        feat, frame, tiles, var = _sampled(ctx, oracle, "cornell", w, h)
        if (w, h) == (W, H):
            assert len(set(tiles.ravel().tolist())) > 1  # differing counts: one divisor would not do
            assert (var > 0).any() and (var == 0).any()  # lit pixels, and pixels whose samples all agree
        # defaults; step 16 past every edge; the luminance term off
        for cfg in (_cfg(), _cfg(iterations=5), _cfg(sigma_luma=0.0)):
            ref, rvar = reference_denoise_var(frame, var, feat, w, h, cfg)
            got, rgba, gvar = ctx.denoise_var(None, cfg=cfg, want_rgba=True, want_variance=True)
            assert ctx.last_denoise_ms > 0
            assert np.array_equal(got, ref), (cfg, np.abs(got - ref).max())
            assert np.array_equal(got[:, 3], np.ones(w * h))
            assert np.array_equal(gvar, rvar), (cfg, np.abs(gvar - rvar).max())
            assert np.array_equal(rgba, oracle.post_rgba8(ref, w, h)), cfg
        assert not np.array_equal(ctx.denoise_var(None), frame) or w * h == 1  # it filters


def test_sources_agree(gpu, oracle):
    with _ctx(scene("cornell", W, H)) as ctx:
        feat, frame, tiles, var = _sampled(ctx, oracle, "cornell", W, H)
        dev = ctx.denoise_var(None, want_rgba=True, want_variance=True)
        host = ctx.denoise_var(frame, variance=var, want_rgba=True, want_variance=True)
        for d, h in zip(dev, host):
            assert np.array_equal(d, h)
        # the host call staged its inputs in buffers of the call's own: the device source still stands
        for d, h in zip(dev, ctx.denoise_var(None, want_rgba=True, want_variance=True)):
            assert np.array_equal(d, h)


@pytest.mark.parametrize("name", ["spot", "spot16_instanced@2l"])
def test_parity_other_scenes(gpu, oracle, name):
    """Spheres' and meshes' features (spot), and the features of a two-level scene."""
    from mafrixraytracing_amd.denoise import reference_denoise_var
    with _ctx(scene(name, W, H)) as ctx:
        feat, frame, tiles, var = _sampled(ctx, oracle, name, W, H)
        got, gvar = ctx.denoise_var(None, want_variance=True)
    ref, rvar = reference_denoise_var(frame, var, feat, W, H, _cfg())
    assert np.array_equal(got, ref) and np.array_equal(gvar, rvar)


def test_sigma_luma_zero_is_mfx_denoise(gpu):
    """With the luminance term off the colour is mfx_denoise's (sigma_color 0) of the adaptive frame."""
    from mafrixraytracing_amd.denoise import DenoiseConfig
    with _ctx(scene("cornell", W, H)) as ctx:
        ctx.aov(4)
        frame, tiles = ctx.sample_adaptive(*ADAPTIVE)
        for it in (1, 3, 5):
            want = ctx.denoise(frame, cfg=DenoiseConfig(iterations=it))
            assert np.array_equal(ctx.denoise_var(None, cfg=_cfg(iterations=it, sigma_luma=0.0)), want), it


def test_it_leaves_the_context_alone(gpu):
    a = scene("cornell", W, H)

    def run(with_denoise):
        with _ctx(a) as ctx:
            ctx.render_rgba8(1)
            ctx.aov(4)
            frame, tiles = ctx.sample_adaptive(*ADAPTIVE)
            if with_denoise:
                first = ctx.denoise_var(None, want_rgba=True, want_variance=True)
                ctx.denoise_var(frame, variance=np.full(W * H, 0.01))
                # the accumulator, the moments and the tiles' counts are as they were: the same bits again
                for x, y in zip(first, ctx.denoise_var(None, want_rgba=True, want_variance=True)):
                    assert np.array_equal(x, y)
            return ctx.film_mean(), ctx.ray_counts(), ctx.sample(1)

    for got, want in zip(run(True), run(False)):
        assert np.array_equal(got, want)


def test_refusals(gpu):
    from mafrixraytracing_amd.abi import MfxDenoiseVarCfg, dptr
    a = scene("cornell", 16, 16)
    frame = np.zeros((16 * 16, 4))
    variance = np.zeros(16 * 16)
    HOST = dict(color=frame, variance=variance)
    DEV = dict(source=2, color=None, variance=None)

    def denoise_var(ctx, color=frame, variance=variance, **kw):
        d = dict(iterations=3, source=0, sigma_normal=0.1, sigma_depth=0.02, sigma_albedo=0.05, sigma_luma=4.0,
                 luma_floor=1e-6)
        reserved = kw.pop("reserved", (0, 0))
        d.update(kw)
        cfg = MfxDenoiseVarCfg(**d)
        cfg.reserved[0], cfg.reserved[1] = reserved
        rc = ctx.lib.mfx_denoise_var(ctx._h, C.byref(cfg), dptr(color) if color is not None else None,
                                     dptr(variance) if variance is not None else None, None, None, None, None)
        return rc, ctx.lib.mfx_last_error()

    def adaptive(ctx):
        ctx.sample_adaptive(2, 4, 2, 0.25, 0.01)

    with _ctx(a) as ctx:
        for src in (HOST, DEV):
            rc, err = denoise_var(ctx, **src)
            assert rc == -4 and b"mfx_aov" in err, src  # MFX_E_STATE: no feature buffers yet
        ctx.aov(2)
        rc, err = denoise_var(ctx, **DEV)
        assert rc == -4 and b"mfx_sample_adaptive" in err  # MFX_E_STATE: no adaptive result yet
        assert denoise_var(ctx)[0] == 0  # the host source needs none; every output pointer may be NULL
        adaptive(ctx)
        assert denoise_var(ctx, **DEV)[0] == 0  # every output pointer may be NULL
        # whatever writes or swaps the accumulator ends the adaptive result
        for spoil in (lambda: ctx.accum_clear(), lambda: ctx.sample(1), lambda: ctx.trace_accumulate(1, 40)):
            adaptive(ctx)
            assert denoise_var(ctx, **DEV)[0] == 0
            spoil()
            rc, err = denoise_var(ctx, **DEV)
            assert rc == -4 and b"mfx_sample_adaptive" in err
            assert denoise_var(ctx)[0] == 0  # the host source does not depend on it
        adaptive(ctx)
        nan, inf = float("nan"), float("inf")
        for bad in (dict(iterations=0), dict(iterations=9), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
                    dict(sigma_normal=-0.1), dict(sigma_depth=nan), dict(sigma_albedo=inf), dict(sigma_luma=-1.0),
                    dict(sigma_luma=nan), dict(sigma_luma=inf), dict(luma_floor=0.0), dict(luma_floor=-1e-6),
                    dict(luma_floor=nan), dict(luma_floor=inf)):
            for src in (HOST, DEV):  # a bad struct field, whatever the source
                rc, err = denoise_var(ctx, **{**src, **bad})
                assert rc == -1 and b"mfx_denoise_var" in err, (src, bad)  # MFX_E_INVALID
        for bad in (dict(source=1), dict(source=3), dict(source=-1), dict(source=1, color=None, variance=None),
                    # pointers that do not fit the source
                    dict(color=None), dict(variance=None), dict(color=None, variance=None),
                    dict(source=2), dict(source=2, variance=None), dict(source=2, color=None)):
            rc, err = denoise_var(ctx, **bad)
            assert rc == -1 and b"mfx_denoise_var" in err, bad  # MFX_E_INVALID
        assert ctx.lib.mfx_denoise_var(ctx._h, None, dptr(frame), dptr(variance), None, None, None, None) == -1
        assert denoise_var(ctx, **DEV)[0] == 0  # none of the refused calls ended the adaptive result
    for kw in (dict(devices=[0, 0]), dict(part_index=0, part_count=2)):
        with _ctx(a, **kw) as ctx:
            for src in (HOST, DEV):
                rc, err = denoise_var(ctx, **src)
                assert rc == -4 and b"mfx_denoise_var" in err, (kw, src)  # MFX_E_STATE


def test_refusals_of_sigmas_whose_square_is_zero(gpu):
    """sigma_normal, sigma_depth or sigma_albedo > 0 with a square of 0 in FP64 made every pixel of the
    colour and the variance NaN (the centre tap's term was 0/0): MFX_E_INVALID now. The smallest sigma
    with a non-zero square is accepted, finite, and the reference's bits; sigma_luma needs no such rule
    (lden = 0 * Vf + luma_floor > 0)."""
    from mafrixraytracing_amd.abi import MfxDenoiseVarCfg, dptr
    from mafrixraytracing_amd.denoise import reference_denoise_var
    w = h = 16
    s_min, s_below = smallest_with_a_square()

    def rc_of(ctx, frame, variance, **kw):
        d = dict(iterations=3, source=0, sigma_normal=0.1, sigma_depth=0.02, sigma_albedo=0.05, sigma_luma=4.0,
                 luma_floor=1e-6)
        d.update(kw)
        cfg = MfxDenoiseVarCfg(**d)
        out, vout = np.full((w * h, 4), -1.0), np.full(w * h, -1.0)
        rc = ctx.lib.mfx_denoise_var(ctx._h, C.byref(cfg), dptr(frame), dptr(variance), dptr(out), dptr(vout), None, None)
        return rc, ctx.lib.mfx_last_error(), out, vout

    with _ctx(scene("cornell", w, h)) as ctx:
        feat = ctx.aov(4)
        frame = ctx.sample(4)
        var = np.random.default_rng(11).uniform(0.0, 0.05, w * h)
        var[::7] = 0.0
        for name in ("sigma_normal", "sigma_depth", "sigma_albedo"):
            for bad in (1e-163, 1e-170, 5e-324, s_below):
                rc, err, out, vout = rc_of(ctx, frame, var, **{name: bad})
                assert rc == -1 and b"mfx_denoise_var" in err, (name, bad)  # MFX_E_INVALID
                assert (out == -1.0).all() and (vout == -1.0).all()  # nothing was written
            for ok in ({name: s_min}, {name: s_min, "sigma_luma": 1e-170}):
                rc, err, out, vout = rc_of(ctx, frame, var, **ok)
                assert rc == 0, (ok, err)
                assert np.isfinite(out).all() and np.isfinite(vout).all(), ok
                ref, rvar = reference_denoise_var(frame, var, feat, w, h, _cfg(**ok))
                assert np.array_equal(out, ref) and np.array_equal(vout, rvar), ok
        for luma in (1e-170, 5e-324, s_below, s_min):
            rc, err, out, vout = rc_of(ctx, frame, var, sigma_luma=luma)
            assert rc == 0, (luma, err)
            ref, rvar = reference_denoise_var(frame, var, feat, w, h, _cfg(sigma_luma=luma))
            assert np.isfinite(ref).all() and np.isfinite(rvar).all()
            assert np.array_equal(out, ref) and np.array_equal(vout, rvar), luma
