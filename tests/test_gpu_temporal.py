"""mfx_temporal on the GPU, bit for bit (every comparison is array_equal): the merged frame, variance and
counts, the number of accepted pixels and the RGBA8 post are the numpy statement of the rule
(mafrixraytracing_amd/temporal.py, reference_temporal) applied to the same inputs, the features mfx_aov
returned and the cameras mfx_camera_info reports; the history it carries from call to call is the one the
library keeps on the device."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED, scene
from denoise_var_helpers import mean_and_moments, pixel_counts
from temporal_helpers import moved, with_camera

pytestmark = pytest.mark.gpu

W, H = 44, 36
ADAPTIVE = (4, 16, 4, 0.25, 0.01)  # min, max, step, rel_error, abs_floor
MOVE1 = dict(dpos=(0.2, 0.1, -0.5), ddir=(0.05, -0.05, 0.0))  # both towards the scene: in place
MOVE2 = dict(dpos=(0.1, 0.15, -0.3), ddir=(-0.05, 0.0, 0.0))


def _ctx(a, **kw):
    from mafrixraytracing_amd.native import NativeContext
    return NativeContext(a, seed=SEED, **kw)


def _cfg(**kw):
    from mafrixraytracing_amd.temporal import TemporalConfig
    return TemporalConfig(**{**dict(tol_depth=0.1, tol_normal2=0.01, max_history=24.0), **kw})


def _check(oracle, got, ref, w, h, what):
    frame, var, cnt, acc, rgba = got
    assert np.array_equal(frame, ref[0]), (what, np.abs(frame - ref[0]).max())
    assert np.array_equal(var, ref[1]), what
    assert np.array_equal(cnt, ref[2]), what
    assert acc == ref[3], (what, acc, ref[3])
    assert np.array_equal(rgba, oracle.post_rgba8(ref[0], w, h)), what
    return ref[4]


@pytest.mark.parametrize("w,h", [(W, H), (16, 8)])
def test_host_source(gpu, oracle, w, h):
    from mafrixraytracing_amd.temporal import reference_temporal
    a = scene("cornell", w, h)
    rng = np.random.default_rng(3)
    npix = w * h
    with _ctx(a) as c:
        def step(hist, cfg, restart=False, spp=2):
            feat = c.aov(2, 100)
            frame = c.sample(spp)
            var = rng.uniform(0.0, 0.05, npix)
            cnt = np.full(npix, float(spp))
            cnt[::9] = 1.0
            cam = c.camera_info()["derived"]
            ref = reference_temporal(frame, var, cnt, feat, cam, hist, w, h, cfg, restart=restart)
            got = c.temporal(frame, var, cnt, cfg=cfg, restart=restart, want_rgba=True)
            assert c.last_temporal_ms > 0
            return got, ref

        got, ref = step(None, _cfg(), spp=8)  # no history yet: every pixel passes through
        hist = _check(oracle, got, ref, w, h, "first")
        assert ref[3] == 0
        got, ref = step(hist, _cfg())  # the same camera: every fully covered pixel takes its own history
        hist = _check(oracle, got, ref, w, h, "same camera")
        assert ref[3] > npix // 4 and (ref[2] > 2.0).any()
        c.set_camera(moved(a.camera, **MOVE1))
        got, ref = step(hist, _cfg())
        hist = _check(oracle, got, ref, w, h, "moved")
        assert 0 < ref[3] < npix  # some pixels came into view or changed surface
        c.set_camera(moved(moved(a.camera, **MOVE1), **MOVE2))  # a second move: the other history buffer is read
        got, ref = step(hist, _cfg(tol_depth=0.03, max_history=4.0))
        hist = _check(oracle, got, ref, w, h, "moved twice")
        assert 0 < ref[3] < npix
        got, ref = step(hist, _cfg(), restart=True)
        hist = _check(oracle, got, ref, w, h, "restart")
        assert ref[3] == 0
        got, ref = step(hist, _cfg(tol_depth=0.0, tol_normal2=0.0))  # the restarted history is this view's
        _check(oracle, got, ref, w, h, "after restart")


def test_adaptive_source(gpu, oracle):
    from mafrixraytracing_amd.denoise import variance_of_mean
    from mafrixraytracing_amd.temporal import reference_temporal
    a = scene("cornell", W, H)
    b = with_camera(a, moved(a.camera, **MOVE1))
    with _ctx(a) as c:
        hist = None
        base = 0
        for view, what in ((a, "first"), (a, "same camera"), (b, "moved")):
            if view is b:
                c.set_camera(b.camera)
            feat = c.aov(2, 200)
            frame, tiles = c.sample_adaptive(*ADAPTIVE)
            n = pixel_counts(tiles, W, H)
            o = oracle.OracleScene(view)
            frames = np.stack([o.sample(1, SEED, sample_base=base + s) for s in range(ADAPTIVE[1])])
            mean, S1, S2 = mean_and_moments(frames, n)
            assert np.array_equal(frame, mean), what  # the inputs are the oracle's
            ref = reference_temporal(frame, variance_of_mean(S1, S2, n), n.astype(np.float64), feat,
                                     c.camera_info()["derived"], hist, W, H, _cfg())
            hist = _check(oracle, c.temporal(None, cfg=_cfg(), want_rgba=True), ref, W, H, what)
            assert (ref[3] > 0) == (what != "first")
            base += ADAPTIVE[1]
        assert len(set(tiles.ravel().tolist())) > 1  # differing counts entered the merge


def test_denoise_var_filters_the_history_where_it_lies(gpu):
    from mafrixraytracing_amd.abi import MfxDenoiseVarCfg, MfxError
    from mafrixraytracing_amd.denoise import DenoiseVarConfig
    a = scene("cornell", W, H)
    npix = W * H
    rng = np.random.default_rng(4)
    with _ctx(a) as c:
        c.aov(2)
        with pytest.raises(MfxError, match=r"\(-4\)"):  # no history yet
            c.denoise_var(source="temporal")
        for k in range(2):
            frame, var, cnt, acc = c.temporal(c.sample(2), rng.uniform(0, 0.05, npix), np.full(npix, 2.0), cfg=_cfg())
            for cfg in (DenoiseVarConfig(), DenoiseVarConfig(iterations=1), DenoiseVarConfig(iterations=4, sigma_luma=0.0)):
                want = c.denoise_var(frame, variance=var, cfg=cfg, want_rgba=True, want_variance=True)
                got = c.denoise_var(cfg=cfg, want_rgba=True, want_variance=True, source="temporal")
                for g, x in zip(got, want):
                    assert np.array_equal(g, x), (k, cfg)
        assert acc > 0
        # host pointers do not fit the source
        cfg = MfxDenoiseVarCfg(iterations=3, source=3, sigma_normal=0.1, sigma_depth=0.02, sigma_albedo=0.05,
                               sigma_luma=4.0, luma_floor=1e-6)
        from mafrixraytracing_amd.abi import dptr
        assert c.lib.mfx_denoise_var(c._h, C.byref(cfg), dptr(frame), dptr(var), None, None, None, None) == -1
        assert c.lib.mfx_denoise_var(c._h, C.byref(cfg), None, None, None, None, None, None) == 0
        # a history merged under another camera than the features': mfx_temporal has to run again
        c.set_camera(moved(a.camera, **MOVE1))
        c.aov(2)
        with pytest.raises(MfxError, match=r"\(-4\)"):
            c.denoise_var(source="temporal")
        c.temporal(c.sample(2), var, cnt, cfg=_cfg())
        c.denoise_var(source="temporal")


def test_it_leaves_the_context_alone(gpu):
    a = scene("cornell", W, H)
    npix = W * H

    def run(with_temporal):
        with _ctx(a) as ctx:
            ctx.render_rgba8(1)
            ctx.aov(4)
            frame, tiles = ctx.sample_adaptive(*ADAPTIVE)
            before = ctx.denoise_var(None, want_variance=True)
            if with_temporal:
                first = ctx.temporal(None, cfg=_cfg(), restart=True)
                ctx.temporal(frame, np.full(npix, 0.01), np.full(npix, 3.0), cfg=_cfg())
                # the accumulator, the moments and the tiles' counts are as they were: the same bits again
                for x, y in zip(first, ctx.temporal(None, cfg=_cfg(), restart=True)):
                    assert np.array_equal(x, y)
                for x, y in zip(before, ctx.denoise_var(None, want_variance=True)):
                    assert np.array_equal(x, y)
            resumed = ctx.sample_adaptive_resume(24, 4, 0.1, 0.01)
            return ctx.film_mean(), ctx.ray_counts(), resumed[0], resumed[1], ctx.sample(1)

    for got, want in zip(run(True), run(False)):
        assert np.array_equal(got, want)


def test_refusals(gpu):
    from mafrixraytracing_amd.abi import MfxTemporalCfg, dptr
    a = scene("cornell", 16, 8)
    npix = 16 * 8
    frame, var, cnt = np.zeros((npix, 4)), np.zeros(npix), np.ones(npix)
    HOST = dict(color=frame, variance=var, count=cnt)
    DEV = dict(source=2, color=None, variance=None, count=None)

    def temporal(ctx, color=frame, variance=var, count=cnt, **kw):
        d = dict(source=0, restart=0, tol_depth=0.1, tol_normal2=0.01, max_history=16.0)
        reserved = kw.pop("reserved", (0, 0))
        d.update(kw)
        cfg = MfxTemporalCfg(**d)
        cfg.reserved[0], cfg.reserved[1] = reserved
        p = [dptr(x) if x is not None else None for x in (color, variance, count)]
        rc = ctx.lib.mfx_temporal(ctx._h, C.byref(cfg), p[0], p[1], p[2], None, None, None, None, None, None)
        return rc, ctx.lib.mfx_last_error()

    with _ctx(a) as ctx:
        for src in (HOST, DEV):
            rc, err = temporal(ctx, **src)
            assert rc == -4 and b"mfx_aov" in err, src  # MFX_E_STATE: no feature buffers yet
        ctx.aov(2)
        rc, err = temporal(ctx, **DEV)
        assert rc == -4 and b"mfx_sample_adaptive" in err  # MFX_E_STATE: no adaptive result yet
        assert temporal(ctx)[0] == 0  # every output pointer may be NULL
        ctx.sample_adaptive(2, 4, 2, 0.25, 0.01)
        assert temporal(ctx, **DEV)[0] == 0
        ctx.accum_clear()
        assert temporal(ctx, **DEV)[0] == -4
        ctx.sample_adaptive(2, 4, 2, 0.25, 0.01)
        nan, inf = float("nan"), float("inf")
        for bad in (dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(tol_depth=-1.0), dict(tol_depth=nan),
                    dict(tol_depth=inf), dict(tol_normal2=-0.1), dict(tol_normal2=nan), dict(max_history=0.0),
                    dict(max_history=-1.0), dict(max_history=nan), dict(max_history=inf)):
            for src in (HOST, DEV):
                rc, err = temporal(ctx, **{**src, **bad})
                assert rc == -1 and b"mfx_temporal" in err, (src, bad)  # MFX_E_INVALID
        for bad in (dict(source=1), dict(source=3), dict(source=-1), dict(color=None), dict(variance=None),
                    dict(count=None), dict(source=2), dict(source=2, color=None), dict(source=2, color=None, variance=None),
                    dict(count=np.where(np.arange(npix) == 5, inf, 1.0)), dict(count=np.where(np.arange(npix) == 7, nan, 1.0))):
            rc, err = temporal(ctx, **bad)
            assert rc == -1 and b"mfx_temporal" in err, bad
        assert ctx.lib.mfx_temporal(ctx._h, None, dptr(frame), dptr(var), dptr(cnt), None, None, None, None, None, None) == -1
        assert temporal(ctx, **DEV)[0] == 0  # none of the refused calls ended the adaptive result
    for kw in (dict(devices=[0, 0]), dict(part_index=0, part_count=2)):
        with _ctx(a, **kw) as ctx:
            for src in (HOST, DEV):
                rc, err = temporal(ctx, **src)
                assert rc == -4 and b"mfx_temporal" in err, (kw, src)  # MFX_E_STATE
