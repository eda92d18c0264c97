"""mfx_sample_adaptive_resume on the GPU, bit for bit (every comparison is array_equal): against
mfx_sample_adaptive itself (a call equals its first pass plus a resume, and the chain of one-pass
resumes), and against the CPU oracle through the rule stated on the host
(mafrixraytracing_amd/adaptive.py, reference_resume): the counts, every pixel (the oracle's samples
0 .. n - 1 summed in order and divided by its tile's n), the RGBA8 frame and the ray counters over
exactly the (pixel, sample) set a resume added. The mixed-count cases are the ones in which the tiles
of one pass start from different counts and get different shares: what the per-tile sample bases of
the listed trace exist for.

As in tests/test_gpu_adaptive.py, a decision whose two sides lie within ~1e-9 of each other could fall
either way with the wave's summation order, so every case asserts that the reference's smallest gap,
the entry checks included, is above 1e-6."""
import ctypes as C
import os

import numpy as np
import pytest

from adaptive_helpers import check_parity, reference, run
from adaptive_resume_helpers import added_paths_stats, first_result, one_pass_chain
from conftest import SEED, scene
from denoise_var_helpers import oracle_sample_frames, pixel_counts

pytestmark = pytest.mark.gpu

W, H = 44, 36  # both sides leave edge tiles
BASE = dict(min_spp=4, step_spp=4, max_spp=32, abs_floor=0.01)  # tests/test_gpu_adaptive.py's
FLOOR = BASE["abs_floor"]
MIXED_MAX, MIXED_STEP = 46, 8  # the mixed-count resume: 32 -> 46 in steps of 8, so the last step is clipped

_mixed = {}


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


def _cfg(rel_error, **kw):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig
    d = dict(BASE, rel_error=rel_error)
    d.update(kw)
    return AdaptiveConfig(d["min_spp"], d["max_spp"], d["step_spp"], d["rel_error"], d["abs_floor"])


def _rcfg(max_spp, step_spp, rel_error, max_passes=0, abs_floor=FLOOR):
    from mafrixraytracing_amd.adaptive import ResumeConfig
    return ResumeConfig(max_spp, step_spp, rel_error, abs_floor, max_passes)


def _resume(ctx, r, want_rgba=True):
    return ctx.sample_adaptive_resume(r.max_spp, r.step_spp, r.rel_error, r.abs_floor, max_passes=r.max_passes,
                                      want_rgba=want_rgba)


def _moments_view(ctx):
    """A function of the moment planes and the counts: the variance plane mfx_denoise_var derives from
    them, through one iteration without the luminance term (needs an aov call before the sampling)."""
    from mafrixraytracing_amd.denoise import DenoiseVarConfig
    return ctx.denoise_var(None, cfg=DenoiseVarConfig(iterations=1, sigma_luma=0.0), want_variance=True)[1]


def mixed_reference(oracle, name, w, h, rel_a, rel_b):
    """sample_adaptive(4, 32, 4, rel_a), then resume(46, 8, rel_b): what both must return, the resume's
    passes one by one, and the oracle's rays over the samples the resume added. Once per case."""
    from mafrixraytracing_amd.adaptive import reference_mean
    key = (name.replace("@2l", ""), w, h, rel_a, rel_b)
    if key not in _mixed:
        cfg, r = _cfg(rel_a), _rcfg(MIXED_MAX, MIXED_STEP, rel_b)
        frames, Y, spp, S1, S2, gap = first_result(oracle, name, w, h, cfg)
        calls, (out, T1, T2), rgap = one_pass_chain(Y, w, h, spp, S1, S2, r)
        print(f"{name} {w}x{h} {rel_a} -> {rel_b}: smallest gaps {gap:.3g}, {rgap:.3g}; {spp.mean():.2f} -> {out.mean():.2f} spp")
        assert min(gap, rgap) > 1e-6, (name, gap, rgap)  # the condition on the inputs: no tile near a tie
        mean = reference_mean(frames[:MIXED_MAX], out, w, h)
        o = oracle.OracleScene(scene(name.replace("@2l", ""), w, h))
        st = added_paths_stats(o, spp, out, w, h, SEED)
        _mixed[key] = dict(cfg=cfg, r=r, spp=spp, out=out, calls=calls, mean=mean, rgba=oracle.post_rgba8(mean, w, h),
                           st=st, S1=T1, S2=T2, Y=Y)
    return _mixed[key]


def check_mixed(ctx, m, what=""):
    """The first call gives m's counts; the resume gives m's counts, pixels, RGBA8 and added rays."""
    _, tiles = run(ctx, m["cfg"], want_rgba=False)
    assert np.array_equal(tiles, m["spp"]), (what, tiles.tolist())
    ctx.ray_counts_total()  # (resets the totals)
    frame, tiles, rgba, active = _resume(ctx, m["r"])
    c = ctx.ray_counts()
    assert active == 0
    assert np.array_equal(tiles, m["out"]), (what, tiles.tolist(), m["out"].tolist())
    assert np.array_equal(frame, m["mean"]), (what, np.abs(frame - m["mean"]).max())
    assert np.array_equal(rgba, m["rgba"]), what
    assert (c[0], c[1], c[2]) == m["st"] and c[3] == c[0], (what, c[:3], m["st"])
    assert tuple(ctx.ray_counts_total()[:3]) == m["st"]
    return frame, tiles


# ---- equivalence -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,rel", [("cornell", 0.25), ("spot", 0.3)])
def test_one_call_equals_split_and_chain(gpu, oracle, name, rel):
    cfg = _cfg(rel)
    a = scene(name, W, H)
    want_next = oracle.OracleScene(a).sample(1, SEED, sample_base=cfg.max_spp)

    def outputs(ctx, res, rays):
        return dict(frame=res[0], tiles=res[1], rgba=res[2], rays=rays, total=ctx.ray_counts_total()[:4],
                    moments=_moments_view(ctx), next=ctx.sample(1))

    with _ctx(a) as ctx:
        ctx.aov(4)
        res = run(ctx, cfg)
        one = outputs(ctx, res, ctx.ray_counts()[:4])
    assert len(set(one["tiles"].ravel().tolist())) > 1  # several passes and stops
    assert np.array_equal(one["next"], want_next)
    first = _cfg(rel, max_spp=cfg.min_spp)
    with _ctx(a) as ctx:  # the first pass, then one resume without a pass limit
        ctx.aov(4)
        _, t0 = run(ctx, first, want_rgba=False)
        assert np.array_equal(t0, np.full_like(t0, cfg.min_spp))
        rays = ctx.ray_counts()[:4]
        res = _resume(ctx, _rcfg(cfg.max_spp, cfg.step_spp, rel))
        assert res[3] == 0
        split = outputs(ctx, res, rays + ctx.ray_counts()[:4])
    npass = 0
    with _ctx(a) as ctx:  # the first pass, then one-pass resumes until nothing is active
        ctx.aov(4)
        run(ctx, first, want_rgba=False)
        rays = ctx.ray_counts()[:4]
        while True:
            res = _resume(ctx, _rcfg(cfg.max_spp, cfg.step_spp, rel, max_passes=1))
            rays = rays + ctx.ray_counts()[:4]
            npass += 1
            assert npass <= 8  # (min 4, step 4, max 32: seven passes at most)
            if res[3] == 0:
                break
        chain = outputs(ctx, res, rays)
    # one pass per step up to the largest count, and a last call that finds nothing unless the budget ended the chain
    passes = (int(one["tiles"].max()) - cfg.min_spp) // cfg.step_spp
    assert passes >= 3 and npass in (passes, passes + 1)
    for other in (split, chain):
        for k, v in one.items():
            assert np.array_equal(other[k], v), k


# ---- mixed counts against the oracle ---------------------------------------------------------------

def test_mixed_counts(gpu, oracle):
    m = mixed_reference(oracle, "cornell", W, H, 0.25, 0.1)
    # the reference's passes: one with tiles of at least three distinct starting counts, one with a
    # clipped tile (fewer samples than the step) beside an unclipped one
    starts = [set(b[a != b].tolist()) for b, a, _ in m["calls"]]
    shares = [set((a - b)[a != b].tolist()) for b, a, _ in m["calls"]]
    assert max(len(s) for s in starts) >= 3, starts
    assert any(MIXED_STEP in s and min(s) < MIXED_STEP for s in shares), shares
    a = scene("cornell", W, H)
    with _ctx(a) as ctx:
        check_mixed(ctx, m)
        assert np.array_equal(ctx.sample(1), oracle.OracleScene(a).sample(1, SEED, sample_base=MIXED_MAX))


@pytest.mark.parametrize("name,rel_a", [("spot16_instanced@2l", 0.3), ("two_spheres_plane", 0.35)])
def test_mixed_counts_other_scenes(gpu, oracle, name, rel_a):
    m = mixed_reference(oracle, name, W, H, rel_a, 0.1)
    assert max(len(set(b[a != b].tolist())) for b, a, _ in m["calls"]) >= 3
    with _ctx(scene(name, W, H)) as ctx:
        if name.endswith("@2l"):
            assert ctx.instancing_info()["instances"] > 0  # traced two-level: k_extend starts the paths
        check_mixed(ctx, m, name)


@pytest.mark.parametrize("w,h", [(5, 3), (9, 8), (16, 16)])
def test_mixed_counts_small_films(gpu, oracle, w, h):
    """5x3: one tile. 9x8: a second tile one pixel wide. 16x16: 8 divides both sides, so the only
    padding windows are those of clipped tiles."""
    m = mixed_reference(oracle, "cornell", w, h, 0.3, 0.15)
    shares = [set((a - b)[a != b].tolist()) for b, a, _ in m["calls"]]
    if (w, h) == (5, 3):
        assert m["spp"].tolist() == [[20]] and m["out"].tolist() == [[46]]
    else:  # a pass with a clipped tile beside an unclipped one
        assert any(MIXED_STEP in s and min(s) < MIXED_STEP for s in shares), shares
    with _ctx(scene("cornell", w, h)) as ctx:
        check_mixed(ctx, m, (w, h))


@pytest.mark.parametrize("env", [{"MFX_POOL": "4096", "MFX_ADAPTIVE_CHECK": "1"}, {"MFX_QUEUE_FROM": "-1"},
                                 {"MFX_QUEUE_FROM": "2"}], ids=["pool4096", "in_place", "queue_from_2"])
def test_mixed_counts_modes(gpu, oracle, env):
    """MFX_POOL=4096: a mixed-count pass spans generations (the first has 30 tiles x 8 samples x 64
    paths), with the host's list validation on; the in-place and the late-queue iterations."""
    m = mixed_reference(oracle, "cornell", W, H, 0.25, 0.1)
    with _ctx(scene("cornell", W, H), env) as ctx:
        check_mixed(ctx, m, env)


# ---- idempotence, no-ops, budgets, pass limits -----------------------------------------------------

def test_idempotence_and_no_ops(gpu, oracle):
    m = mixed_reference(oracle, "cornell", W, H, 0.25, 0.1)
    a = scene("cornell", W, H)
    want_next = oracle.OracleScene(a).sample(1, SEED, sample_base=MIXED_MAX)
    from mafrixraytracing_amd.adaptive import reference_resume
    no_ops = (m["r"],  # the same again
              _rcfg(MIXED_MAX, MIXED_STEP, 0.5),  # a looser threshold
              _rcfg(40, 3, 0.2, abs_floor=1.0),  # and a budget below the reserved one
              _rcfg(2, 1, 0.0, abs_floor=0.0))  # the strictest threshold, no budget
    for r in no_ops:  # the reference runs no pass either, and no check of it is near a tie
        out, active, gap, _, _ = reference_resume(m["Y"], W, H, m["out"], m["S1"], m["S2"], r)
        assert np.array_equal(out, m["out"]) and active == 0 and gap > 1e-6, r
    with _ctx(a) as ctx:
        frame, tiles = check_mixed(ctx, m)
        for r in no_ops:
            f2, t2, rgba2, active = _resume(ctx, r)
            assert active == 0 and np.array_equal(f2, frame) and np.array_equal(t2, tiles), r
            assert np.array_equal(rgba2, m["rgba"])
            assert not ctx.ray_counts()[:4].any() and ctx.stats()[0] == 0, r  # no pass: 0 rays
        assert not ctx.ray_counts_total()[:4].any()
        assert np.array_equal(ctx.sample(1), want_next)  # next_sample did not move


def test_budget_raised_twice(gpu, oracle):
    """32 -> 48 -> 64 under one threshold and step: the counts, pixels and RGBA8 of one call with
    max_spp 64, and the sample counter after it."""
    cfg = _cfg(0.25)
    ref = reference(oracle, "cornell", W, H, _cfg(0.25, max_spp=64))
    assert int(ref[0].max()) > 48 and len(set(ref[0].ravel().tolist())) > 3
    a = scene("cornell", W, H)
    with _ctx(a) as ctx:
        run(ctx, cfg, want_rgba=False)
        _, t48, active = _resume(ctx, _rcfg(48, 4, 0.25), want_rgba=False)
        assert active == 0 and np.array_equal(t48, np.minimum(ref[0], 48))
        frame, tiles, rgba, active = _resume(ctx, _rcfg(64, 4, 0.25))
        assert active == 0 and np.array_equal(tiles, ref[0])
        assert np.array_equal(frame, ref[1]) and np.array_equal(rgba, ref[2])
        assert np.array_equal(ctx.sample(1), oracle.OracleScene(a).sample(1, SEED, sample_base=64))


def test_max_passes_reports_the_active_tiles(gpu, oracle):
    m = mixed_reference(oracle, "cornell", W, H, 0.25, 0.1)
    from dataclasses import replace
    one = replace(m["r"], max_passes=1)
    with _ctx(scene("cornell", W, H)) as ctx:
        run(ctx, m["cfg"], want_rgba=False)
        for before, after, want_active in m["calls"]:
            _, tiles, active = _resume(ctx, one, want_rgba=False)
            assert active == want_active and np.array_equal(tiles, after)
        assert m["calls"][-1][2] == 0 and np.array_equal(tiles, m["out"])
    with _ctx(scene("cornell", W, H)) as ctx:  # two passes per call
        run(ctx, m["cfg"], want_rgba=False)
        _, tiles, active = _resume(ctx, replace(m["r"], max_passes=2), want_rgba=False)
        assert active == m["calls"][1][2] and np.array_equal(tiles, m["calls"][1][1])


def test_denoiser_filters_a_resumed_result(gpu, oracle):
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var, variance_of_mean
    m = mixed_reference(oracle, "cornell", W, H, 0.25, 0.1)
    with _ctx(scene("cornell", W, H)) as ctx:
        feat = ctx.aov(4)
        frame, tiles = check_mixed(ctx, m)
        got, gvar = ctx.denoise_var(None, want_variance=True)
    n = pixel_counts(tiles, W, H)
    var = variance_of_mean(m["S1"], m["S2"], n)
    ref, rvar = reference_denoise_var(frame, var, feat, W, H, DenoiseVarConfig())
    assert np.array_equal(got, ref) and np.array_equal(gvar, rvar)


# ---- refusals and the existing call ---------------------------------------------------------------

def test_refusals(gpu):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL, MfxAdaptiveResume
    a = scene("cornell", 16, 16)

    def call(ctx, **kw):
        d = dict(max_spp=16, step_spp=4, max_passes=0, reserved=0, rel_error=0.05, abs_floor=0.01)
        d.update(kw)
        cfg = MfxAdaptiveResume(**d)
        rc = ctx.lib.mfx_sample_adaptive_resume(ctx._h, C.byref(cfg), None, None, None, None)
        return rc, ctx.lib.mfx_last_error()

    with _ctx(a) as ctx:
        rc, err = call(ctx)
        assert rc == -4 and b"mfx_sample_adaptive_resume" in err  # a fresh context: MFX_E_STATE
        ctx.sample_adaptive(4, 8, 4, 0.1, 0.01)
        for bad in (dict(max_spp=1), dict(step_spp=0), dict(max_passes=-1), dict(reserved=1), dict(rel_error=-0.1),
                    dict(rel_error=float("nan")), dict(abs_floor=-1.0), dict(abs_floor=float("inf"))):
            rc, err = call(ctx, **bad)
            assert rc == -1 and err, bad  # MFX_E_INVALID
        assert ctx.lib.mfx_sample_adaptive_resume(ctx._h, None, None, None, None, None) == -1
        assert ctx.lib.mfx_sample_adaptive_resume(None, None, None, None, None, None) == -1
        assert call(ctx)[0] == 0  # every output pointer may be NULL
        assert call(ctx, max_spp=24)[0] == 0  # and again, with a larger budget
        ctx.sample(1)
        assert call(ctx)[0] == -4  # a trace since
        ctx.sample_adaptive(4, 8, 4, 0.1, 0.01)
        ctx.accum_clear()
        assert call(ctx)[0] == -4
        ctx.sample_adaptive(4, 8, 4, 0.1, 0.01)
        p, n = ctx.accum_device_ptr()
        ctx.accum_attach(p, n)
        assert call(ctx)[0] == -4
        ctx.accum_attach(None)
        ctx.sample_adaptive(4, 8, 4, 0.1, 0.01)
        assert call(ctx)[0] == 0
    with _ctx(a, render_ahead=4) as ctx:  # a render call served by render-ahead draws samples in between
        ctx.sample_adaptive(4, 8, 4, 0.1, 0.01)
        ctx.render_rgba8(1)
        rc, err = call(ctx)
        assert rc == -4 and b"mfx_sample_adaptive_resume" in err
    for kw in (dict(devices=[0, 0]), dict(part_index=0, part_count=2), dict(flags=MFX_F_MEGAKERNEL)):
        with _ctx(a, **kw) as ctx:
            rc, err = call(ctx)
            assert rc == -4 and b"mfx_sample_adaptive_resume" in err, kw  # MFX_E_STATE


def test_sample_adaptive_after_a_resume(gpu, oracle):
    """mfx_sample_adaptive starts afresh on a context that has resumed: it clears the counts and takes a
    new base. After reset-free use its samples are 46 ..., so the reference is the rule on the oracle's
    frames from sample 46 on; on a fresh context it is check_parity's."""
    from mafrixraytracing_amd.adaptive import luminance, reference_mean, reference_tile_spp
    m = mixed_reference(oracle, "cornell", W, H, 0.25, 0.1)
    cfg = m["cfg"]
    frames = oracle_sample_frames(oracle, "cornell", W, H, MIXED_MAX + cfg.max_spp)[MIXED_MAX:]
    spp, gap = reference_tile_spp(luminance(frames), W, H, cfg)
    assert gap > 1e-6
    mean = reference_mean(frames, spp, W, H)
    o = oracle.OracleScene(scene("cornell", W, H))
    st = added_paths_stats(o, np.full_like(spp, MIXED_MAX), spp + MIXED_MAX, W, H, SEED)
    with _ctx(scene("cornell", W, H)) as ctx:
        check_mixed(ctx, m)
        frame, tiles, rgba = run(ctx, cfg)
        c = ctx.ray_counts()
        assert np.array_equal(tiles, spp) and np.array_equal(frame, mean)
        assert np.array_equal(rgba, oracle.post_rgba8(mean, W, H))
        assert (c[0], c[1], c[2]) == st
        # and the new result resumes from its own base: nothing to do under its own threshold
        _, t2, active = _resume(ctx, _rcfg(cfg.max_spp, cfg.step_spp, cfg.rel_error), want_rgba=False)
        assert active == 0 and np.array_equal(t2, spp) and not ctx.ray_counts()[:4].any()
    ref = reference(oracle, "cornell", W, H, cfg) + (cfg,)
    with _ctx(scene("cornell", W, H)) as ctx:
        check_parity(ctx, ref)
