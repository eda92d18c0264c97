"""mfx_sample_adaptive on the GPU against the CPU oracle, bit for bit (every comparison is
array_equal): the tile counts are those of the rule stated on the host
(mafrixraytracing_amd/adaptive.py) applied to the oracle's one-sample frames, every pixel is the
oracle's samples 0 .. n - 1 summed in order and divided by its tile's n, the RGBA8 frame is the
oracle's post of that image, and the ray counters are the oracle's over exactly the (pixel, sample)
set {s < tile_spp of the pixel's tile}.

A decision whose two sides lie within ~1e-9 of each other (relative) could fall either way with the
wave's summation order of E and M, so each test first asserts that the reference's smallest gap is
above 1e-6: no tile of these scenes is near a tie, and every tile is compared."""
import ctypes as C
import os

import numpy as np
import pytest

from adaptive_helpers import check_parity, reference, run
from conftest import SEED, scene

pytestmark = pytest.mark.gpu

W, H = 44, 36  # both sides leave edge tiles
BASE = dict(min_spp=4, step_spp=4, max_spp=32, abs_floor=0.01)
QUEUE_MODES = ["-1", "0", "1", "2", "-2"]  # tests/test_gpu_ray_queue.py's MODES and QCHUNKS
QCHUNKS = [{}, {"MFX_QCHUNK": "64", "MFX_CHUNK": "1024"}]


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


@pytest.mark.parametrize("name,rel", [("cornell", 0.25), ("spot", 0.3), ("two_spheres_plane", 0.3),
                                      ("spot16_instanced@2l", 0.3), ("spot16_instanced", 0.3)])
def test_parity(gpu, oracle, name, rel):
    cfg = _cfg(rel)
    ref = reference(oracle, name, W, H, cfg) + (cfg,)
    assert len(set(ref[0].ravel().tolist())) > 1  # the case exercises several passes and stops
    a = scene(name, W, H)
    with _ctx(a) as ctx:
        if name.endswith("@2l"):
            assert ctx.instancing_info()["instances"] > 0  # traced two-level: k_extend starts the paths
        _, _, _, c = check_parity(ctx, ref, name)
        rays, sec = ctx.stats()
        assert rays == c[0] + c[1] + c[2] and sec > 0 and ctx.last_trace_ms() > 0
        tot = ctx.ray_counts_total()
        assert tuple(tot[:3]) == tuple(c[:3])  # the totals: the sum over the call's passes


def test_clipped_step(gpu, oracle):
    """min 4, step 8, max 30: the last step is 2 samples (4, 12, 20, 28, 30)."""
    cfg = _cfg(0.25, step_spp=8, max_spp=30)
    ref = reference(oracle, "cornell", W, H, cfg) + (cfg,)
    assert ref[0].tolist() == [[30, 30, 30, 30, 30, 30], [12, 20, 28, 20, 12, 20], [20, 20, 20, 12, 12, 12],
                               [28, 20, 20, 30, 20, 12], [30, 20, 28, 30, 30, 30]]
    with _ctx(scene("cornell", W, H)) as ctx:
        check_parity(ctx, ref)


def test_degenerate_schedule_is_sample(gpu):
    """min = max = 8: one pass of 8 samples over every tile, the frame and rays of mfx_sample(8)."""
    a = scene("cornell", W, H)
    with _ctx(a) as ctx:
        want = ctx.sample(8)
        cw = ctx.ray_counts()
    with _ctx(a) as ctx:
        frame, tiles = ctx.sample_adaptive(8, 8, 4, 0.25, 0.01)
        c = ctx.ray_counts()
    assert np.array_equal(frame, want)
    assert np.array_equal(tiles, np.full((5, 6), 8, dtype=np.int32))
    assert tuple(c[:4]) == tuple(cw[:4])


@pytest.mark.parametrize("w,h,counts", [(5, 3, [[12]]), (9, 8, None)])
def test_small_films(gpu, oracle, w, h, counts):
    """5x3: one tile of m = 15 pixels. 9x8: a second tile one pixel wide (m = 8)."""
    cfg = _cfg(0.4)
    ref = reference(oracle, "cornell", w, h, cfg) + (cfg,)
    if counts is not None:
        assert ref[0].tolist() == counts
    else:
        assert ref[0].shape == (1, 2) and sorted(ref[0].ravel().tolist()) == [12, 16]
    with _ctx(scene("cornell", w, h)) as ctx:
        check_parity(ctx, ref)


def test_generations(gpu, oracle):
    """MFX_POOL=4096: several generations per pass (30 tiles x 4 samples x 64 > 4096), the host's
    list validation on (MFX_ADAPTIVE_CHECK=1)."""
    cfg = _cfg(0.25)
    ref = reference(oracle, "cornell", W, H, cfg) + (cfg,)
    with _ctx(scene("cornell", W, H), {"MFX_POOL": "4096", "MFX_ADAPTIVE_CHECK": "1"}) as ctx:
        check_parity(ctx, ref, "pool 4096")
        assert ctx.trace_timing()["total_ms"] > 0


@pytest.mark.parametrize("mode", QUEUE_MODES)
def test_queue_modes(gpu, oracle, mode):
    cfg = _cfg(0.25)
    ref = reference(oracle, "cornell", W, H, cfg) + (cfg,)
    for env in QCHUNKS:
        with _ctx(scene("cornell", W, H), dict(env, MFX_QUEUE_FROM=mode)) as ctx:
            check_parity(ctx, ref, (mode, env))


def test_sequence_and_state(gpu, oracle):
    """The call advances the sample counter by max_spp whatever the tiles did, and leaves the film alone."""
    cfg = _cfg(0.25)
    ref = reference(oracle, "cornell", W, H, cfg) + (cfg,)
    a = scene("cornell", W, H)
    with _ctx(a) as ctx:
        ctx.render_rgba8(1)
        ctx.render_rgba8(1)
        film = ctx.film_mean()
    with _ctx(a) as ctx:
        check_parity(ctx, ref)
        assert np.array_equal(ctx.sample(1), oracle.OracleScene(a).sample(1, SEED, sample_base=32))
    with _ctx(a) as ctx:  # the film of two render calls survives an adaptive call (which draws samples 2 .. 33)
        ctx.render_rgba8(1)
        ctx.render_rgba8(1)
        run(ctx, cfg, want_rgba=False)
        assert np.array_equal(ctx.film_mean(), film)


def test_refusals(gpu):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL, MfxAdaptive
    a = scene("cornell", 16, 16)

    def call(ctx, **kw):
        d = dict(min_spp=4, max_spp=8, step_spp=4, reserved=0, rel_error=0.1, abs_floor=0.01)
        d.update(kw)
        cfg = MfxAdaptive(**d)
        rc = ctx.lib.mfx_sample_adaptive(ctx._h, C.byref(cfg), None, None, None)
        return rc, ctx.lib.mfx_last_error()

    with _ctx(a) as ctx:
        for bad in (dict(min_spp=1), dict(max_spp=3), dict(step_spp=0), dict(rel_error=-0.1),
                    dict(rel_error=float("nan")), dict(reserved=1), dict(abs_floor=float("inf"))):
            rc, err = call(ctx, **bad)
            assert rc == -1 and err, bad  # MFX_E_INVALID
        assert ctx.lib.mfx_sample_adaptive(ctx._h, None, None, None, None) == -1
        assert call(ctx)[0] == 0  # every output pointer may be NULL
    for kw in (dict(devices=[0, 0]), dict(part_index=0, part_count=2), dict(flags=MFX_F_MEGAKERNEL)):
        with _ctx(a, **kw) as ctx:
            rc, err = call(ctx)
            assert rc == -4 and b"mfx_sample_adaptive" in err, kw  # MFX_E_STATE
