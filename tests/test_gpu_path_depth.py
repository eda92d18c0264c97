"""Path depths the other GPU tests never run (they use max_depth 1..5), against the CPU oracle on the
same inputs, bit for bit (tests/test_path_depth_reference.py shows that these inputs tell the depths apart):
  0       a generation is one iteration, no next queue is bound, every path is fresh when shaded
  6, 7    the first iterations past k_extend's per-iteration counters (WF_ITER_CTRS): their extension
          rays land in counter [1], and note_live's scan of the live share ends before them
  15      the limit: a 16-bit lit mask in the depth word and the finished state word, k_resolve's
          rolled loop over vertices 4..15, fifteen queue hand-overs, 16 rows of megakernel records
through the wavefront (two calls: the second with the automatic queue start settled), every queue
start, the megakernel, render-ahead, mfx_sample_adaptive, a device list, the banded readback and
mfx_aov; -1 and 16 are refused."""
import numpy as np
import pytest

from adaptive_helpers import check_parity, reference
from conftest import SEED, scene
from denoise_helpers import oracle_features
from gpu_helpers import (QCHUNKS, assert_frame, assert_megakernel_frame, assert_render_ahead, ctx_env,
                         oracle_frame)

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 24, 3
WE, HE = 44, 36  # both sides leave edge tiles
DEPTH_CASES = [(n, d) for n in ("cornell", "cube_cornell") for d in (0, 6, 7, 15)] + [("spot16_instanced@2l", 15)]


def _two_level(ctx, name):
    if name.endswith("@2l"):
        assert ctx.instancing_info()["instances"] > 0  # traced two-level: k_extend starts the paths


@pytest.mark.parametrize("name,depth", DEPTH_CASES)
def test_wavefront_two_calls(gpu, oracle, name, depth):
    """Sample(3) twice: samples 0..2, then 3..5 with queue_auto settled from the first call's counters."""
    a = scene(name, W, H, max_depth=depth)
    with ctx_env(a) as ctx:
        _two_level(ctx, name)
        for k in range(2):
            img = ctx.sample(SPP)
            assert not ctx.launch_info()["lit_in_hit"] or depth <= 3
            assert_frame(ctx, img, oracle_frame(oracle, name, W, H, depth, SPP, k * SPP), (name, depth, k))
            assert ctx.trace_timing()["iterations"] == depth + 1


def _queue_starts(depth):
    return sorted({-2, -1, 0, 1, depth - 1, depth, depth + 3})  # depth 0: -2, -1, 0, 1, 3


@pytest.mark.parametrize("name,depth", [(n, d) for n in ("cornell", "cube_cornell") for d in (0, 6, 15)]
                         + [("spot16_instanced@2l", 15)])
def test_queue_starts(gpu, oracle, name, depth):
    """MFX_QUEUE_FROM -2, -1, 0, 1, max_depth - 1, max_depth and max_depth + 3 (a start at or past
    max_depth allocates the queues and never binds one), default and small chunks, two calls each."""
    a = scene(name, WE, HE, max_depth=depth)
    refs = [oracle_frame(oracle, name, WE, HE, depth, 2, 2 * k) for k in range(2)]
    starts = _queue_starts(depth)
    assert {-2, -1, 0, depth, depth + 3} <= set(starts) and min(starts) == -2
    for q in starts:
        for env in QCHUNKS:
            with ctx_env(a, dict(env, MFX_QUEUE_FROM=str(q))) as ctx:
                _two_level(ctx, name)
                assert ctx.launch_info()["queue_from"] == q  # the setting was read, unclamped above
                for k, ref in enumerate(refs):
                    assert_frame(ctx, ctx.sample(2), ref, (name, depth, q, env, k))


@pytest.mark.parametrize("name,depth", [(n, d) for n in ("cornell", "cube_cornell") for d in (0, 6, 15)]
                         + [("spot16_instanced@2l", 15)])
def test_megakernel(gpu, oracle, name, depth):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    a = scene(name, W, H, max_depth=depth)
    with ctx_env(a, flags=MFX_F_MEGAKERNEL) as ctx:
        _two_level(ctx, name)
        assert_megakernel_frame(ctx, ctx.sample(1), oracle_frame(oracle, name, W, H, depth, 1, 0), 1, (name, depth))
        assert ctx.trace_timing()["launches"] == 1  # the megakernel
        assert_megakernel_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, name, W, H, depth, SPP, 1), SPP, (name, depth))
        assert ctx.trace_timing()["launches"] == 1


@pytest.mark.parametrize("name,depth", [(n, d) for n in ("cornell", "cube_cornell") for d in (0, 15)])
def test_render_ahead(gpu, oracle, name, depth):
    """render_ahead = 3, four one-sample calls (a batch boundary inside): k_resolve's frames mode."""
    with ctx_env(scene(name, W, H, max_depth=depth), render_ahead=3) as ctx:
        assert_render_ahead(oracle, ctx, name, W, H, depth, 4)


@pytest.mark.parametrize("depth", [0, 15])
def test_adaptive(gpu, oracle, depth):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig
    cfg = AdaptiveConfig(4, 16, 4, 0.25, 0.01)
    ref = reference(oracle, "cornell", WE, HE, cfg, depth=depth) + (cfg,)
    assert len(set(ref[0].ravel().tolist())) > 1  # several passes, tiles that stop at different counts
    with ctx_env(scene("cornell", WE, HE, max_depth=depth)) as ctx:
        check_parity(ctx, ref, depth)


def test_device_list_at_depth_15(gpu, oracle):
    """devices=[0, 0]: two bands of tile rows (5 rows, the last one partial), merged on the primary."""
    a = scene("cube_cornell", WE, HE, max_depth=15)
    with ctx_env(a, devices=[0, 0]) as ctx:
        for k in range(2):
            assert_frame(ctx, ctx.sample(2), oracle_frame(oracle, "cube_cornell", WE, HE, 15, 2, 2 * k), k)


def test_banded_readback_at_depth_15(gpu, oracle):
    """mfx_sample's banded last resolve (10 tile columns, the last one partial, in 8 bands) and the
    unbanded one (MFX_SAMPLE_BANDS=0): both the oracle's frame."""
    w, h = 76, 20
    a = scene("cornell", w, h, max_depth=15)
    ref = oracle_frame(oracle, "cornell", w, h, 15, 2, 0)
    for env in ({}, {"MFX_SAMPLE_BANDS": "0"}):
        with ctx_env(a, env) as ctx:
            assert_frame(ctx, ctx.sample(2), ref, env)


@pytest.mark.parametrize("depth", [0, 15])
def test_aov_does_not_depend_on_depth(gpu, oracle, depth):
    """The first-hit features of a depth-0 and a depth-15 context are the depth-3 scene's."""
    with ctx_env(scene("cornell", W, H, max_depth=depth)) as ctx:
        assert np.array_equal(ctx.aov(2), oracle_features(oracle, "cornell", W, H, 2, 0))


def test_depth_boundaries(gpu):
    from mafrixraytracing_amd.abi import MfxError
    from mafrixraytracing_amd.native import NativeContext
    for depth, msg in ((-1, "max_depth must be >= 0"), (16, "max_depth must be <= 15")):
        for flags_kw in ({}, {"devices": [0, 0]}):
            with pytest.raises(MfxError, match=msg):
                NativeContext(scene("cornell", 16, 16, max_depth=depth), seed=SEED, **flags_kw)
    with pytest.raises(MfxError, match="max_depth must be <= 15"):  # mfx_create_instanced
        NativeContext(scene("spot16_instanced@2l", 16, 16, max_depth=16), seed=SEED)
    for depth in (0, 15):
        with NativeContext(scene("cornell", 16, 16, max_depth=depth), seed=SEED) as ctx:
            assert ctx.sample(2).shape == (256, 4)
