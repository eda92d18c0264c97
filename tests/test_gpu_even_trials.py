"""The wave-shared hemisphere sampler's even share (hemisphere_ball_wave, mfx_wavefront.hip) and the
trace kernels' per-format instances.

After round 0 the np owners still rejecting share all 64 lanes of a round: b = 64 // np trials each,
one more for the first 64 - b * np ranks. Each owner still takes its lowest accepted trial among
consecutive trial indices, so the accepted trial, the point and the draw count are the per-lane
loop's: frames and ray counts must equal the oracle's and the megakernel's (which samples with the
per-lane loop, hemisphere_ball) bit for bit. The films make shading batches of every fill: one
8x8 window, 128 and 192 paths per sample at 1 to 3 spp, cube_cornell (most camera rays hit) and spot
(a third miss): full batches, partial ones, and a launch's last batch with 1 to 63 owners; path depths
0, 1 and 3, in place and with ray queues.

Which rounds an input reaches is computed on the CPU from the oracle's draw counts
(test_rounds_reached_by_the_first_batch): the first-vertex batch of an 8x8 film is one window of one
wave, its owners the pixels whose camera ray hits, in slot order, so its rounds are known. With the
suite's seed neither 8x8 film ends on one pending owner, so two seeds were added that do
(REACH_SEEDS): cube_cornell under seed 7 runs np = 43 (b = 1: shares of 2 and of 1), 32 (b = 2, no
remainder), 17 (b = 3, e = 13), 8 and np = 1 (one owner on all 64 lanes); spot under seed 12 runs
np = 32, 20, 7, 1. An all-pending round of a full batch (np = 64 after round 0) has probability
(1 - pi / 12)^64 = 3.6e-9 per batch, out of reach of a seed search; np = 64 is b = 1, e = 0, the
arithmetic the lanes >= 2 e run in every reached round with np > 32.
(cube_cornell at these films' 16:9 camera: about 55 of 64 camera rays hit, so its 8x8 batch is not
full; the 16x8 and 24x8 films list more than 64 hits in a launch, whose first batch is full.)"""
import math

import numpy as np
import pytest

from conftest import SEED, scene
from gpu_helpers import assert_frame, assert_megakernel_frame, ctx_env, oracle_frame

FILMS = [(8, 8, 1), (16, 8, 1), (16, 8, 2), (16, 8, 3), (24, 8, 1), (24, 8, 2), (24, 8, 3)]
SCENES = ["cube_cornell", "spot"]
DEPTHS = [0, 1, 3]
# tests/test_gpu_ray_queue.py's modes: in place, and ray queues from the first vertex
QUEUE_MODES = {"in place": "-1", "ray queues": "0"}


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", SCENES)
def test_frames_equal_oracle(gpu, oracle, name, depth):
    for w, h, spp in FILMS:
        ref = oracle_frame(oracle, name, w, h, depth, spp)
        a = scene(name, w, h, max_depth=depth)
        for what, mode in QUEUE_MODES.items():
            with ctx_env(a, {"MFX_QUEUE_FROM": mode}) as ctx:
                assert_frame(ctx, ctx.sample(spp), ref, (name, depth, w, h, spp, what))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", SCENES)
def test_wavefront_equals_megakernel(gpu, oracle, name, depth):
    """At 1 spp the megakernel's frame is exact too: the per-lane loop and the wave's shared rounds
    give the same frame."""
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    for w, h in sorted({(w, h) for w, h, _ in FILMS}):
        ref = oracle_frame(oracle, name, w, h, depth, 1)
        a = scene(name, w, h, max_depth=depth)
        with ctx_env(a) as ctx:
            wf = ctx.sample(1)
            assert_frame(ctx, wf, ref, (name, depth, w, h, "wavefront"))
        with ctx_env(a, flags=MFX_F_MEGAKERNEL) as ctx:
            mk = ctx.sample(1)
            assert_megakernel_frame(ctx, mk, ref, 1, (name, depth, w, h, "megakernel"))
        assert np.array_equal(wf, mk), (name, depth, w, h)


@pytest.mark.gpu
def test_fp16_and_fp32_instances_on_spot(gpu, oracle):
    """One context on FP16 nodes and one under MFX_NODE_F32 (as tests/test_gpu_fp16_nodes.py starts
    them): each runs the trace kernels' instances built for its format alone. Equal frames and ray
    counts, the oracle's; and the FP32 walk's traversal counters (the counting instances) equal the
    megakernel's, which walks the same FP32 nodes."""
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL
    w, h, spp = 64, 36, 4
    ref = oracle_frame(oracle, "spot", w, h, 3, spp)
    a = scene("spot", w, h)
    for what, mode in QUEUE_MODES.items():
        frames = {}
        for fmt, env in (("fp16", {}), ("fp32", {"MFX_NODE_F32": "1"})):
            with ctx_env(a, dict(env, MFX_QUEUE_FROM=mode)) as ctx:
                frames[fmt] = ctx.sample(spp)
                assert_frame(ctx, frames[fmt], ref, (what, fmt))
        assert np.array_equal(frames["fp16"], frames["fp32"]), what
    # per-lane camera rays, so the counters are per-ray walks in both pipelines
    with ctx_env(a, {"MFX_NODE_F32": "1", "MFX_CAMERA_PACKETS": "0"}, flags=MFX_F_COUNT_STATS) as ctx:
        ctx.sample(2)
        cw = ctx.ray_counts()
    with ctx_env(a, flags=MFX_F_COUNT_STATS | MFX_F_MEGAKERNEL) as ctx:
        ctx.sample(2)
        cm = ctx.ray_counts()
    assert np.array_equal(cw[:10], cm[:10]), (cw[:10], cm[:10])


def _first_vertex_trials(oracle, a, seed=SEED):
    """Trials of the rejection sampler at the first vertex of every path of sample 0 whose camera ray
    hits, in slot order of an 8x8 tile (slot = x + 8 y), from the oracle: the camera ray from draws 0
    and 1, its hit's normal, and the sampler's draw count after them (3 per trial)."""
    w, h, cam = a.width, a.height, a.camera
    assert (w, h) == (8, 8)
    o = oracle.OracleScene(a)
    rays = np.zeros((64, 6))
    pix = np.zeros(64, dtype=np.int64)
    for slot in range(64):
        x, y = slot & 7, slot >> 3
        pix[slot] = x * h + y
        d = oracle.rng_draws(seed, int(pix[slot]), 0, 2)
        ro, rd = oracle.kat_camera_ray(cam["position"], cam["direction"], cam["fov"], cam["aspect"], (x + d[0]) / w,
                                       (y + d[1]) / h)
        rays[slot, :3], rays[slot, 3:] = ro, rd
    _, prim, nrm = o.closest_hit(rays)
    trials = []
    for slot in range(64):
        if prim[slot] >= 0:
            _, n = oracle.kat_hemisphere(nrm[slot], seed, int(pix[slot]), 0, skip=2)
            assert (n - 2) % 3 == 0
            trials.append((n - 2) // 3)
    return trials


def _rounds(trials):
    """The even share's rounds for a batch whose owners accept their trials[i]-th trial: the list of
    (np, b, e) per shared round, and every owner's last trial index as the wave finds it."""
    need = np.asarray(trials)
    done_at = np.where(need == 1, 1, 0)  # round 0: every owner's own first trial
    nxt = np.ones(len(need), dtype=int)
    out = []
    while (done_at == 0).any():
        pend = np.flatnonzero(done_at == 0)
        n = len(pend)
        b, e = 64 // n, 64 - (64 // n) * n
        out.append((n, b, e))
        first = 0
        for r, i in enumerate(pend):
            m = b + (1 if r < e else 0)
            assert first == r * b + min(r, e)
            if nxt[i] < need[i] <= nxt[i] + m:
                done_at[i] = need[i]
            nxt[i] += m
            first += m
        assert first == 64  # every lane has a trial
    assert np.array_equal(done_at, need)
    return out


# seeds under which the 8x8 film's first-vertex batch ends with one pending owner (np = 1)
REACH_SEEDS = {"cube_cornell": 7, "spot": 12}


def test_rounds_reached_by_the_first_batch(oracle):
    """The rounds of the 8x8 films' first-vertex batches under REACH_SEEDS, from the oracle's draw
    counts (no GPU)."""
    rounds = {n: _rounds(_first_vertex_trials(oracle, scene(n, 8, 8), s)) for n, s in REACH_SEEDS.items()}
    print("first-vertex batches' rounds (np, b, e):", rounds)
    for r in rounds.values():
        assert r[-1] == (1, 64, 0)  # one owner on all 64 lanes
    cc = rounds["cube_cornell"]
    assert any(b == 1 and e > 0 for _, b, e in cc)  # np > 32: shares of 2 and of 1
    assert any(b >= 2 and e > 0 for _, b, e in cc) and any(b >= 2 and e == 0 for _, b, e in cc)
    assert math.isclose((1 - math.pi / 12) ** 64, 3.6e-9, rel_tol=0.02)  # the module's text


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_frames_at_the_seeds_that_end_on_one_owner(gpu, oracle, name):
    seed = REACH_SEEDS[name]
    ref = oracle_frame(oracle, name, 8, 8, 3, 1, seed=seed)
    a = scene(name, 8, 8)
    for what, mode in QUEUE_MODES.items():
        with ctx_env(a, {"MFX_QUEUE_FROM": mode}, seed=seed) as ctx:
            assert_frame(ctx, ctx.sample(1), ref, (name, seed, what))
