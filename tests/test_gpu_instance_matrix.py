"""Every axis by which a launch chooses its trace-kernel instance (mfx_wavefront.hip: the instance key),
walked on purpose at a tiny film and compared with the CPU oracle bit for bit.

The rest of the suite reaches many instances by accident of its scenes. Here a case is one context whose
creation pins the scene kind (flat, slots in LDS, two-level), the stack (default, or a forced spill), the
k_shadow build (3 or 4 waves), in place or ray queues from the first iteration, STATS, and on the flat
scene the node format; the context then runs the three trace kinds: an adaptive call (a tile list), its
resume (a list with per-tile counts) and a plain Sample. mfx_launch_info must show what was pinned.

No combination of these axes is refused by the API today, so no case asserts a refusal."""
import numpy as np
import pytest

from adaptive_helpers import check_parity, reference
from adaptive_resume_helpers import added_paths_stats, first_result, one_pass_chain
from conftest import SEED, scene
from gpu_helpers import assert_frame, ctx_env, oracle_frame

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 24, 16, 2, 3  # 3 x 2 tiles
SPILL = {"MFX_STACK_LDS": "2"}  # every scene's stack bound is above 2 (8, 26 and 33)
SCENES = {"flat": "spot", "slots in LDS": "cube_cornell", "two-level": "spot16_instanced@2l"}
KINDS = [(k, {}) for k in SCENES] + [("flat", {"MFX_NODE_F32": "1"})]
QUEUES = [{"MFX_RAY_QUEUE": "0"}, {"MFX_QUEUE_FROM": "0"}]

_resumed = {}


def _cfgs():
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, ResumeConfig
    return AdaptiveConfig(2, 8, 2, 0.6, 0.01), ResumeConfig(12, 4, 0.3, 0.01, 0)


def _resume_reference(oracle, name):
    """What the resume must return after the adaptive call, and the oracle's rays over the samples it
    added (tests/test_gpu_adaptive_resume.py's mixed_reference, for this file's film). Once per scene."""
    from mafrixraytracing_amd.adaptive import reference_mean
    world = name.replace("@2l", "")
    if world not in _resumed:
        cfg, r = _cfgs()
        frames, Y, spp, S1, S2, gap = first_result(oracle, name, W, H, cfg)
        _, (out, _, _), rgap = one_pass_chain(Y, W, H, spp, S1, S2, r)
        assert min(gap, rgap) > 1e-6, (name, gap, rgap)  # the condition on the inputs: no tile near a tie
        assert (out > spp).any(), (spp.tolist(), out.tolist())  # the resume runs a pass
        mean = reference_mean(frames[:r.max_spp], out, W, H)
        st = added_paths_stats(oracle.OracleScene(scene(world, W, H)), spp, out, W, H, SEED)
        for a in (out, mean):
            a.setflags(write=False)
        _resumed[world] = (out, mean, st)
    return _resumed[world]


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("queue", QUEUES, ids=["in place", "queues"])
@pytest.mark.parametrize("waves", [3, 4])
@pytest.mark.parametrize("spill", [False, True], ids=["default stack", "forced spill"])
@pytest.mark.parametrize("kind,fmt", KINDS, ids=[k + (" f32" if f else "") for k, f in KINDS])
def test_instance(gpu, oracle, kind, fmt, spill, waves, queue, stats):
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS
    name = SCENES[kind]
    cfg, r = _cfgs()
    env = dict(fmt, **queue, MFX_SHADOW_WAVES=str(waves), **(SPILL if spill else {}))
    with ctx_env(scene(name, W, H, max_depth=DEPTH), env, flags=MFX_F_COUNT_STATS if stats else 0) as ctx:
        li = ctx.launch_info()
        assert li["shadow_waves"] == waves and li["queue_from"] == (-1 if "MFX_RAY_QUEUE" in queue else 0), li
        assert (li["ninst_lds"] > 0) == (kind == "two-level"), li
        assert (li["nslot_ext"] > 0) == (li["nslot_shd"] > 0) == (kind == "slots in LDS"), li
        if spill:  # (tests/test_gpu_stack_shapes.py)
            assert li["stack_lds_ext"] == li["stack_lds_shd"] == 2 and li["spill_ext"] and li["spill_shd"], li
        # a tile list
        check_parity(ctx, reference(oracle, name, W, H, cfg, depth=DEPTH) + (cfg,), env)
        assert (ctx.ray_counts()[4:10] > 0).any() == stats
        # a list with per-tile counts
        out, mean, st = _resume_reference(oracle, name)
        frame, tiles, active = ctx.sample_adaptive_resume(r.max_spp, r.step_spp, r.rel_error, r.abs_floor)
        c = ctx.ray_counts()
        assert active == 0 and np.array_equal(tiles, out), (env, tiles.tolist(), out.tolist())
        assert np.array_equal(frame, mean), (env, np.abs(frame - mean).max())
        assert (c[0], c[1], c[2]) == st and c[3] == c[0], (env, c[:4], st)
        assert (c[4:10] > 0).any() == stats
        # a plain trace: the samples after the budget the two calls reserved
        assert_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, name, W, H, DEPTH, SPP, base=r.max_spp), env)
        assert (ctx.ray_counts()[4:10] > 0).any() == stats
