"""The path key's inputs at values no other GPU test uses (they all run SEED, 31 significant bits, and
sample indices of a few dozen): seeds with bits in their upper half and global sample indices around
2^31 and 2^32. The key takes all 64 bits of the seed and the global sample index
modulo 2^32, and it is formed in five places: k_camera, per-lane fresh rays in k_extend, k_shadow
(again at every vertex), the megakernel and k_aov. Every result is compared with the CPU oracle at
the same seed and sample base, bit for bit, so a site that dropped the seed's upper half would show
SEED's image (another one: tests/test_path_depth_reference.py), and one that narrowed the sample
index to 32 bits with a sign, or kept more than 32, would show other samples."""
import numpy as np
import pytest

from adaptive_helpers import check_parity, reference
from conftest import SEED, scene
from denoise_helpers import oracle_features
from gpu_helpers import assert_frame, assert_megakernel_frame, assert_render_ahead, ctx_env, oracle_frame

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 24, 3
SEEDS = [0, SEED | 1 << 32, SEED | 1 << 63, 2 ** 64 - 1]
ids = [f"{s:#x}" for s in SEEDS]
# (first global sample, samples): across 2^31, across the wrap at 2^32, past it
BASES = [(2 ** 31 - 2, 4), (2 ** 32 - 2, 4), (2 ** 32 + 5, 2)]


# ---- the seed, one test per key site ----
@pytest.mark.parametrize("seed", SEEDS, ids=ids)
def test_seed_in_k_camera_and_k_shadow(gpu, oracle, seed):
    """A flat scene's wavefront: camera rays as packets (k_camera), every later draw in k_shadow."""
    with ctx_env(scene("cornell", W, H), seed=seed) as ctx:
        assert ctx.launch_info()["camera_packets"]
        for k in range(2):
            assert_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, "cornell", W, H, 3, SPP, k * SPP, seed), (hex(seed), k))


@pytest.mark.parametrize("seed", SEEDS, ids=ids)
def test_seed_in_k_extend_fresh_rays(gpu, oracle, seed):
    """A two-level scene's camera rays start per lane in k_extend (no packets for instanced scenes)."""
    name = "spot16_instanced@2l"
    with ctx_env(scene(name, W, H), seed=seed) as ctx:
        assert ctx.instancing_info()["instances"] > 0
        assert_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, name, W, H, 3, SPP, 0, seed), hex(seed))


@pytest.mark.parametrize("seed", SEEDS, ids=ids)
def test_seed_in_the_megakernel(gpu, oracle, seed):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    with ctx_env(scene("cornell", W, H), seed=seed, flags=MFX_F_MEGAKERNEL) as ctx:
        assert_megakernel_frame(ctx, ctx.sample(1), oracle_frame(oracle, "cornell", W, H, 3, 1, 0, seed), 1, hex(seed))
        assert_megakernel_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, "cornell", W, H, 3, SPP, 1, seed), SPP, hex(seed))


@pytest.mark.parametrize("seed", SEEDS, ids=ids)
def test_seed_in_aov(gpu, oracle, seed):
    with ctx_env(scene("cornell", W, H), seed=seed) as ctx:
        assert np.array_equal(ctx.aov(2), oracle_features(oracle, "cornell", W, H, 2, 0, seed=seed))


@pytest.mark.parametrize("seed", SEEDS, ids=ids)
def test_seed_in_sample_adaptive(gpu, oracle, seed):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig
    cfg = AdaptiveConfig(4, 16, 4, 0.25, 0.01)
    ref = reference(oracle, "cornell", 44, 36, cfg, seed=seed) + (cfg,)
    assert len(set(ref[0].ravel().tolist())) > 1
    with ctx_env(scene("cornell", 44, 36), seed=seed) as ctx:
        check_parity(ctx, ref, hex(seed))


@pytest.mark.parametrize("seed", SEEDS, ids=ids)
def test_seed_in_render_ahead(gpu, oracle, seed):
    with ctx_env(scene("cornell", W, H), seed=seed, render_ahead=3) as ctx:
        assert_render_ahead(oracle, ctx, "cornell", W, H, 3, 4, seed=seed)


# ---- the sample index ----
def _accumulate(ctx, spp, base):
    ctx.accum_clear()
    ctx.trace_accumulate(spp, base)
    return ctx.accum_read_mean(float(spp))


@pytest.mark.parametrize("name", ["cornell", "spot16_instanced@2l"])  # k_camera + k_shadow; k_extend's fresh rays
@pytest.mark.parametrize("base,spp", BASES)
def test_sample_index_in_the_wavefront(gpu, oracle, name, base, spp):
    with ctx_env(scene(name, W, H)) as ctx:
        assert_frame(ctx, _accumulate(ctx, spp, base), oracle_frame(oracle, name, W, H, 3, spp, base), (name, base))
        if base == 2 ** 32 - 2:  # the call's last two samples are samples 0 and 1
            assert_frame(ctx, _accumulate(ctx, 2, base + 2), oracle_frame(oracle, name, W, H, 3, 2, 0), (name, "wrap"))


@pytest.mark.parametrize("base,spp", BASES)
def test_sample_index_in_aov(gpu, oracle, base, spp):
    with ctx_env(scene("cornell", W, H)) as ctx:
        assert np.array_equal(ctx.aov(spp, sample_base=base), oracle_features(oracle, "cornell", W, H, spp, base))
        if base == 2 ** 32 - 2:
            assert np.array_equal(ctx.aov(2, sample_base=base + 2), oracle_features(oracle, "cornell", W, H, 2, 0))


@pytest.mark.parametrize("base,spp", BASES)
def test_sample_index_in_the_megakernel(gpu, oracle, base, spp):
    """One sample per call at the base, at its last sample and one past it."""
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    with ctx_env(scene("cornell", W, H), flags=MFX_F_MEGAKERNEL) as ctx:
        for b in (base, base + spp - 1, base + spp):
            assert_megakernel_frame(ctx, _accumulate(ctx, 1, b), oracle_frame(oracle, "cornell", W, H, 3, 1, b), 1, b)
            assert ctx.trace_timing()["launches"] == 1


def test_sample_index_in_partitioned_contexts(gpu, oracle):
    """part_count = 3 from sample 2^32 - 4: context g renders global samples base + g + 3 s, on both
    sides of the wrap; the accumulators sum to the unpartitioned frame within
    test_partitioned_contexts_sum_to_whole's bound, and each is the oracle's sum of its own samples."""
    base, spp, G = 2 ** 32 - 4, 8, 3
    a = scene("cornell", W, H)
    total = np.zeros((W * H, 4))
    for g in range(G):
        with ctx_env(a, part_index=g, part_count=G) as ctx:
            ctx.accum_clear()
            ctx.trace_accumulate(spp, base)
            part = ctx.accum_read_mean(1.0)
        own = np.zeros((W * H, 3))
        for s in range(base + g, base + spp, G):  # in sample order, as k_resolve adds them
            own = own + oracle_frame(oracle, "cornell", W, H, 3, 1, s)[0][:, :3]
        assert np.array_equal(part[:, :3], own), g
        total += part
    ref = oracle_frame(oracle, "cornell", W, H, 3, spp, base)[0]
    assert np.abs(total[:, :3] / spp - ref[:, :3]).max() < 1e-12
