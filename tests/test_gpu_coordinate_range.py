"""Every walk on scenes whose coordinates lie past or below what binary16 holds (tests/range_helpers.py):
the per-lane kernels' FP16 nodes (mfx_half.h) then have planes at +-inf on the outward and +-65504 on the
inward side beside finite planes of the same node (node_step_h's fmaf(+-inf, 1/d, -o/d); f_tlim's clamp
keeps such a box from being entered wrongly), or subnormal planes whose outward rounding is many times
the FP32 box. Images and ray counts equal the oracle's bit for bit under the per-lane walk on FP16 and
FP32 nodes, the camera packets, the ray queues on and off and the megakernel; the FP16 walk visits no
fewer nodes than the FP32 one; a two-level scene has its top level far out and its templates at local
scale; the GPU builder's images equal the host's. tests/test_coordinate_range_reference.py asserts on
the oracle alone that the cases are lit and leave the half range; the queries' share is
soup_helpers.FAR."""
import numpy as np
import pytest

from conftest import SEED
from range_helpers import CASES, SPP, case_id, moved_instanced_scene, range_image, range_scene
from test_gpu_build import same_build
from test_gpu_mixed_parity import _ctx, _image_exact

pytestmark = pytest.mark.gpu

PER_LANE = {"MFX_CAMERA_PACKETS": "0"}  # every camera ray through k_extend's per-lane walk too
VARIANTS = {"default": {}, "per lane": PER_LANE, "per lane f32 nodes": dict(PER_LANE, MFX_NODE_F32="1"),
            "per lane queues auto": dict(PER_LANE, MFX_QUEUE_FROM="-2"),
            "per lane queues off": dict(PER_LANE, MFX_QUEUE_FROM="-1")}


@pytest.mark.parametrize("c", CASES, ids=case_id)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_range_wavefront_image_exact(gpu, oracle, c, variant):
    ref, st = range_image(oracle, c)
    with _ctx(range_scene(c), VARIANTS[variant]) as ctx:
        _image_exact(ctx, ref, st)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_range_megakernel_image_exact(gpu, oracle, c):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    ref, st = range_image(oracle, c, spp=1)
    with _ctx(range_scene(c), flags=MFX_F_MEGAKERNEL) as ctx:
        _image_exact(ctx, ref, st, spp=1)  # one path per pixel: bit for bit


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_range_fp16_walk_is_a_superset_of_the_fp32_walk(gpu, c):
    """The same rays either way (ray_counts()[:4]), and with MFX_F_COUNT_STATS no fewer node visits on the
    FP16 nodes: their boxes contain the FP32 ones (test_gpu_parity's
    test_megakernel_and_wavefront_counters_agree)."""
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS
    a = range_scene(c)
    out = []
    for env in (PER_LANE, dict(PER_LANE, MFX_NODE_F32="1")):
        with _ctx(a, env, flags=MFX_F_COUNT_STATS) as ctx:
            img = ctx.sample(SPP)
            out.append((img, ctx.ray_counts()))
    (i16, c16), (i32, c32) = out
    print(f"{case_id(c)}: visits FP16 {c16[4:10].tolist()}, FP32 {c32[4:10].tolist()}")
    assert np.array_equal(c16[:4], c32[:4]), (c16[:4], c32[:4])
    assert np.array_equal(i16, i32)
    assert np.all(c16[4:10] >= c32[4:10]), (c16[4:10], c32[4:10])


@pytest.mark.parametrize("two_level", [True, False], ids=["two-level", "default"])
def test_range_two_level_image_exact(gpu, oracle, two_level):
    """Loose primitives, instance offsets, light and camera moved by (1e5, 0, -7e4): MFX_F_TWO_LEVEL keeps
    the instances (TLAS planes beyond the half range, template BVHs at local scale), the default flattens."""
    from mafrixraytracing_amd.abi import MFX_F_TWO_LEVEL
    a = moved_instanced_scene()
    ref, st = oracle.OracleScene(a).sample(SPP, SEED, with_stats=True)
    with _ctx(a, flags=MFX_F_TWO_LEVEL if two_level else 0) as ctx:
        assert (ctx.instancing_info()["instances"] == 8) == two_level
        _image_exact(ctx, ref, st)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_range_gpu_bvh_equals_host_bvh(gpu, c):
    same_build(range_scene(c))


@pytest.mark.parametrize("two_level", [True, False], ids=["two-level", "default"])
def test_range_two_level_gpu_bvh_equals_host_bvh(gpu, two_level):
    a = moved_instanced_scene()
    a.two_level = two_level
    same_build(a)
