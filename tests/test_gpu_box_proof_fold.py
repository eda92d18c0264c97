"""The leaf test's box proof with its per-ray conditions folded (mfx_trace_common.h, tri_box_pass<true>:
one integer compare for the six range checks, min / max for the two selects on the direction's sign, so
the slot loop carries no lane masks) decides exactly as the plain statement, tri_box_pass<false>.

mfx_aabb_selftest evaluates both on every record and adds 2 to the proof's answer where they differ. The
families are the ones tests/test_gpu_aabb_screen.py holds the proof to, plus the places where the fold
could part from the plain form: direction components at, one float below and one float above 2^-60 and
2^60, zero, negative zero, subnormal, infinite and NaN components, triangles scaled until their extent
R = |v0 - o| + |e1| + |e2| crosses the same two bounds, and a triangle collapsed onto the ray's origin
(R = 0).

The rest are frames through the three kernels that run the proof in their slot loops (k_camera, k_extend,
k_shadow), compared with the CPU oracle by array_equal on the image and the ray counts: one 8x8 window and a
padded film, 64-slot chunks, a pool of three generations, the queue modes at max_depth 3 and 5, the
forced stack spill, the LDS-slot instances (cube_cornell), the two-level scene (k_extend traces its camera
rays), the mixed triangle / rect / sphere soup, a row-partitioned context, and the traversal counters of
the wavefront against the megakernel's on FP32 nodes."""
import numpy as np
import pytest

from conftest import scene
from gpu_helpers import assert_frame, ctx_env, oracle_frame
from test_gpu_aabb_screen import cases, triangle_cases

pytestmark = pytest.mark.gpu

SPP = 3
FILMS = [(8, 8), (44, 20)]  # one window; 6 x 3 tiles with padding on both sides
SPILL = {"MFX_STACK_LDS": "2"}  # spot's stack bound is above 2: both per-lane kernels run their SPILL instances


def _boundary_families(rng, n):
    lo60, hi60 = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
    edge = np.array([lo60, np.nextafter(lo60, np.float32(0)), np.nextafter(lo60, np.float32(1)),
                     hi60, np.nextafter(hi60, np.float32(0)), np.nextafter(hi60, np.float32(np.inf)),
                     0.0, 5e-324, 1e-310, 1e-30, 1e30, np.inf, np.nan], dtype=np.float64)
    edge = np.concatenate([edge, -edge])
    # 1. one direction component at an edge value (the others as they were: unit-length rays)
    a = triangle_cases(rng, n)
    a[np.arange(n), 9 + rng.integers(0, 3, n)] = edge[rng.integers(0, len(edge), n)]
    # 2. every direction component at an edge value
    b = triangle_cases(rng, n)
    b[:, 9:12] = edge[rng.integers(0, len(edge), (n, 3))]
    # 3. the triangle, its box and the origin scaled: R crosses 2^-60 and 2^60
    c = triangle_cases(rng, n)
    s = 2.0 ** rng.choice([-64, -61, -60, -59, -56, 56, 59, 60, 61, 64], (n, 1)).astype(np.float64)
    c[:, 0:9] *= s
    c[:, 12:14] *= s  # (the query interval with them: in range, the scaled case is the unscaled one)
    c[:, 14:23] *= s
    # 4. a triangle collapsed onto the origin: R = 0 on every axis
    d = triangle_cases(rng, n // 4)
    d[:, 14:17] = d[:, 6:9]
    d[:, 17:23] = 0.0
    d[:, 0:3] = d[:, 3:6] = d[:, 6:9]
    return [a, b, c, d]


def test_folded_proof_decides_as_the_plain_proof(gpu):
    from mafrixraytracing_amd.native import aabb_selftest
    rng = np.random.default_rng(20261020)
    n = 100_000
    fams = [triangle_cases(rng, n), triangle_cases(rng, n, flat=True), cases(rng, n // 4)] + _boundary_families(rng, n)
    rec = np.concatenate(fams)
    exact, _, proof = aabb_selftest(rec)
    bad = np.flatnonzero(proof >= 2)
    assert bad.size == 0, (bad.size, rec[bad[:3]])
    # both answers are reached, and a proof is never wrong (as test_gpu_aabb_screen.py holds)
    assert (proof[:n] == 1).any() and (proof[:n] == 0).any()
    assert not ((proof == 1) & (exact != 1)).any()
    # a direction component outside [2^-60, 2^60] as a float (or NaN) is never proved, by either form
    with np.errstate(over="ignore"):
        ad = np.abs(rec[:, 9:12].astype(np.float32))
    out = ~((ad >= np.float32(2.0 ** -60)) & (ad <= np.float32(2.0 ** 60))).all(axis=1)
    assert out.sum() > n and (proof[out] == 0).all()
    # scaled triangles whose R stays in range are proved as unscaled ones are; R = 0 never is
    lo = 2 * n + len(fams[2])
    assert (proof[lo + 2 * n:lo + 3 * n] == 1).any()
    assert (proof[lo + 3 * n:] == 0).all()


# ---- frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("chunk", [{"MFX_CHUNK": "64"}, {}], ids=["chunk64", "default"])
def test_spot_forced_spill(gpu, oracle, film, chunk):
    w, h = film
    with ctx_env(scene("spot", w, h), dict(SPILL, **chunk)) as ctx:
        li = ctx.launch_info()
        assert li["spill_ext"] and li["spill_shd"] and li["nslot_ext"] == 0, li
        if chunk:
            assert li["chunk"] == 64, li
        assert_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, "spot", w, h, 3, SPP), (film, chunk))


def test_three_generations(gpu, oracle):
    """MFX_POOL=2048: generations of 4,096 paths; 8 spp of the 18-tile film are 9,216."""
    with ctx_env(scene("spot", 44, 20), {"MFX_POOL": "2048", "MFX_CHUNK": "64"}) as ctx:
        assert_frame(ctx, ctx.sample(8), oracle_frame(oracle, "spot", 44, 20, 3, 8))
        assert ctx.trace_timing()["generations"] >= 3


QUEUES = [{"MFX_QUEUE_FROM": "0"}, {"MFX_QUEUE_FROM": "1"}, {"MFX_QUEUE_FROM": "2"}, {"MFX_RAY_QUEUE": "0"}]


@pytest.mark.parametrize("depth", [3, 5])
@pytest.mark.parametrize("queue", QUEUES, ids=["from0", "from1", "from2", "in_place"])
def test_queue_modes(gpu, oracle, queue, depth):
    with ctx_env(scene("spot", 44, 20, max_depth=depth), queue) as ctx:
        if "MFX_RAY_QUEUE" in queue:
            assert ctx.launch_info()["queue_from"] == -1
        assert_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, "spot", 44, 20, depth, SPP), (queue, depth))


@pytest.mark.parametrize("name", ["cube_cornell", "spot16_instanced@2l"])
@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
def test_scene_kinds(gpu, oracle, name, film):
    w, h = film
    with ctx_env(scene(name, w, h)) as ctx:
        li = ctx.launch_info()
        if name == "cube_cornell":
            assert li["nslot_ext"] > 0 and li["nslot_shd"] > 0, li  # the LDS-slot instances
        else:
            assert li["ninst_lds"] > 0 and not li["camera_packets"], li  # two-level: k_extend starts the paths
        assert_frame(ctx, ctx.sample(SPP), oracle_frame(oracle, name, w, h, 3, SPP), (name, film))


def test_mixed_soup(gpu, oracle):
    from soup_helpers import IMAGE_SOUPS, SPP as SOUP_SPP, image_answer, soup_case
    ref, st = image_answer(oracle, IMAGE_SOUPS[0])
    with ctx_env(soup_case(*IMAGE_SOUPS[0])) as ctx:
        img = ctx.sample(SOUP_SPP)
        assert tuple(ctx.ray_counts()[:3]) == tuple(st[:3])
        assert np.array_equal(img, ref)


def test_row_partitions_sum_to_the_whole_film(gpu, oracle):
    from mafrixraytracing_amd.abi import MFX_F_ROW_PARTITION
    a = scene("spot", 44, 20)
    with ctx_env(a) as ctx:
        ctx.trace_accumulate(SPP, 0)
        whole = ctx.accum_read_mean(1.0)
        cw = ctx.ray_counts()[:3].copy()
    total = np.zeros_like(whole)
    ct = np.zeros(3)
    for p in range(3):
        with ctx_env(a, flags=MFX_F_ROW_PARTITION, part_index=p, part_count=3) as ctx:
            ctx.trace_accumulate(SPP, 0)
            total[:, :3] += ctx.accum_read_mean(1.0)[:, :3]
            ct += ctx.ray_counts()[:3]
    assert np.array_equal(ct, cw)
    assert np.array_equal(total[:, :3], whole[:, :3])
    assert tuple(cw) == oracle_frame(oracle, "spot", 44, 20, 3, SPP)[1]


def test_wavefront_and_megakernel_counters_agree_on_the_soup(gpu):
    """MFX_F_COUNT_STATS on the soup, per-lane camera rays, FP32 nodes: the wavefront's ray counts and visit
    counters (nodes, leaves, primitives of closest and shadow rays) are the megakernel's."""
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL
    from soup_helpers import IMAGE_SOUPS, soup_case
    a = soup_case(*IMAGE_SOUPS[0])
    env = {"MFX_CAMERA_PACKETS": "0", "MFX_NODE_F32": "1"}
    with ctx_env(a, env, flags=MFX_F_COUNT_STATS) as w:
        w.sample(2)
        cw = w.ray_counts()
    with ctx_env(a, env, flags=MFX_F_COUNT_STATS | MFX_F_MEGAKERNEL) as m:
        m.sample(2)
        cm = m.ray_counts()
    assert (cw[4:10] > 0).all(), cw
    assert np.array_equal(cw[:4], cm[:4]), (cw[:4], cm[:4])
    assert np.array_equal(cw[4:10], cm[4:10]), (cw[4:10], cm[4:10])
