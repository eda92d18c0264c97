"""On-GPU traversal-BVH build (the reference builds on the host, Bvh.Build,
BvhNode.fs:24-61) against the host build: mfx_build.hip builds the same binned-SAH tree as
mfx_scene_bvh.cpp's SahBuilder, so the device images are byte-identical (equal FNV digests) and every
traversal, counter and image is identical too. The default context builds on the GPU, so every
other GPU parity test also runs on the GPU-built tree."""
import numpy as np
import pytest

from conftest import SEED, scene

pytestmark = pytest.mark.gpu

SCENES = ["two_spheres_plane", "cornell", "spot", "cube_cornell", "renault", "spot16", "spot16_instanced", "spot16_instanced@2l"]


def both(a):
    from mafrixraytracing_amd.abi import MFX_F_HOST_BVH
    from mafrixraytracing_amd.native import NativeContext
    with NativeContext(a, seed=SEED) as g:
        bg = g.build_info()
    with NativeContext(a, seed=SEED, flags=MFX_F_HOST_BVH) as h:
        bh = h.build_info()
    return bg, bh


@pytest.mark.parametrize("name", SCENES)
def test_gpu_bvh_equals_host_bvh(gpu, name):
    a = scene(name, 16, 16)
    bg, bh = both(a)
    assert bg["gpu_bvh"] and not bh["gpu_bvh"]
    # flat (and auto-flattened) scenes: collapse and layout on the GPU too
    assert bg["gpu_images"] == (a.instancing is None or not a.two_level)
    for k in ("nodes2", "nodes4", "slots"):
        assert bg[k] == bh[k], (k, bg[k], bh[k])
    assert bg["digest"] == bh["digest"]


def soup(n, rng, dup_frac=0.2, grid=False):
    """Random triangles with duplicated and axis-aligned ones: coincident centroids, flat boxes and
    equal SAH costs exercise the tie rules and the all-centroids-equal split."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
    base = scene("spot", 32, 18)
    p = np.zeros(n, dtype=PRIM_DTYPE)
    v0 = rng.uniform(-1, 1, size=(n, 3))
    if grid:
        v0 = np.round(v0 * 4) / 4
    p["p"][:, 0] = v0
    p["p"][:, 1] = v0 + rng.uniform(-0.05, 0.05, size=(n, 3))
    p["p"][:, 2] = v0 + rng.uniform(-0.05, 0.05, size=(n, 3))
    nd = int(n * dup_frac)
    p[n - nd:] = p[:nd]  # exact duplicates
    flat = rng.random(n) < 0.1
    p["p"][flat, :, 1] = p["p"][flat, 0:1, 1]  # flat in y (zero box extent)
    p["kind"] = 0
    return SceneArrays(p, base.albedo[:1], base.light, base.camera, 32, 18)


@pytest.mark.parametrize("n,grid", [(1, False), (2, False), (5, True), (777, True), (20000, False), (60000, True)])
def test_gpu_bvh_equals_host_bvh_on_triangle_soup(gpu, n, grid):
    bg, bh = both(soup(n, np.random.default_rng(n), grid=grid))
    assert bg["digest"] == bh["digest"], (bg, bh)


def same_build(a):
    """GPU-built and host-built images of one scene: equal counts and equal digests."""
    bg, bh = both(a)
    assert bg["gpu_bvh"] and not bh["gpu_bvh"]
    for k in ("nodes2", "nodes4", "slots"):
        assert bg[k] == bh[k], (k, bg[k], bh[k])
    assert bg["digest"] == bh["digest"], (bg, bh)
    return bg


# ---- the branches unit-scale soups never take (digests and counts only; nothing is rendered) --------
def coincident(n_tri, n_sph):
    """n_tri copies of one triangle, then n_sph spheres of different radii around one centre: every
    centroid of a kind coincides (the spheres' boxes differ), so a range of more than max_leaf of them has
    no axis to bin on and k_sah_level / SahBuilder::build split it by position (best_axis < 0)."""
    from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
    base = scene("spot", 32, 18)
    p = np.zeros(n_tri + n_sph, dtype=PRIM_DTYPE)
    p["p"][:n_tri, :3] = [(0.1, 0.2, 0.3), (0.6, 0.25, 0.3), (0.2, 0.7, 0.45)]
    p["kind"][n_tri:] = 2
    p["p"][n_tri:, 0] = (-0.3, 0.4, 0.1)
    p["p"][n_tri:, 1, 0] = 0.01 + 0.002 * np.arange(n_sph)
    return SceneArrays(p, base.albedo[:1], base.light, base.camera, 32, 18)


@pytest.mark.parametrize("n_tri,n_sph", [(5, 0), (64, 0), (65, 0), (1000, 0), (0, 300), (65, 300)])
def test_gpu_bvh_equals_host_bvh_when_centroids_coincide(gpu, n_tri, n_sph):
    bg = same_build(coincident(n_tri, n_sph))
    assert bg["nodes2"] >= (n_tri + n_sph) // 4 - 1  # more than max_leaf items: split, not one leaf


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129])
def test_gpu_bvh_equals_host_bvh_at_wave_boundaries(gpu, n):
    """Ranges that end on, one before and one after a multiple of the 64 lanes that share a range."""
    same_build(soup(n, np.random.default_rng(n), grid=True))


@pytest.mark.parametrize("leaf_max", [1, 2, 3])
@pytest.mark.parametrize("c_isect", [0.25, 8])
def test_gpu_bvh_equals_host_bvh_under_other_sah_parameters(gpu, monkeypatch, leaf_max, c_isect):
    """MFX_LEAF_MAX and MFX_SAH_CI (both builders read them at every build) away from their defaults, 4
    and 1.5: the leaf rule's other outcomes, on triangles and on the mixed soup."""
    from soup_helpers import soup_case
    scenes = (soup(777, np.random.default_rng(777), grid=True), soup_case(777, 3))
    default = [same_build(a)["nodes4"] for a in scenes]
    monkeypatch.setenv("MFX_LEAF_MAX", str(leaf_max))
    monkeypatch.setenv("MFX_SAH_CI", str(c_isect))
    other = [same_build(a)["nodes4"] for a in scenes]
    print(f"MFX_LEAF_MAX={leaf_max} MFX_SAH_CI={c_isect}: nodes4 {other}, default {default}")
    # the parameters reached both builders: the host build's BVH4 has 308 and 274 nodes by default and
    # between 160 and 371 under these six pairs, never the default's count
    assert all(o != d for o, d in zip(other, default))


@pytest.mark.parametrize("s", [1e18, 3e19, 1e30])
def test_gpu_bvh_equals_host_bvh_where_sah_areas_overflow(gpu, s):
    """The 777 mixed soup scaled until the SAH areas are finite but their products with the weights
    overflow near the root (1e18: areas to 1e37), partly +inf (3e19) and all +inf (1e30). An inf cost is
    not below the FLT_MAX best_cost starts at, nor below the FLT_MAX of an invalid lane, so both builders
    fall to the positional split; no NaN arises (every box is widened by eps > 0, and an empty bin's
    area is 0). The host build has 274 BVH4 nodes at unit scale, 371 at 1e18 and 109 at 3e19 and 1e30."""
    from range_helpers import similar
    from soup_helpers import soup_case
    a = soup_case(777, 3)
    bg = same_build(similar(a, s, (0.0, 0.0, 0.0)))
    b1 = same_build(a)
    print(f"s={s:g}: nodes4 {bg['nodes4']}, unit scale {b1['nodes4']}")
    assert bg["nodes4"] != b1["nodes4"]  # positional splits somewhere: another tree than at unit scale


def test_gpu_bvh_build_time_reported(gpu):
    bg, bh = both(scene("spot16", 16, 16))
    assert bg["bvh_ms"] > 0 and bh["bvh_ms"] > 0 and bg["levels"] > 1
    print(f"spot16 BVH2: GPU {bg['bvh_ms']:.1f} ms ({bg['levels']} levels), host {bh['bvh_ms']:.1f} ms; "
          f"reference grouping {bh['ref_bvh_ms']:.1f} ms; scene {bg['scene_ms']:.1f} / {bh['scene_ms']:.1f} ms")
