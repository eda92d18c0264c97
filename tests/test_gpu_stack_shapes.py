"""Every traversal stack and launch shape mfx_create can choose, pinned and compared with the CPU oracle.

mfx_create decides from occupancy queries which stack a context's kernels use (the whole bound in LDS,
or the first entries in LDS and the deeper ones in a global spill column), how many top nodes, slots and
instance records live in LDS, and which k_shadow build runs; each choice is another template instance.
The rest of the suite runs whatever those rules pick for scenes whose bound is at most 44. Here the
choices are forced through the MFX_* variables the library reads at creation, on chain scenes
(tests/deep_helpers.py) whose bounds are 51, 67, 81 and 93, and every test asserts through
mfx_launch_info that the variant it meant to force is the one that ran: a variable the library clamped
or ignored fails the test instead of passing it empty.

A wrong pop in a deep stack, or a spill column two lanes share, gives plausible images: every
comparison is array_equal (the megakernel above 1 spp keeps test_gpu_parity.py's 1e-12 bar).
tests/test_deep_scenes.py asserts on the host alone that the scenes are as deep as they are meant to be
and that their rays and films reach the chain."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED, scene
from deep_helpers import (ADAPTIVE, DEEPEST, H, K_LARGE, M_RAYS, REFUSED, SPP, STACK_MAX, SWEEP, TWO67, W, adaptive_answer,
                          chain_index, chain_instanced, deep_scene, image_answer, oracle_scene, query_answer, query_rays,
                          stack_bound, through_rays, with_film)

pytestmark = pytest.mark.gpu

IDS = ["51", "67", "80"]
SPILL2 = {"MFX_STACK_LDS": "2"}  # the forced spill of the bound-67 scene: 2 entries in LDS, 65 in the column


def _ctx(monkeypatch, a, env=None, **kw):
    """A context created under `env` (the library reads these at creation and at each trace)."""
    from mafrixraytracing_amd.native import NativeContext
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return NativeContext(a, seed=SEED, **kw)


def _clear(monkeypatch, env):
    for k in env:
        monkeypatch.delenv(k, raising=False)


def _image_exact(ctx, ref, st, spp=SPP, what=""):
    img = ctx.sample(spp)
    counts = ctx.ray_counts()
    assert tuple(counts[:3]) == tuple(st[:3]), (what, counts[:3], st[:3])
    assert np.array_equal(img, ref), (what, np.abs(img - ref).max())  # bit for bit


def _queries_exact(ctx, rays, tmax, want, what=""):
    (ot, op, on), occ = want
    gt, gp, gn = ctx.closest_hit(rays)
    assert np.array_equal(gp, op), f"{what}: prim mismatch on {(gp != op).sum()} rays"
    assert np.array_equal(gt, ot), what
    assert np.array_equal(gn, on), what
    got = ctx.any_hit(rays, tmax)
    assert np.array_equal(got, occ), f"{what}: occlusion mismatch on {(got != occ).sum()} rays"


def _spill_fits(li):
    """The spill buffer holds every deep entry of every lane of either kernel's grid."""
    assert li["spill_lanes"] >= 256 * max(li["wf_ext_grid"], li["wf_shd_grid"]), li
    assert li["spill_entries_per_lane"] >= li["stack_size"] - min(li["stack_lds_ext"], li["stack_lds_shd"]), li
    assert li["spill_ext"] == (li["stack_lds_ext"] < li["stack_size"]), li
    assert li["spill_shd"] == (li["stack_lds_shd"] < li["stack_size"]), li
    assert 1 <= li["stack_lds_ext"] <= li["stack_size"] and 1 <= li["stack_lds_shd"] <= li["stack_size"], li


# ---- a. the stack-share sweep -----------------------------------------------------------------------
@pytest.mark.parametrize("key", SWEEP, ids=IDS)
def test_stack_share_sweep(gpu, oracle, monkeypatch, key):
    """MFX_STACK_LDS = 1, 2, 16, bound - 1 and unset: the wavefront image and the ray counts are the
    oracle's, and with MFX_F_COUNT_STATS the traversal counters [4:10] (node, leaf and primitive visits
    of closest and shadow rays) are the same for every share: a different stack changes no visit."""
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS
    a = deep_scene(key)
    ref, st = image_answer(oracle, a, name=key)
    bound = stack_bound(a)
    visits = {}
    for share in ("1", "2", "16", str(bound - 1), None):
        env = {"MFX_STACK_LDS": share} if share else {}
        for flags in (0, MFX_F_COUNT_STATS):
            with _ctx(monkeypatch, a, env, flags=flags) as ctx:
                li = ctx.launch_info()
                assert li["stack_size"] == bound, (li, bound)  # the GPU build's bound is the host build's
                _spill_fits(li)
                if share:
                    assert li["stack_lds_ext"] == li["stack_lds_shd"] == int(share), (share, li)
                    assert li["spill_ext"] and li["spill_shd"], (share, li)
                _image_exact(ctx, ref, st, what=(share, flags))
                if flags:
                    visits[share] = ctx.ray_counts()[4:10].copy()
        _clear(monkeypatch, env)
    first = visits["1"]
    assert (first > 0).all(), first
    for share, v in visits.items():
        assert np.array_equal(v, first), (share, v, first)


# ---- b. the query kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", SWEEP, ids=IDS)
def test_queries_exact(gpu, oracle, monkeypatch, key):
    a = deep_scene(key)
    rays, tmax = query_rays(key)
    want = query_answer(oracle, key)
    prim = want[0][1]
    h = M_RAYS // 2
    assert (prim >= 0).mean() >= 0.05
    assert ((prim[:h] >= 0) & (chain_index(a, prim[:h]) < K_LARGE)).mean() >= 0.20  # the pops matter
    with _ctx(monkeypatch, a) as ctx:
        assert ctx.launch_info()["stack_size"] == stack_bound(a)
        _queries_exact(ctx, rays, tmax, want)


def test_queries_exact_with_spheres_in_the_template(gpu, oracle, monkeypatch):
    """Every fourth chain primitive a sphere, in a two-level template: more than a tenth of the hits are
    spheres (the rays' targets lie within rel of the chain, so the smallest ones are still missed)."""
    a = deep_scene(TWO67, spheres=True)
    rays = through_rays(a, M_RAYS, np.random.default_rng(4300))
    tmax = np.random.default_rng(4301).uniform(0.05, 3.0, size=M_RAYS)
    o = oracle_scene(oracle, a)
    want = (o.closest_hit(rays), o.any_hit(rays, tmax))
    prim = want[0][1]
    k = chain_index(a, prim[prim >= 0])
    assert (a.prims["kind"][prim[prim >= 0]] == 2).mean() > 0.1 and (k < K_LARGE).any()
    with _ctx(monkeypatch, a) as ctx:
        assert ctx.launch_info()["stack_size"] >= 60
        _queries_exact(ctx, rays, tmax, want)
    with _ctx(monkeypatch, a, SPILL2) as ctx:
        _image_exact(ctx, *image_answer(oracle, a, name=(TWO67, "spheres")))


# ---- c. the megakernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SWEEP, ids=IDS)
@pytest.mark.parametrize("waves", [1, 4])
def test_megakernel(gpu, oracle, monkeypatch, key, waves):
    from mafrixraytracing_amd.abi import MFX_F_MEGAKERNEL
    a = deep_scene(key)
    ref1, st1 = image_answer(oracle, a, spp=1, name=key)
    ref, st = image_answer(oracle, a, name=key)
    env = {"MFX_MEGA_WAVES": str(waves)}
    with _ctx(monkeypatch, a, env, flags=MFX_F_MEGAKERNEL) as ctx:
        assert ctx.launch_info()["mega_waves"] == waves
        _image_exact(ctx, ref1, st1, spp=1)  # one path per pixel: bit for bit
    with _ctx(monkeypatch, a, env, flags=MFX_F_MEGAKERNEL) as ctx:
        img = ctx.sample(SPP)
        counts = ctx.ray_counts()
    assert tuple(counts[:3]) == tuple(st[:3]), (counts[:3], st[:3])
    diff = np.abs(img[:, :3] - ref[:, :3])  # FP64 atomics add a pixel's paths in arrival order
    assert diff.max() <= 1e-12 * max(1.0, np.abs(ref).max()), diff.max()
    assert np.all(img[:, 3] == 1.0)


# ---- d. everything else that shares the kernels, under a forced spill ---------------------------------
def _spilled(ctx):
    li = ctx.launch_info()
    assert li["stack_lds_ext"] == li["stack_lds_shd"] == 2 and li["spill_ext"] and li["spill_shd"], li
    assert li["stack_size"] >= 60, li
    _spill_fits(li)
    return li


def test_spill_adaptive(gpu, oracle, monkeypatch):
    """mfx_sample_adaptive's listed launches (the LIST instances of k_extend and k_shadow)."""
    spp, mean, rgba, st, gap = adaptive_answer(oracle, TWO67)
    assert gap > 1e-9, gap
    with _ctx(monkeypatch, deep_scene(TWO67), SPILL2) as ctx:
        _spilled(ctx)
        frame, tiles, out8 = ctx.sample_adaptive(*ADAPTIVE, want_rgba=True)
        c = ctx.ray_counts()
    assert np.array_equal(tiles, spp), (tiles.tolist(), spp.tolist())
    assert np.array_equal(frame, mean), np.abs(frame - mean).max()
    assert np.array_equal(out8, rgba)
    assert (c[0], c[1], c[2]) == (st[0], st[1], st[2]), (c[:3], st)


def test_spill_render_ahead(gpu, oracle, monkeypatch):
    """Render-ahead batches of 4 against one sample per call and the oracle's film and post."""
    from mafrixraytracing_amd.abi import dptr
    a = deep_scene(TWO67)
    o = oracle_scene(oracle, a)
    npix = W * H
    accum, target, fc = np.zeros((npix, 4)), np.zeros((npix, 4)), np.zeros(1)
    with _ctx(monkeypatch, a, SPILL2) as c1, _ctx(monkeypatch, a, SPILL2, render_ahead=4) as c2:
        _spilled(c1), _spilled(c2)
        for k in range(6):
            r1, r2 = c1.render_rgba8(1), c2.render_rgba8(1)
            fr = o.sample(1, SEED, sample_base=k)
            oracle.lib().oracle_film_add(dptr(accum), dptr(target), dptr(fc), dptr(fr), npix)
            ref = oracle.post_rgba8(target, W, H)
            assert np.array_equal(r1, ref), (k, (r1 != ref).sum())
            assert np.array_equal(r2, ref), (k, (r2 != ref).sum())
        m1, m2 = c1.film_mean(), c2.film_mean()
    assert np.array_equal(m1, m2)
    assert np.array_equal(m2[:, :3], target[:, :3])


def test_spill_aov(gpu, oracle, monkeypatch):
    from denoise_helpers import scene_features
    a = deep_scene(TWO67)
    ref = scene_features(oracle, a.flat(), SPP, 3)
    assert (ref[:, 7] > 0).any() and (ref[:, 7] == 0).any()
    with _ctx(monkeypatch, a, SPILL2) as ctx:
        _spilled(ctx)
        got = ctx.aov(SPP, sample_base=3)
        assert np.array_equal(got, ref), np.abs(got - ref).max(axis=0)
        _image_exact(ctx, *image_answer(oracle, a, name=TWO67))


@pytest.mark.parametrize("mode", ["0", "-1"])
def test_spill_queue_modes(gpu, oracle, monkeypatch, mode):
    """The ray-queue instances (queues from the first vertex) and everything in place."""
    a = deep_scene(TWO67)
    with _ctx(monkeypatch, a, dict(SPILL2, MFX_QUEUE_FROM=mode)) as ctx:
        assert _spilled(ctx)["queue_from"] == int(mode)
        _image_exact(ctx, *image_answer(oracle, a, name=TWO67))


def test_spill_generations(gpu, oracle, monkeypatch):
    """MFX_POOL=2048 (generations of 4,096 paths): 8 spp of the 12-tile film run in two."""
    a = deep_scene(TWO67)
    with _ctx(monkeypatch, a, dict(SPILL2, MFX_POOL="2048")) as ctx:
        assert _spilled(ctx)["pool_max"] == 2048
        _image_exact(ctx, *image_answer(oracle, a, spp=8, name=TWO67), spp=8)
        assert ctx.trace_timing()["generations"] > 1


def test_spill_in_flight(gpu, oracle, monkeypatch):
    """MFX_F_IN_FLIGHT: 512-slot chunk fetches, whole ones for k_shadow."""
    from mafrixraytracing_amd.abi import MFX_F_IN_FLIGHT
    a = deep_scene(TWO67)
    with _ctx(monkeypatch, a, SPILL2, flags=MFX_F_IN_FLIGHT) as ctx:
        li = _spilled(ctx)
        assert li["chunk"] == 512 and not li["shd_half"], li
        _image_exact(ctx, *image_answer(oracle, a, name=TWO67))


# ---- e. residency knobs ------------------------------------------------------------------------------
KNOB_SCENES = ["spot", "cube_cornell", "spot16_instanced@2l"]


def _named(name, depth=3):
    return scene(name, W, H, max_depth=depth)


def _named_answer(oracle, name, depth=3):
    return image_answer(oracle, _named(name, depth), name=(name, depth))


@pytest.fixture(scope="module")
def defaults(gpu):
    """launch_info of the three scene kinds with no variable set."""
    from mafrixraytracing_amd.native import NativeContext
    out = {}
    for name in KNOB_SCENES:
        with NativeContext(_named(name), seed=SEED) as ctx:
            out[name] = ctx.launch_info()
    return out


def test_default_shapes(gpu, defaults):
    """What the knob tests start from: spot FLAT, cube_cornell with its slots in LDS, the instanced scene
    with its 16 records in LDS and no camera packets; the lit mask in the HIT word at max_depth 3."""
    s, c, i = (defaults[n] for n in KNOB_SCENES)
    assert s["nslot_ext"] == 0 and s["nslot_shd"] == 0 and s["camera_packets"] and s["wf_cam_grid"] > 0
    assert c["nslot_ext"] > 0 and c["nslot_shd"] > 0
    assert i["ninst_lds"] == 16 and not i["camera_packets"] and i["wf_cam_grid"] == 0 and i["nslot_ext"] == 0
    for li in (s, c, i):
        assert li["lit_in_hit"] and li["gray_light"] and li["shadow_waves"] in (3, 4) and li["mega_waves"] in (1, 4)
        assert li["ntop_ext"] >= 1 and li["ntop_shd"] >= 1 and li["shd_half"] and li["chunk"] == 256
        _spill_fits(li)  # (whether a kernel spills by default is the occupancy rule's choice)


def _per_cu(li, d):
    """Both grids one block per CU: equal, and the default grids whole multiples of them."""
    g = li["wf_ext_grid"]
    return g == li["wf_shd_grid"] and d["wf_ext_grid"] % g == 0 and d["wf_shd_grid"] % g == 0 and \
        max(d["wf_ext_grid"], d["wf_shd_grid"]) > g


KNOBS = {
    "ntop 0": ({"MFX_NTOP": "0"}, lambda li, d: li["ntop_ext"] == 0 and li["ntop_shd"] == 0),
    "ntop 1": ({"MFX_NTOP": "1"}, lambda li, d: li["ntop_ext"] == 1 and li["ntop_shd"] == 1),
    "no slots in LDS": ({"MFX_SLOT_LDS": "0"}, lambda li, d: li["nslot_ext"] == 0 and li["nslot_shd"] == 0),
    "shadow 3 waves": ({"MFX_SHADOW_WAVES": "3"}, lambda li, d: li["shadow_waves"] == 3),
    "shadow 4 waves": ({"MFX_SHADOW_WAVES": "4"}, lambda li, d: li["shadow_waves"] == 4),
    "whole shadow chunks": ({"MFX_SHD_HALF": "0"}, lambda li, d: not li["shd_half"]),
    "half shadow chunks": ({"MFX_SHD_HALF": "1"}, lambda li, d: li["shd_half"]),
    "one block per CU": ({"MFX_BLOCKS_PER_CU": "1"}, _per_cu),
    "one camera block per CU": ({"MFX_CAM_BLOCKS": "1"},
                                lambda li, d: li["wf_cam_grid"] > 0 and d["wf_cam_grid"] % li["wf_cam_grid"] == 0 and
                                li["wf_cam_grid"] * 8 >= d["wf_cam_grid"]),
    "lit mask not in the HIT word": ({"MFX_NO_LIT_IN_HIT": "1"}, lambda li, d: not li["lit_in_hit"]),
}
ALL_TOGETHER = {"MFX_NTOP": "1", "MFX_SLOT_LDS": "0", "MFX_SHD_HALF": "0", "MFX_BLOCKS_PER_CU": "1", "MFX_CAM_BLOCKS": "1",
                "MFX_NO_LIT_IN_HIT": "1"}


# cube_cornell is the only scene with slots in LDS by default, and a two-level scene runs no camera packets
# (test_default_shapes): those variables select nothing elsewhere
KNOB_CASES = [(n, k) for k in KNOBS for n in KNOB_SCENES
              if not (k == "no slots in LDS" and n != "cube_cornell") and not (k == "one camera block per CU" and "@2l" in n)]


@pytest.mark.parametrize("name,knob", KNOB_CASES)
def test_residency_knob(gpu, oracle, monkeypatch, defaults, name, knob):
    """One variable off the default: launch_info shows it, image and ray counts are the oracle's."""
    env, shows = KNOBS[knob]
    with _ctx(monkeypatch, _named(name), env) as ctx:
        li = ctx.launch_info()
        assert shows(li, defaults[name]), (knob, li, defaults[name])
        _spill_fits(li)
        _image_exact(ctx, *_named_answer(oracle, name), what=knob)


@pytest.mark.parametrize("name", KNOB_SCENES[:2])
def test_one_camera_block_per_cu_is_one_block_per_cu(gpu, monkeypatch, defaults, name):
    """MFX_CAM_BLOCKS=1 and MFX_BLOCKS_PER_CU=1 give the same grid: the device's CU count."""
    assert defaults[name]["camera_packets"]
    with _ctx(monkeypatch, _named(name), {"MFX_CAM_BLOCKS": "1", "MFX_BLOCKS_PER_CU": "1"}) as ctx:
        li = ctx.launch_info()
    assert li["wf_cam_grid"] == li["wf_ext_grid"] == li["wf_shd_grid"], li


@pytest.mark.parametrize("name", KNOB_SCENES)
def test_max_depth_5(gpu, oracle, monkeypatch, name):
    """max_depth > 3 turns lit_in_hit off without a variable."""
    with _ctx(monkeypatch, _named(name, 5)) as ctx:
        assert not ctx.launch_info()["lit_in_hit"]
        _image_exact(ctx, *_named_answer(oracle, name, 5))


@pytest.mark.parametrize("name", KNOB_SCENES)
@pytest.mark.parametrize("depth", [3, 5])
def test_all_residency_knobs_together(gpu, oracle, monkeypatch, defaults, name, depth):
    d = defaults[name]
    env = dict(ALL_TOGETHER, MFX_SHADOW_WAVES=str(7 - d["shadow_waves"]))  # the other k_shadow build
    with _ctx(monkeypatch, _named(name, depth), env) as ctx:
        li = ctx.launch_info()
        assert li["ntop_ext"] == 1 and li["ntop_shd"] == 1 and li["nslot_ext"] == 0 and li["nslot_shd"] == 0, li
        assert li["shadow_waves"] == 7 - d["shadow_waves"] and not li["shd_half"] and not li["lit_in_hit"], li
        assert li["wf_ext_grid"] == li["wf_shd_grid"] and d["wf_ext_grid"] % li["wf_ext_grid"] == 0, li
        assert li["wf_cam_grid"] == (li["wf_ext_grid"] if d["camera_packets"] else 0), li
        _image_exact(ctx, *_named_answer(oracle, name, depth))


# ---- f. more instance records than LDS holds --------------------------------------------------------------
@pytest.mark.parametrize("m", [64, 65, 100])
def test_instances_beyond_the_lds_records(gpu, oracle, monkeypatch, m):
    """WF_INST_LDS = 64 records live in LDS; instance 64 and up are read from global memory. Exactly 64,
    65, and the 100 of the bound-67 scene, two-level and flattened."""
    from mafrixraytracing_amd.abi import MFX_F_FLATTEN
    a = deep_scene(TWO67) if m == 100 else chain_instanced(40, 0.7, 0.1, m, 0.85, spheres=True)
    rays = through_rays(a, M_RAYS, np.random.default_rng(4400 + m))
    tmax = np.random.default_rng(4500 + m).uniform(0.05, 3.0, size=M_RAYS)
    o = oracle_scene(oracle, a)
    want = (o.closest_hit(rays), o.any_hit(rays, tmax))
    prim = want[0][1]
    n = len(a.instancing[0])
    assert (prim >= 0).mean() >= 0.05 and (prim[prim >= 0] // n).max() == m - 1  # the last instance is hit
    ref, st = image_answer(oracle, a, name=("instances", m))
    assert st[1] > 0 and st[2] > 0
    a.two_level = True
    with _ctx(monkeypatch, a) as ctx:
        li = ctx.launch_info()
        assert li["ninst_lds"] == 64 and ctx.instancing_info()["instances"] == m, li
        _queries_exact(ctx, rays, tmax, want, "two-level")
        _image_exact(ctx, ref, st)
    a.two_level = False
    try:
        with _ctx(monkeypatch, a, flags=MFX_F_FLATTEN) as ctx:
            assert ctx.launch_info()["ninst_lds"] == 0 and ctx.instancing_info()["instances"] == 0
            _queries_exact(ctx, rays, tmax, want, "flattened")
            _image_exact(ctx, ref, st)
    finally:
        a.two_level = True


# ---- g. the limit -----------------------------------------------------------------------------------
def test_deepest_accepted_scene(gpu, oracle, monkeypatch):
    """A bound in [90, 96]: a context is created, and a 16x16x1 wavefront image and 2,000 query rays are
    the oracle's."""
    from mafrixraytracing_amd.abi import MFX_F_WAVEFRONT
    monkeypatch.setenv("MFX_LEAF_MAX", "1")
    a = with_film(deep_scene(DEEPEST), 16, 16, narrow=True)
    rays, tmax = query_rays(DEEPEST, 2000)
    want = query_answer(oracle, DEEPEST, 2000)
    assert (want[0][1] >= 0).mean() >= 0.05
    ref, st = image_answer(oracle, a, spp=1, name=(DEEPEST, 16))
    with _ctx(monkeypatch, a, flags=MFX_F_WAVEFRONT) as ctx:
        li = ctx.launch_info()
        assert 90 <= li["stack_size"] <= STACK_MAX and li["stack_size"] == stack_bound(a), li
        _spill_fits(li)
        _image_exact(ctx, ref, st, spp=1)
        _queries_exact(ctx, rays, tmax, want)
    assert st[1] > 0 and st[2] > 0, st


def test_too_deep_scene_is_refused(gpu, oracle, monkeypatch):
    """A bound of more than 96 entries: MFX_E_INVALID and "too deep"; a context created right after
    renders cornell exactly."""
    from mafrixraytracing_amd.abi import MFX_F_TWO_LEVEL, MfxInstance, MfxOptions
    from mafrixraytracing_amd.native import NativeContext
    monkeypatch.setenv("MFX_LEAF_MAX", "1")
    a = deep_scene(REFUSED)
    assert stack_bound(a) > STACK_MAX
    d = a.desc(templates=True)
    ins = a.instancing[1]
    opt = MfxOptions(seed=SEED, device=0, flags=MFX_F_TWO_LEVEL, part_index=0, part_count=1, ndevices=0, render_ahead=0,
                     devices=None)
    h = C.c_void_p()
    rc = gpu.mfx_create_instanced(C.byref(d), ins.ctypes.data_as(C.POINTER(MfxInstance)), len(ins), C.byref(opt), C.byref(h))
    assert rc == -1 and not h.value, rc
    assert b"too deep" in gpu.mfx_last_error(), gpu.mfx_last_error()
    monkeypatch.delenv("MFX_LEAF_MAX")
    c = scene("cornell", W, H)
    with NativeContext(c, seed=SEED) as ctx:
        _image_exact(ctx, *image_answer(oracle, c, name="cornell"))
