"""The per-tile slot cull of the camera cuts and the ray-free windows of empty tiles (mfx_camera_cuts.h,
k_camera's CUTS instances) against the same packets started from the root (MFX_CAMERA_CUTS=0): the FP64
accumulator and the ray counts are equal bit for bit. Films are 40 x 24 and 17 x 9 (edge tiles padded), 4
samples a trace. The scenes: spot, cube_cornell, the mixed soup with rects and spheres, a camera that sees
nothing (every tile's cut is empty: no window makes a ray) and one inside a closed view (no tile's is);
forced capacities 1, 2, 8 and 16; the edge-case cameras of test_camera_packets_at_edge_case_cameras; a
camera change from the empty view to a full one; a row partition and listed traces; the device table equal
to the host twin's byte for byte, narrowed leaf codes among its entries; and the rule that a table gets the
cull only once its camera has served MFX_CAMERA_CUT_CULL_MIN_SAMPLES samples."""
import numpy as np
import pytest

from conftest import scene
from gpu_helpers import ctx_env
from temporal_helpers import with_camera

pytestmark = pytest.mark.gpu

SPP = 4
# every trace builds and uses a table, and builds it with the slot cull, whatever the default thresholds
ON = {"MFX_CAMERA_CUT_MIN_SAMPLES": "1", "MFX_CAMERA_CUT_CULL_MIN_SAMPLES": "1"}
OFF = {"MFX_CAMERA_CUTS": "0"}
SOUP = (777, 40000, 0, False)  # soup_helpers.IMAGE_SOUPS[0]
FILMS = ((40, 24), (17, 9))
# far from the spot scene and turned away from it: every tile's pyramid misses every box
NOTHING = {"position": (24.0, 13.0, -34.0), "direction": (2.4, 1.2, -3.4), "fov": 40.0}
# tests/test_gpu_parity.py's _CONE_CAMERAS
EDGE_CAMERAS = [
    ("cube_cornell", {"position": (0.0, 0.0, 0.5), "direction": (0.0, 0.2, -1.0), "fov": 100.0}),
    ("cube_cornell", {"position": (-1.0, 0.0, 0.99), "direction": (1.0, 0.8, -1.0), "fov": 90.0}),
    ("cube_cornell", {"position": (0.0, 1e-7, 0.9), "direction": (0.0, 0.0, -1.0), "fov": 120.0}),
    ("spot", {"position": (0.0, 0.0, 0.0), "direction": (0.3, -0.2, 1.0), "fov": 110.0}),
    ("spot", {"position": (0.33, -0.39, 0.45), "direction": (-0.1, -0.05, -1.0), "fov": 60.0}),
    ("spot", {"position": (240.0, 120.0, -340.0), "direction": (-2.4, -1.2, 3.4), "fov": 0.6}),
    ("renault", None),
]

_off = {}


def _arrays(name, w, h):
    if name == "soup":
        from soup_helpers import soup_case
        return soup_case(*SOUP).with_film(w, h)
    if name == "nothing":
        a = scene("spot", w, h)
        return with_camera(a, dict(a.camera, **NOTHING))
    return scene(name, w, h)


def _trace(a, env, spp=SPP, **kw):
    """(accumulator, ray counts, launch_info, camera_cut_info) of one trace from a context created under env."""
    with ctx_env(a, env, **kw) as ctx:
        ctx.trace_accumulate(spp, 0)
        acc = ctx.accum_read_mean(1.0)
        return acc, ctx.ray_counts()[:3].copy(), ctx.launch_info(), ctx.camera_cut_info()


def _off_answer(name, w, h):
    """The cuts-off trace of a case: computed once, left unchanged."""
    key = (name, w, h)
    if key not in _off:
        acc, counts, li, _ = _trace(_arrays(name, w, h), OFF)
        assert li["camera_packets"] and not li["camera_cuts"] and li["cut_builds"] == 0
        acc.setflags(write=False)
        _off[key] = (acc, counts)
    return _off[key]


def _assert_same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), (what, int(np.any(got[0] != want[0], axis=1).sum()))


@pytest.mark.parametrize("w,h", FILMS)
@pytest.mark.parametrize("name", ["spot", "cube_cornell", "soup", "nothing"])
def test_cull_on_equals_cuts_off(gpu, name, w, h):
    want = _off_answer(name, w, h)
    acc, counts, li, info = _trace(_arrays(name, w, h), ON)
    assert li["camera_cuts"] and li["cut_builds"] == 1 and li["cut_cap"] == 8
    _assert_same((acc, counts), want, name)
    assert info["slots_culled"] <= info["slots_seen"] and info["leaves_dropped"] + info["leaves_narrowed"] <= info["slots_seen"]
    if name == "nothing":  # every tile is empty: no ray is made, every path is a counted miss
        assert info["empty_tiles"] == info["tiles"] and info["len_sum"] == 0
        assert counts[0] == w * h * SPP and counts[1] == 0 and counts[2] == 0
    if name == "cube_cornell":  # the camera looks into the box: no tile is empty
        assert info["empty_tiles"] == 0
    if (name, w) in (("spot", 40), ("cube_cornell", 40), ("soup", 17)):  # (the host twin's figures for these films)
        assert info["slots_culled"] > 0


@pytest.mark.parametrize("name,w,h", [("spot", 40, 24), ("soup", 17, 9)])
@pytest.mark.parametrize("cap", [1, 2, 8, 16])
def test_forced_capacities(gpu, name, w, h, cap):
    acc, counts, li, info = _trace(_arrays(name, w, h), dict(ON, MFX_CAMERA_CUT_CAP=str(cap)))
    assert li["camera_cuts"] and li["cut_cap"] == cap and li["cut_len_max"] <= cap
    _assert_same((acc, counts), _off_answer(name, w, h), (name, cap))


@pytest.mark.parametrize("name,cam", EDGE_CAMERAS)
def test_edge_case_cameras(gpu, name, cam):
    a = scene(name, 40, 24)
    if cam is not None:
        a = with_camera(a, dict(a.camera, **cam))
    on = _trace(a, ON)
    assert on[2]["camera_cuts"] and on[2]["cut_builds"] == 1
    _assert_same(on, _trace(a, OFF), (name, cam))


def test_camera_change_fills_empty_tiles(gpu):
    """From the view of nothing to the scene's own camera through mfx_set_camera: the table is rebuilt, tiles
    that were empty are no longer, and the trace is a fresh context's."""
    full = scene("spot", 40, 24)
    with ctx_env(_arrays("nothing", 40, 24), ON) as ctx:
        ctx.trace_accumulate(SPP, 0)
        _assert_same((ctx.accum_read_mean(1.0), ctx.ray_counts()[:3]), _off_answer("nothing", 40, 24), "nothing")
        before = ctx.camera_cut_info()
        assert before["builds"] == 1 and before["empty_tiles"] == before["tiles"] == 15
        ctx.set_camera(full.camera)
        ctx.accum_clear()
        ctx.trace_accumulate(SPP, 0)
        _assert_same((ctx.accum_read_mean(1.0), ctx.ray_counts()[:3]), _off_answer("spot", 40, 24), "spot")
        after = ctx.camera_cut_info()
        assert after["builds"] == 2 and after["empty_tiles"] < 15 and after["len_sum"] > 0


def test_cull_waits_for_a_camera_that_stays(gpu):
    """MFX_CAMERA_CUT_CULL_MIN_SAMPLES=8 and traces of 4 samples: a camera's first trace builds the plain
    table, its second (8 samples served) the culled one, which later traces keep; a camera change starts
    over. Every trace equals the cuts-off one."""
    a = scene("spot", 40, 24)
    want = _off_answer("spot", 40, 24)
    with ctx_env(a, {"MFX_CAMERA_CUT_MIN_SAMPLES": "1", "MFX_CAMERA_CUT_CULL_MIN_SAMPLES": "8"}) as ctx:
        def step(builds, culled):
            ctx.accum_clear()
            ctx.trace_accumulate(SPP, 0)
            _assert_same((ctx.accum_read_mean(1.0), ctx.ray_counts()[:3]), want, (builds, culled))
            info = ctx.camera_cut_info()
            assert info["builds"] == builds and info["culled"] == culled and (info["slots_culled"] > 0) == culled

        step(1, False)
        step(2, True)
        step(2, True)
        ctx.set_camera(dict(a.camera, **NOTHING))
        ctx.trace_accumulate(SPP, 0)
        assert ctx.camera_cut_info()["builds"] == 3 and not ctx.camera_cut_info()["culled"]
        ctx.set_camera(a.camera)
        step(4, False)
        step(5, True)


def test_row_partition_and_listed_traces(gpu):
    from mafrixraytracing_amd.abi import MFX_F_ROW_PARTITION
    a = scene("spot", 40, 24)
    kw = dict(flags=MFX_F_ROW_PARTITION, part_index=1, part_count=3)
    on = _trace(a, ON, spp=8, **kw)
    assert on[2]["camera_cuts"] and on[2]["cut_builds"] == 1
    _assert_same(on, _trace(a, OFF, spp=8, **kw), "partition")
    out = []
    for env in (ON, OFF):  # mfx_sample_adaptive and its resume: k_camera's LIST instances
        with ctx_env(a, env) as ctx:
            f1, t1 = ctx.sample_adaptive(2, 8, 2, 0.3, 0.01)
            c1 = ctx.ray_counts()[:3].copy()
            f2, t2, active = ctx.sample_adaptive_resume(14, 4, 0.1, 0.01)
            out.append((f1, t1, c1, f2, t2, active, ctx.ray_counts()[:3].copy()))
            assert ctx.launch_info()["cut_builds"] == (1 if env is ON else 0)
    for x, y in zip(*out):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name,w,h,cap", [("spot", 40, 24, 8), ("spot", 40, 24, 16), ("soup", 17, 9, 8), ("cube_cornell", 40, 24, 2)])
def test_device_table_equals_the_host_twin(gpu, name, w, h, cap):
    with ctx_env(_arrays(name, w, h), dict(ON, MFX_CAMERA_CUT_CAP=str(cap))) as ctx:
        dev, host = ctx.camera_cut_table(), ctx.camera_cut_table(host=True)
        info = ctx.camera_cut_info()
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert dev.shape == (tiles, cap, 32) and np.array_equal(dev, host)
    codes = np.ascontiguousarray(dev[:, :, :4]).view(np.int32)[:, :, 0]
    lengths = (codes != -2**31).sum(axis=1)
    assert info["tiles"] == tiles and info["len_sum"] == lengths.sum() and info["empty_tiles"] == (lengths == 0).sum()
    assert info["hist"][:cap + 1] == np.bincount(lengths, minlength=cap + 1).tolist()
    if name == "spot":  # entries dropped and narrowed codes are among what was compared
        assert info["slots_seen"] > info["slots_culled"] > 0 and info["leaves_dropped"] > 0 and info["leaves_narrowed"] > 0
