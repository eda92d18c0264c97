"""Camera packets started from the per-tile BVH cut (k_camera's CUTS instances, mfx_camera_cuts.h) against
the same packets started from the root (MFX_CAMERA_CUTS=0): the FP64 accumulator and the ray counts are
equal bit for bit, on every scene kind, at forced capacities, at edge-case cameras, across camera changes,
on row partitions, several generations and listed traces; the device-built table equals the host twin's
byte for byte. Every case is small (films of at most 96 x 54) and traces 4 samples.
MFX_CAMERA_CUT_MIN_SAMPLES=1 makes every trace build and use the table, whatever the default threshold."""
import numpy as np
import pytest

from conftest import SEED, scene
from gpu_helpers import ctx_env, oracle_frame
from temporal_helpers import moved, with_camera

pytestmark = pytest.mark.gpu

SPP = 4
ON = {"MFX_CAMERA_CUT_MIN_SAMPLES": "1"}
OFF = {"MFX_CAMERA_CUTS": "0"}
SOUP = (777, 40000, 0, False)  # soup_helpers.IMAGE_SOUPS[0]

_off = {}


def _arrays(name, w, h):
    if name == "soup":
        from soup_helpers import soup_case
        return soup_case(*SOUP).with_film(w, h)
    return scene(name, w, h)


def _trace(a, env, spp=SPP, **kw):
    """(accumulator, ray counts, launch_info) of one trace of spp samples from a context created under env."""
    with ctx_env(a, env, **kw) as ctx:
        ctx.trace_accumulate(spp, 0)
        acc = ctx.accum_read_mean(1.0)
        return acc, ctx.ray_counts()[:3].copy(), ctx.launch_info()


def _off_answer(name, w, h):
    """The cuts-off trace of a case: computed once, left unchanged."""
    key = (name, w, h)
    if key not in _off:
        acc, counts, li = _trace(_arrays(name, w, h), OFF)
        assert li["camera_packets"] and not li["camera_cuts"] and li["cut_builds"] == 0
        acc.setflags(write=False)
        _off[key] = (acc, counts)
    return _off[key]


def _assert_same(got, want, what=""):
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), (what, int(np.any(got[0] != want[0], axis=1).sum()))


CASES = [(n, w, h) for n in ("spot", "cube_cornell", "two_spheres_plane", "soup") for (w, h) in ((96, 54), (17, 9))]
CASES.append(("renault", 40, 24))


@pytest.mark.parametrize("name,w,h", CASES)
def test_cuts_on_equals_cuts_off(gpu, oracle, name, w, h):
    want = _off_answer(name, w, h)
    acc, counts, li = _trace(_arrays(name, w, h), ON)
    assert li["camera_cuts"] and li["cut_builds"] == 1 and li["cut_cap"] == 8 and li["cut_table_bytes"] > 0
    assert 0 < li["cut_len_max"] <= 8
    _assert_same((acc, counts), want, name)
    if name != "soup":  # and both equal the oracle's Sample(4): its mean times 4 is the sum's last rounding away
        frame, st = oracle_frame(oracle, name, w, h, 3, SPP)
        assert tuple(counts) == st
        with ctx_env(_arrays(name, w, h), ON) as ctx:
            assert np.array_equal(ctx.sample(SPP), frame)


@pytest.mark.parametrize("name,w,h", [("spot", 96, 54), ("renault", 40, 24), ("soup", 17, 9)])
@pytest.mark.parametrize("cap", [1, 2, None])
def test_forced_capacities(gpu, name, w, h, cap):
    env = dict(ON)
    if cap is not None:
        env["MFX_CAMERA_CUT_CAP"] = str(cap)
    acc, counts, li = _trace(_arrays(name, w, h), env)
    assert li["camera_cuts"] and li["cut_cap"] == (cap or 8) and li["cut_len_max"] <= (cap or 8)
    if cap == 1:
        assert li["cut_root_tiles"] > 0  # a tile whose pyramid meets two children of the root keeps {root}
    if cap is None:
        assert li["cut_root_tiles"] == 0
    _assert_same((acc, counts), _off_answer(name, w, h), (name, cap))


# tests/test_gpu_parity.py's _CONE_CAMERAS: on a wall's plane, at a vertex, grazing the floor, inside the mesh,
# close to it, far and narrow
EDGE_CAMERAS = [
    ("cube_cornell", {"position": (0.0, 0.0, 0.5), "direction": (0.0, 0.2, -1.0), "fov": 100.0}),
    ("cube_cornell", {"position": (-1.0, 0.0, 0.99), "direction": (1.0, 0.8, -1.0), "fov": 90.0}),
    ("cube_cornell", {"position": (0.0, 1e-7, 0.9), "direction": (0.0, 0.0, -1.0), "fov": 120.0}),
    ("spot", {"position": (0.0, 0.0, 0.0), "direction": (0.3, -0.2, 1.0), "fov": 110.0}),
    ("spot", {"position": (0.33, -0.39, 0.45), "direction": (-0.1, -0.05, -1.0), "fov": 60.0}),
    ("spot", {"position": (240.0, 120.0, -340.0), "direction": (-2.4, -1.2, 3.4), "fov": 0.6}),
    ("renault", None),
]


@pytest.mark.parametrize("name,cam", EDGE_CAMERAS)
def test_edge_case_cameras(gpu, name, cam):
    a = scene(name, 40, 24)
    if cam is not None:
        c = dict(a.camera)
        c.update(cam)
        a = with_camera(a, c)
    on = _trace(a, ON)
    assert on[2]["camera_cuts"] and on[2]["cut_builds"] == 1
    _assert_same(on, _trace(a, OFF), (name, cam))


def _fresh(a):
    return _trace(a, ON)[:2]


@pytest.mark.parametrize("name,move,rebuilds", [("spot", dict(dpos=(-0.4, 0.1, 0.6), ddir=(0.1, 0.0, 0.0)), 0),
                                                ("cornell", dict(dpos=(0.5, 0.5, 5.0)), 1)])
def test_camera_changes_rebuild_the_table(gpu, name, move, rebuilds):
    """To a second camera and back (the second case's position needs a larger eps: the images are built
    again): each trace is a fresh context's with that camera, and the table is built exactly when the
    camera epoch moved."""
    a = scene(name, 44, 36)
    cam_b = moved(a.camera, **move)
    b = with_camera(a, cam_b)
    want_a, want_b = _fresh(a), _fresh(b)

    def step(ctx, want, epoch, builds):
        ctx.accum_clear()
        ctx.trace_accumulate(SPP, 0)
        _assert_same((ctx.accum_read_mean(1.0), ctx.ray_counts()[:3]), want, (name, epoch))
        assert ctx.camera_info()["epoch"] == epoch and ctx.launch_info()["cut_builds"] == builds

    with ctx_env(a, ON) as ctx:
        assert ctx.launch_info()["cut_builds"] == 0  # lazily: nothing before the first k_camera launch
        step(ctx, want_a, 0, 1)
        step(ctx, want_a, 0, 1)
        ctx.set_camera(cam_b)
        assert ctx.camera_info()["rebuilds"] == rebuilds
        step(ctx, want_b, 1, 2)
        ctx.set_camera(cam_b)  # the current camera: no new epoch, no build
        step(ctx, want_b, 1, 2)
        ctx.set_camera(a.camera)
        step(ctx, want_a, 2, 3)


def test_row_partition_and_generations(gpu):
    """Part 1 of 3 of the tile rows, and MFX_POOL=2048: generations of 4,096 paths where 8 samples of the
    partition's tiles are more; the table is indexed by film tile, whatever the trace covers."""
    from mafrixraytracing_amd.abi import MFX_F_ROW_PARTITION
    a = scene("spot", 44, 36)
    for env in ({}, {"MFX_POOL": "2048"}):
        kw = dict(flags=MFX_F_ROW_PARTITION, part_index=1, part_count=3)
        on = _trace(a, dict(ON, **env), spp=8, **kw)
        assert on[2]["camera_cuts"] and on[2]["cut_builds"] == 1
        _assert_same(on, _trace(a, dict(OFF, **env), spp=8, **kw), env)


def test_listed_traces(gpu):
    """mfx_sample_adaptive and mfx_sample_adaptive_resume (k_camera's LIST instances)."""
    a = scene("spot", 44, 36)
    out = []
    for env in (ON, OFF):
        with ctx_env(a, env) as ctx:
            f1, t1 = ctx.sample_adaptive(2, 8, 2, 0.3, 0.01)
            c1 = ctx.ray_counts()[:3].copy()
            f2, t2, active = ctx.sample_adaptive_resume(14, 4, 0.1, 0.01)
            out.append((f1, t1, c1, f2, t2, active, ctx.ray_counts()[:3].copy()))
            assert ctx.launch_info()["cut_builds"] == (1 if env is ON else 0)
    assert out[0][4].max() > 2  # some tile went on past the first pass: its later passes were listed traces
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_device_table_equals_the_host_twin(gpu):
    with ctx_env(scene("spot", 96, 54), ON) as ctx:
        dev, host = ctx.camera_cut_table(), ctx.camera_cut_table(host=True)
        info = ctx.camera_cut_info()
    assert dev.shape == (12 * 7, 8, 32) and np.array_equal(dev, host)
    codes = np.ascontiguousarray(dev[:, :, :4]).view(np.int32)[:, :, 0]
    lengths = (codes != -2**31).sum(axis=1)
    assert info["builds"] == 1 and info["tiles"] == 84 and info["len_sum"] == lengths.sum() and info["len_max"] == lengths.max()
    assert lengths.max() > 1 and (codes < 0).any() and info["hist"][:9] == np.bincount(lengths, minlength=9).tolist()
