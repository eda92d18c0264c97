"""mfx_temporal's rule on the host, and the camera constructor the library exports (CPU only).
The derived camera is held against the CPU oracle's camera rays bit for bit; the numpy statement of the
rule (mafrixraytracing_amd/temporal.py) against a per-pixel restatement in Python floats and against
cases whose answer is known by construction; its use, on the oracle's images of two nearby cameras."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import SEED, scene
from denoise_helpers import scene_features
from temporal_helpers import history_of, moved, random_view, scalar_temporal, with_camera

W, H = 44, 36

CAMERAS = [
    {"position": (0.0, 1.0, 3.0), "direction": (0.0, 0.0, -1.0), "fov": 120.0, "aspect": 1.0},
    {"position": (2.4, 1.3, -3.4), "direction": (-2.4, -1.2, 3.4), "fov": 90.0, "aspect": 16.0 / 9.0},
    {"position": (-7.25, 0.3, 11.0), "direction": (0.3, -0.2, -0.9), "fov": 47.5, "aspect": 1.3},
    {"position": (1e3, -2e3, 5.5), "direction": (1.0, 1.0, 1.0), "fov": 170.0, "aspect": 0.5},
]


def _cfg(**kw):
    from mafrixraytracing_amd.temporal import TemporalConfig
    return TemporalConfig(**kw)


def _ray(cam, u, v):
    """PinholeCamera.GetRay from the twelve derived doubles, one rounding per operation."""
    o, tl, r, d = (np.asarray(cam[k], dtype=np.float64) for k in ("position", "topleft", "right", "down"))
    t = ((tl + r * u) + d * v) - o
    ln = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return o, t / ln


def test_symbols_and_struct():
    from mafrixraytracing_amd import abi
    lib = abi.load_library()
    for name in ("mfx_pinhole_derive", "mfx_camera_info", "mfx_set_camera", "mfx_temporal"):
        assert hasattr(lib, name), name
    assert C.sizeof(abi.MfxTemporalCfg) == 40 and abi.MfxTemporalCfg.tol_depth.offset == 16
    assert abi.MFX_DN_SRC_TEMPORAL == 3
    out = np.zeros(12)
    assert lib.mfx_pinhole_derive(None, abi.dptr(out)) == -1  # MFX_E_INVALID
    p = abi.pinhole_struct(CAMERAS[0])
    assert lib.mfx_pinhole_derive(C.byref(p), None) == -1
    assert lib.mfx_set_camera(None, C.byref(p)) == -1 and lib.mfx_camera_info(None, abi.dptr(out)) == -1


@pytest.mark.parametrize("cam", CAMERAS)
def test_derived_camera_gives_the_oracles_rays(oracle, cam):
    from mafrixraytracing_amd.temporal import pinhole_derive
    d = pinhole_derive(cam)
    assert np.array_equal(d["position"], np.array(cam["position"], dtype=np.float64))
    rng = np.random.default_rng(5)
    uv = [(0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.0, 1.0)] + [tuple(x) for x in rng.uniform(0.0, 1.0, (12, 2))]
    for u, v in uv:
        ro, rd = oracle.kat_camera_ray(cam["position"], cam["direction"], cam["fov"], cam["aspect"], float(u), float(v))
        o, dr = _ray(d, float(u), float(v))
        assert np.array_equal(o, ro) and np.array_equal(dr, rd), (cam, u, v)


def test_derived_fields_pass_through():
    from mafrixraytracing_amd.temporal import pinhole_derive
    given = {"position": (1.5, -2.0, 0.25), "topleft": (0.1, 0.2, 0.3), "right": (2.0, 0.0, 1e-3), "down": (0.0, -1.0, 0.5)}
    d = pinhole_derive(given)
    for k, v in given.items():
        assert np.array_equal(d[k], np.array(v)), k
    # and the constructor's output fed back in comes out as it went in
    c = pinhole_derive(CAMERAS[1])
    again = pinhole_derive(c)
    assert all(np.array_equal(c[k], again[k]) for k in c)


@pytest.mark.parametrize("w,h,seed", [(W, H, 1), (16, 8, 2), (5, 3, 3)])
def test_numpy_statement_equals_the_scalar_one(w, h, seed):
    from mafrixraytracing_amd.temporal import pinhole_derive, reference_temporal
    rng = np.random.default_rng(seed)
    base = {"position": (0.0, 1.0, 3.0), "direction": (0.0, 0.0, -1.0), "fov": 120.0, "aspect": w / h}
    cam_h = pinhole_derive(moved(base, rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.1, 0.1, 3)))
    cam_c = pinhole_derive(moved(base, rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.1, 0.1, 3)))
    npix = w * h
    hist = history_of(rng.uniform(0, 2, (npix, 3)), rng.uniform(0, 0.1, npix), rng.integers(1, 40, npix).astype(float),
                      random_view(rng, w, h, cam_h), cam_h)
    feat = random_view(rng, w, h, cam_c)
    color, var, cnt = rng.uniform(0, 2, (npix, 4)), rng.uniform(0, 0.1, npix), rng.integers(1, 9, npix).astype(float)
    total = 0
    for cfg in (_cfg(tol_depth=0.5, tol_normal2=0.5, max_history=16.0), _cfg(tol_depth=0.05, tol_normal2=0.0),
                _cfg(tol_depth=1e9, tol_normal2=1e9, max_history=1e9)):
        for restart in (False, True):
            got = reference_temporal(color, var, cnt, feat, cam_c, hist, w, h, cfg, restart=restart)
            want = scalar_temporal(color, var, cnt, feat, cam_c, hist, w, h, cfg, restart=restart)
            for g, x in zip(got[:3], want[:3]):
                assert np.array_equal(g, x), (cfg, restart)
            assert got[3] == want[3]
            assert restart is False or got[3] == 0
            total += got[3]
            new = got[4]
            assert np.array_equal(new.color, got[0][:, :3]) and np.array_equal(new.count, got[2])
            assert np.array_equal(new.depth, feat[:, 3]) and np.array_equal(new.hit, feat[:, 7])
    assert total > 0  # the cameras overlap: the accepting branch ran
    none = reference_temporal(color, var, cnt, feat, cam_c, None, w, h)
    assert none[3] == 0 and np.array_equal(none[0][:, :3], color[:, :3]) and np.array_equal(none[2], cnt)


def test_same_camera_is_the_count_weighted_merge():
    from mafrixraytracing_amd.temporal import pinhole_derive, reference_temporal
    rng = np.random.default_rng(7)
    npix = W * H
    cam = pinhole_derive(CAMERAS[0])
    feat = random_view(rng, W, H, cam)
    hfeat = feat.copy()
    hfeat[::5, 7] = 0.5  # some history pixels were not fully covered
    HC, HV, HN = rng.uniform(0, 2, (npix, 3)), rng.uniform(0, 0.1, npix), rng.integers(1, 100, npix).astype(float)
    hist = history_of(HC, HV, HN, hfeat, cam)
    Cc, V, n = rng.uniform(0, 2, (npix, 4)), rng.uniform(0, 0.1, npix), rng.integers(1, 9, npix).astype(float)
    for cap in (1e9, 8.0):
        frame, var, cnt, acc, new = reference_temporal(Cc, V, n, feat, cam, hist, W, H, _cfg(tol_depth=1e-9, tol_normal2=0.0,
                                                                                          max_history=cap))
        both = (feat[:, 7] == 1.0) & (hfeat[:, 7] == 1.0)
        assert acc == int(both.sum()) and 0 < acc < npix  # every such pixel reprojects to itself
        nh = np.minimum(HN, cap)
        nt = n + nh
        wc, wh = n / nt, nh / nt
        assert np.array_equal(frame[both, :3], (wc[:, None] * Cc[:, :3] + wh[:, None] * HC)[both])
        assert np.array_equal(var[both], ((wc * wc) * V + (wh * wh) * HV)[both])
        assert np.array_equal(cnt[both], nt[both])
        if cap == 8.0:
            assert (cnt[both] <= n[both] + 8.0).all() and (HN[both] > 8.0).any()
        # the others pass through
        assert np.array_equal(frame[~both, :3], Cc[~both, :3]) and np.array_equal(var[~both], V[~both])
        assert np.array_equal(cnt[~both], n[~both])
        assert np.array_equal(frame[:, 3], np.ones(npix))


def _wall(w, h, cam):
    """Features of a wall z = -4 facing a camera that looks down -z from `cam`'s position."""
    f = np.zeros((w * h, 8))
    for x in range(w):
        for y in range(h):
            o, d = _ray(cam, (x + 0.5) / w, (y + 0.5) / h)
            f[x * h + y] = [0.0, 0.0, 1.0, (-4.0 - o[2]) / d[2], 0.5, 0.5, 0.5, 1.0]
    return f


def test_wall_shifted_by_whole_pixels():
    """A 16x8 film over an image plane 2 x 1 at distance 1: a pixel's footprint on the wall at depth 4 is
    1/2. The camera moves 3 footprints along `right`: an interior pixel x takes history pixel x + 3, and the
    3 columns that came into view have no history."""
    from mafrixraytracing_amd.temporal import reference_temporal
    w, h, k = 16, 8, 3
    cam_a = {"position": (0.0, 0.0, 0.0), "topleft": (-1.0, 0.5, -1.0), "right": (2.0, 0.0, 0.0), "down": (0.0, -1.0, 0.0)}
    cam_b = {"position": (1.5, 0.0, 0.0), "topleft": (0.5, 0.5, -1.0), "right": (2.0, 0.0, 0.0), "down": (0.0, -1.0, 0.0)}
    npix = w * h
    HC = np.arange(npix, dtype=np.float64)[:, None] * np.ones(3)  # a history pixel's colour names it
    hist = history_of(HC, np.zeros(npix), np.full(npix, 4.0), _wall(w, h, cam_a), cam_a)
    Cc = np.zeros((npix, 4))
    frame, var, cnt, acc, new = reference_temporal(Cc, np.zeros(npix), np.full(npix, 4.0), _wall(w, h, cam_b), cam_b, hist,
                                                   w, h, _cfg(tol_depth=1e-6, tol_normal2=0.0))
    assert acc == (w - k) * h
    for x in range(w):
        for y in range(h):
            p = x * h + y
            if x < w - k:
                assert frame[p, 0] == 0.5 * ((x + k) * h + y) and cnt[p] == 8.0, (x, y)
            else:
                assert frame[p, 0] == 0.0 and cnt[p] == 4.0, (x, y)
    # the new history is the current view's
    assert np.array_equal(new.camera["position"], np.array(cam_b["position"]))


def test_disocclusion_is_rejected():
    from mafrixraytracing_amd.temporal import pinhole_derive, reference_temporal
    rng = np.random.default_rng(9)
    npix = W * H
    cam = pinhole_derive(CAMERAS[0])
    feat = random_view(rng, W, H, cam)
    feat[:, 7] = 1.0
    # ze, the distance the rule computes for the pixel's point from the (same) history eye, by its operations
    ze = np.zeros(npix)
    for x in range(W):
        for y in range(H):
            o, d = _ray(cam, (x + 0.5) / W, (y + 0.5) / H)
            e = (o + d * feat[x * H + y, 3]) - o
            ze[x * H + y] = math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    args = (rng.uniform(0, 2, (npix, 4)), np.zeros(npix), np.full(npix, 4.0), feat, cam)
    hcol = rng.uniform(0, 2, (npix, 3))

    def accepted(hfeat, **kw):
        hist = history_of(hcol, np.zeros(npix), np.full(npix, 8.0), hfeat, cam)
        r = reference_temporal(*args, hist, W, H, _cfg(**kw))
        return r[2] > 4.0

    far = feat.copy()
    far[:, 3] = ze
    far[::3, 3] = ze[::3] * 1.06  # another surface behind
    acc = accepted(far, tol_depth=0.05, tol_normal2=0.0)
    assert not acc[::3].any() and acc[1::3].all() and acc[2::3].all()
    turned = feat.copy()
    turned[:, 3] = ze
    turned[::4, 0:3] = feat[::4, 0:3] + np.array([0.0, 0.2, 0.0])  # d2 = 0.04
    acc = accepted(turned, tol_depth=0.05, tol_normal2=0.03)
    assert not acc[::4].any() and acc[1::4].all()
    assert accepted(turned, tol_depth=0.05, tol_normal2=0.05).all()
    # tol_depth = 0: only a history depth equal to ze, bit for bit
    exact = feat.copy()
    exact[:, 3] = ze
    exact[::2, 3] = np.nextafter(ze[::2], np.inf)
    acc = accepted(exact, tol_depth=0.0, tol_normal2=0.0)
    assert not acc[::2].any() and acc[1::2].all()


def test_history_lowers_the_error_after_a_small_move(oracle):
    """cornell at two nearby cameras, on the oracle: 32 spp before the move, 4 spp after it, against 256 spp
    of other samples at the new camera. tol_depth 0.1: a pixel of this 44-pixel film subtends 0.024 rad, so on
    a surface seen at 75 degrees from its normal the depth changes by 9 % from one pixel to the next, and
    the nearest history pixel may be half a pixel off on either side."""
    from mafrixraytracing_amd.temporal import pinhole_derive, reference_temporal
    a = scene("cornell", W, H)
    b = with_camera(a, moved(a.camera, dpos=(0.15, 0.05, -0.1)))
    npix = W * H
    before = oracle.OracleScene(a).sample(32, SEED)
    hist = history_of(before, np.zeros(npix), np.full(npix, 32.0), scene_features(oracle, a, 2, 0), pinhole_derive(a.camera))
    ob = oracle.OracleScene(b)
    raw = ob.sample(4, SEED, sample_base=32)
    truth = ob.sample(256, SEED, sample_base=1000)
    merged, _, cnt, acc, _ = reference_temporal(raw, np.zeros(npix), np.full(npix, 4.0), scene_features(oracle, b, 2, 32),
                                                pinhole_derive(b.camera), hist, W, H, _cfg(tol_depth=0.1, tol_normal2=0.01))

    def rmse(f):
        return float(np.sqrt(((f[:, :3] - truth[:, :3]) ** 2).mean()))

    print("accepted", acc, "of", npix, "rmse raw", rmse(raw), "merged", rmse(merged))
    assert acc > 0
    assert rmse(merged) < rmse(raw)
