"""The thin lens on the CPU (mfx_set_lens): the library's host-only statements of the rule (mfx_lens_derive,
mfx_lens_rays: the header the kernels compile) against the Python statement (mafrixraytracing_amd/lens.py), bit
for bit; the focus property; the restatement of the path trace with the lens ray (tests/lens_helpers.py) against
the ones it is built on; unbiasedness where depth of field cannot matter; and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import lights_helpers
from conftest import SEED, scene
from lens_helpers import (FOCUS_APERTURE, FOCUS_DISTANCE, FOCUS_H, FOCUS_SPP, FOCUS_W, film_mean_and_error, focus_plane_scene,
                          reference_paths)
from lights_helpers import film_paths
from mafrixraytracing_amd import abi
from mafrixraytracing_amd import lens as lens_py

W, H, SPP = 19, 13, 2
SEED64 = 0xC0FFEE12_3456789B
LENS = (0.07, 2.6)


def _cameras():
    a = scene("cornell", W, H)
    made = dict(a.camera)
    d = abi.pinhole_derive(made)
    # a derived camera that no constructor gives: a sheared, rescaled film plane
    derived = {"position": tuple(d["position"] + np.array((0.11, -0.07, 0.05))),
               "topleft": tuple(d["topleft"] + np.array((0.02, 0.01, -0.03))),
               "right": tuple(d["right"] * 1.1 + np.array((0.0, 0.03, 0.0))),
               "down": tuple(d["down"] * 0.9 + np.array((0.02, 0.0, 0.01)))}
    return {"constructed": made, "derived": derived}


CAMERAS = _cameras()


def test_mix64_is_the_oracles(oracle):
    """lens.py's own mix64 and draw against pyoracle.rng_draws on a path's low counters."""
    for seed, pixel, sample in ((SEED, 0, 0), (SEED64, 19 * 13 - 1, 7), (SEED64, 123456, (1 << 31) + 5)):
        want = oracle.rng_draws(seed, pixel, sample, 12)
        key = lens_py.path_key(seed, pixel, sample)
        got = np.array([lens_py.draw(key, m) for m in range(1, 13)])
        assert np.array_equal(got, want)


def _rays(cam, lens=LENS):
    px, py, smp = film_paths(W, H, SPP)
    out, trials = abi.lens_rays(cam, lens, SEED64, W, H, px, py, smp)
    return px, py, smp, out, trials


@pytest.mark.parametrize("which", list(CAMERAS))
def test_host_statement(which):
    cam = CAMERAS[which]
    assert abi.pinhole_struct(cam).derived == (1 if which == "derived" else 0)
    d = abi.pinhole_derive(cam)
    rec = lens_py.derive(d, *LENS)
    got = abi.lens_derive(cam, LENS)
    assert np.array_equal(got, np.array(rec["U"] + rec["V"] + (rec["s"],)))
    if which == "constructed":
        assert abs(rec["dplane"] - 0.5) < 1e-12
    px, py, smp, out, trials = _rays(cam)
    assert len(out) == W * H * SPP and trials.max() > 1 and trials.min() == 1  # some path took more than one trial
    for k in range(len(out)):
        o, dd, a, b, t, _ = lens_py.path_ray(d, rec, SEED64, W, H, int(px[k]), int(py[k]), int(smp[k]))
        assert np.array_equal(out[k], np.array(o + dd + (a, b))), k
        assert trials[k] == t
    assert np.all(out[:, 6] ** 2 + out[:, 7] ** 2 < 1.0)
    # an aperture of 0 is the pinhole ray up to the rounding of pin * s: the same origin exactly
    zero, _ = abi.lens_rays(cam, (0.0, LENS[1]), SEED64, W, H, px[:8], py[:8], smp[:8])
    assert np.array_equal(zero[:, :3], np.tile(d["position"], (8, 1)))


@pytest.mark.parametrize("which", list(CAMERAS))
def test_focus_property(which):
    """Ray(o, d) meets the plane dot(x - P0, f) = focus at fp, within 1e-12 * (|P0| + focus): a rounding bound."""
    cam = CAMERAS[which]
    d = abi.pinhole_derive(cam)
    rec = lens_py.derive(d, *LENS)
    px, py, smp, out, _ = _rays(cam)
    P0, f, focus = np.array(d["position"]), np.array(rec["f"]), LENS[1]
    bound = 1e-12 * (float(np.linalg.norm(P0)) + focus)
    worst = 0.0
    for k in range(len(out)):
        fp = np.array(lens_py.path_ray(d, rec, SEED64, W, H, int(px[k]), int(py[k]), int(smp[k]))[5])
        o, dd = out[k, :3], out[k, 3:6]
        t = (focus - float(np.dot(o - P0, f))) / float(np.dot(dd, f))
        worst = max(worst, float(np.linalg.norm(o + dd * t - fp)))
        assert abs(float(np.dot(fp - P0, f)) - focus) <= bound  # fp lies in the focus plane
    print("focus property: worst distance", worst, "bound", bound)
    assert worst <= bound


def test_restatement_without_the_lens_step(oracle):
    """With the lens step skipped, lens_helpers.reference_paths is lights_helpers.reference_paths, bit for bit."""
    w, h, spp = 16, 12, 2
    a = scene("cornell", w, h)
    px, py, smp = film_paths(w, h, spp)
    osc = oracle.OracleScene(a)
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 3, lens=None, oscene=osc)
    want, wcounts, _, _ = lights_helpers.reference_paths(a, [a.light], SEED, px, py, smp, 3, oscene=osc)
    assert np.array_equal(rad, want) and np.array_equal(counts, wcounts)
    assert np.array_equal(rad, osc.paths(px, py, smp, SEED)[0])
    # and with it, the image differs and the primary rays are the same
    lrad, lcounts = reference_paths(a, [a.light], SEED, px, py, smp, 3, lens=(0.1, 2.5), oscene=osc)
    assert not np.array_equal(lrad, want) and lcounts[0] == wcounts[0]
    assert oracle.kat_camera_ray.__module__ == "pyoracle"  # nothing is left in place


def test_unbiased_in_the_focus_plane(oracle):
    """One rect in the focus plane, one light: the film mean with a lens and without agree within four standard
    errors of their difference (from the per-sample variances of the two runs, on disjoint samples). Observed:
    2.34842 +- 0.01273 with the lens, 2.35922 +- 0.01272 without at 16 x 12 x 128."""
    a = focus_plane_scene()
    osc = oracle.OracleScene(a)
    px, py, smp = film_paths(FOCUS_W, FOCUS_H, FOCUS_SPP)
    pin, _ = reference_paths(a, [a.light], SEED, px, py, smp, a.max_depth, oscene=osc)
    got, _ = reference_paths(a, [a.light], SEED, px, py, smp + 4096, a.max_depth, lens=(FOCUS_APERTURE, FOCUS_DISTANCE), oscene=osc)
    (m0, e0), (m1, e1) = film_mean_and_error(pin), film_mean_and_error(got)
    print(f"focus plane: lens {m1:.5f} +- {e1:.5f}, pinhole {m0:.5f} +- {e0:.5f}")
    assert m0 > 0.1 and e0 > 0.0 and e1 > 0.0
    assert abs(m1 - m0) <= 4.0 * math.sqrt(e0 * e0 + e1 * e1)
    # (the rect's edges are on the film: some paths hit it, some leave)
    hit0 = np.count_nonzero(pin.any(axis=1))
    assert 0 < hit0 < len(pin)


def _refused(fn, what):
    with pytest.raises(abi.MfxError, match=r"\(-1\)") as e:
        fn()
    assert what in str(e.value), str(e.value)


def test_refusals():
    cam = CAMERAS["constructed"]
    d = abi.pinhole_derive(cam)
    one = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int64))
    for call in (lambda c, l: abi.lens_derive(c, l), lambda c, l: abi.lens_rays(c, l, SEED, W, H, *one)):
        for ap in (-0.1, math.nan, math.inf):
            _refused(lambda: call(cam, (ap, 1.0)), "aperture")
        for fo in (0.0, -1.0, math.nan, math.inf):
            _refused(lambda: call(cam, (0.1, fo)), "focus")
        flat = dict(position=d["position"], topleft=d["topleft"], right=(0.0, 0.0, 0.0), down=d["down"])
        _refused(lambda: call(flat, LENS), "(lr)")
        flat = dict(position=d["position"], topleft=d["topleft"], right=d["right"], down=(0.0, 0.0, 0.0))
        _refused(lambda: call(flat, LENS), "(ld)")
        flat = dict(position=d["position"], topleft=d["topleft"], right=d["right"], down=d["right"])
        _refused(lambda: call(flat, LENS), "(ln)")
        behind = dict(position=d["position"], topleft=2.0 * d["position"] - d["topleft"], right=d["right"], down=d["down"])
        _refused(lambda: call(behind, LENS), "dplane")
        inplane = dict(position=d["topleft"], topleft=d["topleft"], right=d["right"], down=d["down"])
        _refused(lambda: call(inplane, LENS), "dplane")
        huge = dict(position=d["position"], topleft=d["topleft"], right=d["right"] * 1e100, down=d["down"] * 1e100)
        _refused(lambda: call(huge, LENS), "(ln)")  # the cross product overflows
        tiny = dict(position=(0.0, 0.0, 0.0), topleft=(d["topleft"] - d["position"]) * 1e-300,  # dplane about 5e-301
                    right=d["right"], down=d["down"])
        _refused(lambda: call(tiny, (0.1, 1e300)), " s ")
    _refused(lambda: abi.lens_rays(cam, LENS, SEED, 0, H, *one), "width and height")
    _refused(lambda: abi.lens_rays(cam, LENS, SEED, W, H, np.array([W], np.int32), one[1], one[2]), "outside the film")
    lib = abi.load_library()
    p, ln = abi.pinhole_struct(cam), abi.lens_struct(LENS)
    out = np.zeros(7)
    assert lib.mfx_lens_derive(None, C.byref(ln), abi.dptr(out)) == -1 and b"null" in lib.mfx_last_error()
    assert lib.mfx_lens_derive(C.byref(p), None, abi.dptr(out)) == -1
    assert lib.mfx_lens_rays(C.byref(p), C.byref(ln), 1, W, H, -1, None, None, None, None, None) == -1
    assert lib.mfx_lens_rays(C.byref(p), C.byref(ln), 1, W, H, 1, None, None, None, None, None) == -1
