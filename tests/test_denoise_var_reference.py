"""The variance-guided denoiser, host side (no GPU): known answers of the numpy statement of the rule
(mafrixraytracing_amd/denoise.py, reference_denoise_var), its agreement with a per-pixel scalar
statement, what the variance term buys over the feature-only filter against the CPU oracle's converged
image, and the C layout of mfx_denoise_var_cfg."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from denoise_helpers import oracle_features, oracle_frame, smallest_with_a_square
from denoise_var_helpers import mean_and_moments, oracle_sample_frames, scalar_denoise_var

HEADER = os.path.join(ROOT, "include", "mafrix_rt.h")
NO_FEATURES = dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)


def _features(rng, n):
    f = rng.uniform(-1.0, 1.0, (n, 8))
    f[:, 3] = rng.uniform(0.5, 9.0, n)
    return f


def _inputs(w, h, seed=3):
    """Random features with some all-zero pixels (misses), random colour, random variance >= 0 with
    some exact zeros."""
    rng = np.random.default_rng(seed)
    f = _features(rng, w * h)
    f[rng.integers(0, w * h, 6)] = 0.0
    color = rng.uniform(0.0, 2.0, (w * h, 4))
    var = rng.uniform(0.0, 0.05, w * h)
    var[rng.integers(0, w * h, 5)] = 0.0
    return color, var, f


def test_defaults():
    from mafrixraytracing_amd.denoise import DenoiseVarConfig
    d = DenoiseVarConfig()
    assert (d.iterations, d.sigma_normal, d.sigma_depth, d.sigma_albedo, d.sigma_luma, d.luma_floor) == \
        (3, 0.1, 0.02, 0.05, 4.0, 1e-6)
    for bad in (dict(iterations=0), dict(iterations=9), dict(sigma_normal=-1.0), dict(sigma_luma=float("nan")),
                dict(sigma_luma=-0.5), dict(sigma_depth=float("inf")), dict(luma_floor=0.0), dict(luma_floor=-1e-6),
                dict(luma_floor=float("nan")), dict(luma_floor=float("inf"))):
        with pytest.raises(ValueError):
            DenoiseVarConfig(**bad)


def test_sigmas_whose_square_is_zero_are_refused():
    """sigma_normal, sigma_depth or sigma_albedo > 0 with a square of 0 in FP64 would make the centre tap's
    term 0/0: ValueError, as the library's MFX_E_INVALID. sigma_luma needs no such rule: its square is
    added to luma_floor > 0."""
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var
    s_min, s_below = smallest_with_a_square()
    w, h = 7, 5
    color, var, f = _inputs(w, h)
    for name in ("sigma_normal", "sigma_depth", "sigma_albedo"):
        for bad in (1e-163, 1e-170, 5e-324, s_below):
            with pytest.raises(ValueError):
                DenoiseVarConfig(**{name: bad})
        out, v = reference_denoise_var(color, var, f, w, h, DenoiseVarConfig(**{name: s_min}))
        assert np.isfinite(out).all() and np.isfinite(v).all(), name
    for luma in (1e-170, 5e-324, s_below):
        out, v = reference_denoise_var(color, var, f, w, h, DenoiseVarConfig(sigma_luma=luma))
        assert np.isfinite(out).all() and np.isfinite(v).all(), luma


def test_variance_of_mean():
    """d = S2 - (S1*S1)/n, clamped at +0.0, over n (n - 1); n a number or per pixel."""
    from mafrixraytracing_amd.denoise import variance_of_mean
    S1 = np.array([3.0, 2.0, 0.0, 1.0])
    S2 = np.array([5.0, 1.0, 0.0, 0.5])  # samples {1, 2}: d = 0.5; d = -1 -> 0; black; n = 4 below
    got = variance_of_mean(S1, S2, np.array([2, 2, 2, 4]))
    assert got.tolist() == [(5.0 - 9.0 / 2.0) / 2.0, 0.0, 0.0, (0.5 - 1.0 / 4.0) / 12.0]
    assert not np.signbit(got).any()
    assert variance_of_mean(S1[:1], S2[:1], 2).tolist() == [0.25]


def test_cfg_layout_matches_header(tmp_path):
    """mfx_denoise_var_cfg is 56 bytes and its ctypes field offsets are gcc's for the header."""
    from mafrixraytracing_amd.abi import MFX_DN_SRC_ADAPTIVE, MfxDenoiseVarCfg
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(mfx_denoise_var_cfg));', 'printf("adaptive %d\\n", MFX_DN_SRC_ADAPTIVE);']
    for f in MfxDenoiseVarCfg._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(mfx_denoise_var_cfg, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    lay = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert lay["size"] == 56 == C.sizeof(MfxDenoiseVarCfg)
    assert lay["adaptive"] == 2 == MFX_DN_SRC_ADAPTIVE
    for f in MfxDenoiseVarCfg._fields_:
        assert lay[f[0]] == getattr(MfxDenoiseVarCfg, f[0]).offset, f[0]
    assert len(lay) == 2 + len(MfxDenoiseVarCfg._fields_) == 10
    assert [lay[k] for k in ("iterations", "source", "reserved", "sigma_normal", "sigma_luma", "luma_floor")] == \
        [0, 4, 8, 16, 40, 48]


def test_null_context_is_invalid_without_a_device():
    from mafrixraytracing_amd.abi import MfxDenoiseVarCfg, load_library
    lib = load_library()
    cfg = MfxDenoiseVarCfg(iterations=3, source=2, sigma_normal=0.1, sigma_luma=4.0, luma_floor=1e-6)
    assert lib.mfx_denoise_var(None, C.byref(cfg), None, None, None, None, None, None) == -1
    assert b"mfx_denoise_var" in lib.mfx_last_error()


@pytest.mark.parametrize("kw", [dict(), dict(iterations=4), dict(sigma_luma=0.0), NO_FEATURES])
def test_numpy_statement_equals_scalar_statement(kw):
    """Step 8 reaches past every edge of a 7x5 film; some pixels are misses, some variances exact zeros."""
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var
    w, h = 7, 5
    color, var, f = _inputs(w, h)
    cfg = DenoiseVarConfig(**kw)
    got, gv = reference_denoise_var(color, var, f, w, h, cfg)
    ref, rv = scalar_denoise_var(color, var, f, w, h, cfg)
    assert got.shape == (w * h, 4) and gv.shape == (w * h,)
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    assert np.array_equal(gv, rv), np.abs(gv - rv).max()
    assert (gv >= 0).all() and np.isfinite(gv).all()


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_sigma_luma_zero_is_the_feature_filter(iterations):
    """With the luminance term off the colour is reference_denoise's with sigma_color = 0, to the bit; the
    variance is still propagated."""
    from mafrixraytracing_amd.denoise import DenoiseConfig, DenoiseVarConfig, reference_denoise, reference_denoise_var
    w, h = 11, 7
    color, var, f = _inputs(w, h, seed=4)
    got, gv = reference_denoise_var(color, var, f, w, h, DenoiseVarConfig(iterations=iterations, sigma_luma=0.0))
    assert np.array_equal(got, reference_denoise(color, f, w, h, DenoiseConfig(iterations=iterations, sigma_color=0.0)))
    assert not np.array_equal(gv, var) and (gv >= 0).all()


def test_constant_image_stays_constant():
    """wt * 0.5 is exact, so num = 0.5 * den to the bit whatever the weights are; dl is 0 everywhere."""
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var
    w, h = 11, 7
    rng = np.random.default_rng(1)
    color = np.full((w * h, 4), 0.5)
    color[:, 1] = 2.0
    color[:, 2] = 0.0
    var = rng.uniform(0.0, 1.0, w * h)
    out, _ = reference_denoise_var(color, var, _features(rng, w * h), w, h, DenoiseVarConfig(iterations=4))
    assert np.array_equal(out[:, 0], np.full(w * h, 0.5))
    assert np.array_equal(out[:, 1], np.full(w * h, 2.0))
    assert np.array_equal(out[:, 2], np.zeros(w * h))
    assert np.array_equal(out[:, 3], np.ones(w * h))


def test_one_pixel_film():
    """The only tap is the centre: g = 1, wt = 9/64; V' = (wt*wt * V) / (wt*wt)."""
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var
    c = np.array([[0.3, 0.7, 1.9, 5.0]])
    out, v = reference_denoise_var(c, np.array([0.37]), np.zeros((1, 8)), 1, 1, DenoiseVarConfig(iterations=1))
    k = 9.0 / 64.0
    assert out.tolist() == [[(k * 0.3) / k, (k * 0.7) / k, (k * 1.9) / k, 1.0]]
    assert v.tolist() == [((k * k) * 0.37) / (k * k)]


def test_uniform_variance_plain_filter_by_hand():
    """Every sigma 0 and V = 1 on a 9x9 film: an interior pixel takes all 25 taps with wt = k[|dx|] k[|dy|],
    den = 1 and V' = sum wt^2 = (sum k^2)^2 = (35/128)^2, every sum dyadic: exact."""
    from mafrixraytracing_amd.denoise import DenoiseVarConfig, reference_denoise_var
    w = h = 9
    rng = np.random.default_rng(5)
    cfg = DenoiseVarConfig(iterations=1, sigma_luma=0.0, **NO_FEATURES)
    _, v = reference_denoise_var(rng.uniform(0, 1, (w * h, 3)), np.ones(w * h), np.zeros((w * h, 8)), w, h, cfg)
    assert (3 / 8) ** 2 + 2 * (1 / 4) ** 2 + 2 * (1 / 16) ** 2 == 35 / 128
    assert v.reshape(w, h)[4, 4] == (35 / 128) ** 2
    assert (v.reshape(w, h)[2:7, 2:7] == (35 / 128) ** 2).all()
    # a corner keeps dx, dy = 0..2: den = (11/16)^2, vn = (sum_{0..2} k^2)^2 = (53/256)^2
    assert v.reshape(w, h)[0, 0] == (53 / 256) ** 2 / ((11 / 16) ** 2 * (11 / 16) ** 2)


_QUALITY = {}


def _quality(oracle, name, n):
    """RMSEs against the oracle's 2048-spp frame of samples 1000..3047 on a 44x36 film: the raw mean of
    samples 0..n-1, reference_denoise and reference_denoise_var of it at 3 and 5 iterations, features of
    samples 0..3, moments of the one-sample frames in sample order."""
    from mafrixraytracing_amd.denoise import (DenoiseConfig, DenoiseVarConfig, reference_denoise, reference_denoise_var,
                                              variance_of_mean)
    if (name, n) in _QUALITY:
        return _QUALITY[(name, n)]
    w, h = 44, 36
    feat = oracle_features(oracle, name, w, h, 4, 0)
    conv = oracle_frame(oracle, name, w, h, 2048, 1000)
    raw, S1, S2 = mean_and_moments(oracle_sample_frames(oracle, name, w, h, 16), n)
    var = variance_of_mean(S1, S2, n)

    def rmse(a):
        return float(np.sqrt(((a[:, :3] - conv[:, :3]) ** 2).mean()))

    r = {"raw": rmse(raw)}
    for it in (3, 5):
        r[f"feat{it}"] = rmse(reference_denoise(raw, feat, w, h, DenoiseConfig(iterations=it)))
        r[f"var{it}"] = rmse(reference_denoise_var(raw, var, feat, w, h, DenoiseVarConfig(iterations=it))[0])
    print(f"{name}, {n} spp: " + ", ".join(f"{k} {v:.5f}" for k, v in r.items()) +
          f", var3/feat3 {r['var3'] / r['feat3']:.3f}")
    _QUALITY[(name, n)] = r
    return r


@pytest.mark.parametrize("n", [8, 16])
@pytest.mark.parametrize("name", ["cornell", "two_spheres_plane", "spot"])
def test_variance_term_beats_the_feature_filter(oracle, name, n):
    """Default configs, 3 iterations: the variance-guided RMSE is strictly below the feature-only one (a
    numpy prototype measured ratios 0.905 / 0.781 / 0.860 at 8 spp and 0.788 / 0.674 / 0.793 at 16)."""
    r = _quality(oracle, name, n)
    assert r["var3"] < r["feat3"]


@pytest.mark.parametrize("name", ["cornell", "two_spheres_plane", "spot"])
def test_five_iterations_stay_below_raw_at_16_spp(oracle, name):
    """Where the feature-only filter ends worse than the raw image on two scenes, the variance-guided one
    stays below it (the prototype: 0.0070 < 0.0113, 0.0970 < 0.1481, 0.0598 < 0.0744)."""
    r = _quality(oracle, name, 16)
    assert r["var5"] < r["raw"]
