"""Adaptive sampling, host side (no GPU): the numpy statement of the rule
(mafrixraytracing_amd/adaptive.py) reproduces the tile counts recorded for the CPU oracle
(tests/golden/adaptive_tile_spp.json), the mfx_adaptive struct has the header's layout, and the entry
point refuses a NULL context without a device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SEED, scene

HEADER = os.path.join(ROOT, "include", "mafrix_rt.h")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "adaptive_tile_spp.json")))["cases"]

_frames = {}


def oracle_frames(oracle, name, w, h, nsamples):
    """One-sample oracle images of global samples 0 .. nsamples - 1, computed once per scene."""
    key = (name, w, h)
    have = _frames.get(key)
    if have is None or len(have) < nsamples:
        o = oracle.OracleScene(scene(name, w, h))
        have = np.stack([o.sample(1, SEED, sample_base=s) for s in range(nsamples)])
        have.setflags(write=False)
        _frames[key] = have
    return have[:nsamples]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['scene']}-{c['min_spp']}-{c['step_spp']}-{c['max_spp']}")
def test_reference_reproduces_recorded_counts(oracle, case):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, luminance, reference_mean, reference_tile_spp, tile_pixels
    w, h = case["w"], case["h"]
    cfg = AdaptiveConfig(case["min_spp"], case["max_spp"], case["step_spp"], case["rel_error"], case["abs_floor"])
    frames = oracle_frames(oracle, case["scene"], w, h, 32)[:cfg.max_spp]
    spp, gap = reference_tile_spp(luminance(frames), w, h, cfg)
    print("smallest gap", case["scene"], gap)
    assert spp.tolist() == case["tile_spp"]
    assert gap > 1e-6
    # the schedule: every count is min + k * step, or the clipped max
    for n in spp.ravel():
        assert n == cfg.max_spp or (n - cfg.min_spp) % cfg.step_spp == 0
    # a tile at a uniform count is the oracle's own Sample(n) of those pixels
    mean = reference_mean(frames, spp, w, h)
    assert np.array_equal(mean[:, 3], np.ones(w * h))
    o = oracle.OracleScene(scene(case["scene"], w, h))
    for n in sorted(set(spp.ravel().tolist()))[:2]:
        ref = o.sample(int(n), SEED)
        for ty, tx in zip(*np.nonzero(spp == n)):
            p = tile_pixels(w, h, tx, ty)
            assert np.array_equal(mean[p], ref[p]), (n, ty, tx)


def test_reference_rule_by_hand():
    """One 3x2 film (one tile, m = 6) with known moments: the two sides as the rule states them."""
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, check_sides, reference_tile_spp
    cfg = AdaptiveConfig(2, 4, 2, 0.5, 0.0)
    Y = np.array([[1.0, 1, 1, 1, 1, 1], [3.0, 1, 1, 1, 1, 1], [1.0, 1, 1, 1, 1, 1], [3.0, 1, 1, 1, 1, 1]])
    # n = 2: pixel 0 has S1 = 4, S2 = 10, v = (10 - 8) / 2 = 1; the others v = 0, mean 1
    lhs, rhs = check_sides(Y[:2].sum(0), (Y[:2] ** 2).sum(0), 2, cfg)
    assert lhs == 1.0 * 6 and rhs == 0.25 * (2.0 + 5.0) ** 2
    spp, gap = reference_tile_spp(Y, 3, 2, cfg)
    assert spp.tolist() == [[2]] and gap == (rhs - lhs) / rhs
    # a tighter threshold goes on to max_spp; an all-black film stops at min_spp with no gap recorded
    assert reference_tile_spp(Y, 3, 2, AdaptiveConfig(2, 4, 2, 0.1, 0.0))[0].tolist() == [[4]]
    spp0, gap0 = reference_tile_spp(np.zeros((4, 6)), 3, 2, cfg)
    assert spp0.tolist() == [[2]] and gap0 == float("inf")
    with pytest.raises(ValueError):
        AdaptiveConfig(1, 4, 2, 0.5, 0.0)


def test_adaptive_struct_layout_matches_header(tmp_path):
    """mfx_adaptive is 32 bytes and its ctypes field offsets are gcc's for the header."""
    from mafrixraytracing_amd.abi import MfxAdaptive
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(mfx_adaptive));']
    for f in MfxAdaptive._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(mfx_adaptive, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    lay = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert lay["size"] == 32 == C.sizeof(MfxAdaptive)
    for f in MfxAdaptive._fields_:
        assert lay[f[0]] == getattr(MfxAdaptive, f[0]).offset, f[0]
    assert len(lay) == 1 + len(MfxAdaptive._fields_) == 7


def test_null_context_is_invalid_without_a_device():
    from mafrixraytracing_amd.abi import MfxAdaptive, load_library
    lib = load_library()
    cfg = MfxAdaptive(min_spp=4, max_spp=8, step_spp=4, reserved=0, rel_error=0.1, abs_floor=0.01)
    assert lib.mfx_sample_adaptive(None, C.byref(cfg), None, None, None) == -1
    assert b"null" in lib.mfx_last_error()
