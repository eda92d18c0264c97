"""What the GPU tests of path depth, seed and sample index (tests/test_gpu_path_depth.py,
tests/test_gpu_rng_keys.py) rely on, shown on the CPU oracle alone: the inputs they choose tell a
wrong kernel from a right one.

Depth: a path's 16th vertex (max_depth 15) must change pixels, or depth 15 could not be told from
depth 14; extension rays must grow with the depth, or the later iterations would run empty. Seed and
sample index: the key is stated here a second time in Python ints, every seed under
test gives an image of its own, and the sample index enters modulo 2^32.
"""
import numpy as np
import pytest

from conftest import SEED, scene

W, H, SPP = 40, 24, 3
M64 = (1 << 64) - 1
SEEDS = [0, SEED | 1 << 32, SEED | 1 << 63, 2 ** 64 - 1]  # beside SEED itself (31 significant bits)
SAMPLES = [0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5]

_runs = {}


def run(oracle, name, depth, w=W, h=H, spp=SPP, seed=SEED):
    key = (name, depth, w, h, spp, seed)
    if key not in _runs:
        img, st = oracle.OracleScene(scene(name, w, h, max_depth=depth)).sample(spp, seed, with_stats=True)
        img.setflags(write=False)
        _runs[key] = (img, st[:3].copy())
    return _runs[key]


# pixels that must differ between max_depth 14 and 15 (measured on the oracle: 131, 162 and 4)
@pytest.mark.parametrize("name,need", [("cornell", 50), ("cube_cornell", 50), ("spot16_instanced", 1)])
def test_depth_15_is_visible_and_rays_grow(oracle, name, need):
    ext = [run(oracle, name, d)[1][1] for d in (5, 6, 14, 15)]
    assert all(a < b for a, b in zip(ext, ext[1:])), ext
    i14, i15 = run(oracle, name, 14)[0], run(oracle, name, 15)[0]
    differ = int(np.any(i14 != i15, axis=1).sum())
    print(name, "extension rays at depths 5, 6, 14, 15:", ext, "pixels differing 14 vs 15:", differ)
    assert differ >= need, differ


def test_two_spheres_plane_is_no_depth_15_witness(oracle):
    """An open scene: no path of this film reaches a lit 16th vertex, so it is not used at depth."""
    assert np.array_equal(run(oracle, "two_spheres_plane", 14)[0], run(oracle, "two_spheres_plane", 15)[0])


@pytest.mark.parametrize("name", ["cornell", "cube_cornell", "spot16_instanced"])
def test_depth_0_is_direct_light_only(oracle, name):
    img, st = run(oracle, name, 0)
    assert st[0] == W * H * SPP and st[1] == 0 and st[2] > 0, st
    assert img[:, :3].max() > 0


# ---- the key, a second time ----
def mix64(z):
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9 & M64
    z = (z ^ (z >> 27)) * 0x94d049bb133111eb & M64
    return z ^ (z >> 31)


def path_key(seed, pixel, sample):
    return mix64(seed ^ mix64(((pixel << 32) & M64) | (sample & 0xffffffff)))


def draws(seed, pixel, sample, n):
    key = path_key(seed, pixel, sample)
    return [float(mix64((key + k * 0x9e3779b97f4a7c15) & M64) >> 11) * (1.0 / 9007199254740992.0) for k in range(1, n + 1)]


def test_rng_key_restated_in_python(oracle):
    pixels = [0, 959, (1 << 21) + 12345]
    for seed in [SEED] + SEEDS:
        for smp in SAMPLES:
            for p in pixels:
                got = oracle.rng_draws(seed, p, smp, 6)
                assert got.tolist() == draws(seed, p, smp, 6), (hex(seed), smp, p)
                assert np.all((got >= 0.0) & (got < 1.0))


def test_sample_index_enters_modulo_2_32(oracle):
    for seed in [SEED] + SEEDS:
        for k in (0, 1, 5, 2 ** 31):
            assert np.array_equal(oracle.rng_draws(seed, 77, 2 ** 32 + k, 8), oracle.rng_draws(seed, 77, k, 8))
        # and nothing shorter: 2^31 apart is another stream
        assert not np.array_equal(oracle.rng_draws(seed, 77, 2 ** 31 + 3, 8), oracle.rng_draws(seed, 77, 3, 8))
    o = oracle.OracleScene(scene("cornell", 24, 16))
    assert np.array_equal(o.sample(2, SEED, sample_base=2 ** 32 + 1), o.sample(2, SEED, sample_base=1))
    assert not np.array_equal(o.sample(2, SEED, sample_base=2 ** 31 + 1), o.sample(2, SEED, sample_base=1))


def test_every_seed_under_test_has_its_own_image(oracle):
    """A key site that dropped the seed's upper half would render SEED's image (or seed 0's, or
    0xffffffff's): none of those is the image of a seed under test."""
    imgs = {s: run(oracle, "cornell", 3, 24, 16, 2, s)[0] for s in [SEED] + SEEDS + [SEED & 0xffffffff, 0xffffffff]}
    for s in SEEDS:
        assert not np.array_equal(imgs[s], imgs[SEED]), hex(s)
        if s >> 32:
            assert not np.array_equal(imgs[s], imgs[s & 0xffffffff]), hex(s)
    assert np.array_equal(imgs[SEED], imgs[SEED & 0xffffffff])  # SEED has no upper half
