"""The sky's rule on the CPU (no GPU): the Python statement of the texel rule against the C function the kernels
share their code with; the restatement with the miss term (tests/env_helpers.py) pinned to the oracle where
the sky is black; the test inputs reach the miss term at every iteration; the furnace's closed form; and the
lat-long resampler's orientation."""
import math

import numpy as np

from conftest import SEED, scene
from env_helpers import (FURNACE_H, FURNACE_SPP, FURNACE_W, distinct_map, furnace_check, furnace_scene,
                         reference_paths)
from lights_helpers import film_paths, frame_of
from mafrixraytracing_amd import environment
from mafrixraytracing_amd.abi import MfxError, env_texel_index

SIZES = (1, 2, 5, 64, 4096)


def _special_directions():
    r = math.sqrt(0.5)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    edges = [(sx * r, sy * r, 0.0) for sx in (1, -1) for sy in (1, -1)]
    edges += [(sx * r, 0.0, sz * r) for sx in (1, -1) for sz in (1, -1)]
    edges += [(0.0, sy * r, sz * r) for sy in (1, -1) for sz in (1, -1)]
    assert len(edges) == 12
    zero_y = [(x, y, z) for y in (0.0, -0.0) for (x, z) in ((1.0, 0.0), (-1.0, 0.0), (0.6, 0.8), (-0.6, -0.8), (r, -r), (0.0, -1.0))]
    tiny = []
    for t in (1e-300, -1e-300):
        tiny += [(t, 1.0, 0.0), (t, -1.0, 0.0), (0.0, t, 1.0), (1.0, t, 0.0), (-r, t, r), (0.0, 1.0, t), (0.0, -1.0, t),
                 (t, -r, -r), (r, -r, t)]
    return np.array(axes + edges + zero_y + tiny, dtype=np.float64)


def test_python_statement_equals_the_c_function():
    rng = np.random.default_rng(20261021)
    d = rng.standard_normal((20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.concatenate([d, _special_directions()])
    for size in SIZES:
        got = env_texel_index(d, size)
        want = np.array([environment.texel_index(v, size) for v in d], dtype=np.uint32)
        assert np.array_equal(got, want), (size, int((got != want).sum()))
        assert int(got.max()) < size * size
        if size >= 5:  # the directions spread over the map (both halves, all four quadrants)
            assert len(np.unique(got)) > min(size * size, len(d)) // 2
    # dy = -0.0 takes the upper half's branch, a tiny negative dy the lower half's
    assert environment.texel_index((0.6, -0.0, 0.8), 64) == environment.texel_index((0.6, 0.0, 0.8), 64)


def test_size_refusal():
    for size in (0, -1, 4097):
        try:
            env_texel_index(np.array([[0.0, 1.0, 0.0]]), size)
        except MfxError as e:
            assert "size" in str(e)
        else:
            raise AssertionError(f"size {size} was accepted")


def test_texel_direction_round_trips():
    for size in (5, 64):
        d = environment.texel_direction(size)
        assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-15)
        ids = env_texel_index(d.reshape(-1, 3), size)
        assert np.array_equal(ids, np.arange(size * size, dtype=np.uint32))
        assert all(environment.texel_index(v, size) == k for k, v in enumerate(d.reshape(-1, 3)))


def _restated(name, w, h, spp, depth, env):
    a = scene(name, w, h, max_depth=depth)
    px, py, smp = film_paths(w, h, spp)
    info = {}
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, depth, env=env, info=info)
    return a, rad, counts, info


def test_restatement_is_the_oracle_under_a_black_sky(oracle):
    w, h, spp = 16, 12, 2
    a = scene("cornell", w, h)
    ref, st = oracle.OracleScene(a).sample(spp, SEED, with_stats=True)
    for env in (None, np.zeros((5, 5, 3), dtype=np.float32)):
        _, rad, counts, _ = _restated("cornell", w, h, spp, 3, env)
        assert np.array_equal(frame_of(rad, w, h, spp), ref)
        assert tuple(counts) == tuple(st[:3])


def test_the_inputs_reach_the_miss_term(oracle):
    """Misses per iteration as this loop counts them: spot 24 x 20 x 2 at depth 3 has 356 / 485 / 74 / 30,
    cornell 16 x 12 x 2 at depth 6 has 103 / 78 / 31 / 24 / 18 / 15 / 6 (spot at depth 6 has none at
    iteration 6, so the deep GPU test uses cornell)."""
    env = distinct_map()
    deep = 0
    for name, w, h, depth in (("spot", 24, 20, 3), ("cornell", 16, 12, 6)):
        _, rad, _, info = _restated(name, w, h, 2, depth, env)
        _, black, _, _ = _restated(name, w, h, 2, depth, None)
        print(name, depth, "misses per iteration", info["misses"], "unlit paths missing after >= 2 vertices", info["unlit_deep"])
        assert len(info["misses"]) == depth + 1 and all(m >= 1 for m in info["misses"]), info["misses"]
        deep += info["unlit_deep"]
        # every path that missed carries the sky, every other path is as without
        missed = info["miss_nv"] >= 0
        assert np.array_equal(rad[~missed], black[~missed])
        assert np.all(np.any(rad[missed] != black[missed], axis=1))
    assert deep >= 1


def test_furnace_closed_form(oracle):
    a = furnace_scene()
    px, py, smp = film_paths(FURNACE_W, FURNACE_H, FURNACE_SPP)
    info = {}
    rad, counts = reference_paths(a, [a.light], SEED, px, py, smp, 1, env=environment.constant((1.0, 1.0, 1.0)), info=info)
    K = FURNACE_W * FURNACE_H * FURNACE_SPP
    assert info["misses"] == [0, K] and tuple(counts) == (K, K, K)  # every camera ray hits the floor, every bounce leaves
    mean, bound = furnace_check(frame_of(rad, FURNACE_W, FURNACE_H, FURNACE_SPP))
    print("furnace mean", mean, "bound", bound)
    assert np.all(np.abs(mean - np.array((0.2, 0.5, 0.8))) <= bound)


def test_from_latlong_orientation():
    flat = environment.from_latlong(np.full((8, 16, 3), 0.25), 16)
    assert flat.shape == (16, 16, 3) and flat.dtype == np.float32 and np.all(flat == np.float32(0.25))
    img = np.zeros((32, 64, 3))
    img[:16] = 1.0  # above the horizon
    for size in (5, 16, 64):
        m = environment.from_latlong(img, size)
        up = environment.texel_direction(size)[..., 1] > 0.0
        assert np.array_equal(m[..., 0] == 1.0, up) and np.all((m == 0.0) | (m == 1.0))
    assert environment.constant((1, 2, 3)).shape == (1, 1, 3)
    g = environment.gradient(8, (0.1, 0.2, 1.0), (0.8, 0.8, 0.8), (0.1, 0.1, 0.1))
    assert g.shape == (8, 8, 3) and g.dtype == np.float32 and np.all(g >= 0.0) and np.all(np.isfinite(g))
