"""The chain scenes of tests/deep_helpers.py on the host (no GPU): the traversal-stack bounds they are
built for, from the host builder (mfx_build_leaves / mfx_build_instanced_info), and on the oracle alone
that their rays and films reach what tests/test_gpu_stack_shapes.py compares on them.

The bounds are ranges, so that a change to the builder that keeps the scenes deep does not break this
file; the values at the time of writing are in the comments. The bundled scenes stop at 44 (C4) and
tests/test_instancing.py holds the one instanced scene to <= 48: everything here lies beyond that."""
import numpy as np
import pytest

from deep_helpers import (DEEPEST, FLAT51, K_LARGE, M_RAYS, REFUSED, STACK_MAX, SWEEP, TWO67, TWO76, TWO80, chain_index,
                          chain_instanced, chain_shape, deep_scene, image_answer, query_answer, query_rays, stack_bound)


def test_flat_chain_bound():
    assert 48 <= stack_bound(deep_scene(FLAT51)) <= 60  # 51


@pytest.mark.parametrize("key", [TWO67, TWO76, TWO80], ids=["67", "76", "80"])
def test_two_level_chain_bounds(key):
    """The two mid scenes of the sweep (67 and 81) and the 40,000-primitive one between (75), each well
    past its template's own bound: the sum over the two levels is what makes them deep."""
    from mafrixraytracing_amd.abi import SceneArrays, build_leaves
    a = deep_scene(key)
    b = stack_bound(a)
    assert 60 <= b <= 85, b
    assert len(a.prims) == key[0] * key[3]
    template = build_leaves(SceneArrays(a.instancing[0], a.albedo, a.light, a.camera, a.width, a.height))[3]["stack"]
    assert b >= template + 15, (b, template)


def test_deepest_accepted_and_refused_bounds(monkeypatch):
    monkeypatch.setenv("MFX_LEAF_MAX", "1")
    a, r = deep_scene(DEEPEST), deep_scene(REFUSED)
    assert 90 <= stack_bound(a) <= STACK_MAX  # 93
    assert stack_bound(r) > STACK_MAX  # 97
    assert len(a.prims) == 80000 and len(r.prims) < 200000


def test_leaf_max_deepens_the_tree(monkeypatch):
    a = deep_scene(DEEPEST)
    b4 = stack_bound(a)
    monkeypatch.setenv("MFX_LEAF_MAX", "1")
    assert stack_bound(a) > b4


@pytest.mark.parametrize("m", [64, 65])
def test_instance_count_scenes(m):
    from mafrixraytracing_amd.abi import MFX_F_TWO_LEVEL, build_instanced_info
    a = chain_instanced(40, 0.7, 0.1, m, 0.85, spheres=True)
    info = build_instanced_info(a, MFX_F_TWO_LEVEL)
    assert info["instances"] == m and info["templates"] == 1 and info["template_slots"] == 40
    assert (a.instancing[0]["kind"] == 2).sum() == 10


def test_chain_shape_read_back():
    for key in SWEEP:
        n, r, rel, off = chain_shape(deep_scene(key))
        assert n == key[0] and abs(r - key[1]) < 1e-12 and abs(rel - key[2]) < 1e-12
        assert len(off) == (key[3] if len(key) == 5 else 1)


@pytest.mark.parametrize("key", SWEEP, ids=["51", "67", "80"])
def test_through_rays_reach_the_large_end(oracle, key):
    """At least 5 % of the query rays hit, and at least 20 % of those aimed through the dense end hit a
    primitive of the large end (k < 20): they popped what the dense end pushed."""
    a = deep_scene(key)
    rays, tmax = query_rays(key)
    assert rays.shape == (M_RAYS, 6) and np.allclose(np.linalg.norm(rays[:, 3:], axis=1), 1.0, atol=1e-12)
    (t, prim, nrm), occ = query_answer(oracle, key)
    h = M_RAYS // 2
    assert (prim >= 0).mean() >= 0.05
    assert ((prim[:h] >= 0) & (chain_index(a, prim[:h]) < K_LARGE)).mean() >= 0.20
    assert 0.02 < occ.mean() < 0.98
    n, r, rel, off = chain_shape(a)
    assert (rays[:h, 0] - off[:, 0].max() < 0).all()  # the aimed rays start outside the chain, on its small side


@pytest.mark.parametrize("key", SWEEP, ids=["51", "67", "80"])
def test_films_see_the_chain(oracle, key):
    ref, st = image_answer(oracle, deep_scene(key), name=key)
    assert (ref[:, :3].sum(1) != 0).mean() > 0.05 and st[1] > 0 and st[2] > 0
