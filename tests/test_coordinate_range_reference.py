"""The conditions under which tests/test_gpu_coordinate_range.py means something, asserted on the CPU
oracle and the host build alone for exactly its cases (tests/range_helpers.py holds them): the images
are lit with shadow and bounce rays, the coordinates really lie past (or below) the binary16 range, and
the two-level case keeps its instances with the top level far out and the templates at local scale."""
import numpy as np
import pytest

from range_helpers import CASES, SPP, case_id, moved_instanced_scene, range_image, range_scene


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_range_images_are_lit(oracle, c):
    ref, st = range_image(oracle, c)
    lit = (ref[:, :3].sum(1) != 0).mean()
    print(f"{case_id(c)}: lit {lit:.3f}, camera {st[0]}, bounce {st[1]}, shadow {st[2]} rays")
    assert lit > 0.05 and st[1] > 0 and st[2] > 0
    assert np.isfinite(ref).all()


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_range_cases_leave_the_half_range(c):
    """The soup's primitives (all but the ground) have a coordinate past 65504 in magnitude: every one
    where an offset of 1e5 or 1e7 puts them, most where the offset is 65504 itself or the scale 1e5. At
    scale 1e-4 the soup fits in 1.1e-4 and a good share of its non-zero coordinates are subnormal halves
    (below 2^-14)."""
    s, off = c
    a = range_scene(c)
    first = a.prims["p"][:-1, 0]  # (the ground sphere is last)
    if s == 1e-4:
        assert np.abs(first).max() <= 1.1e-4
        assert (np.abs(first[first != 0]) < 2.0 ** -14).mean() > 0.3
    else:
        past = (np.abs(first).max(axis=1) > 65504.0).mean()
        assert past == 1.0 if max(np.abs(off)) >= 1e5 else past > 0.5, past
    assert np.isfinite(a.prims["p"]).all() and np.isfinite(np.asarray(a.light["p"])).all()


def test_moved_two_level_scene(oracle):
    """The expansion the oracle sees is the library's; the instances stay (two templates, eight uses) with
    offsets past the half range; the image is lit."""
    from conftest import SEED
    from mafrixraytracing_amd.abi import MFX_F_TWO_LEVEL, build_instanced_info
    a = moved_instanced_scene()
    info = build_instanced_info(a, MFX_F_TWO_LEVEL)
    assert info["instances"] == 8 and info["templates"] == 2, info
    T, I = a.instancing
    used = I[I["flags"] == 0]
    assert (np.abs(used["offset"]).max(axis=1) > 65504.0).all()
    tmpl = np.concatenate([T[int(e["first"]):int(e["first"]) + int(e["count"])] for e in used])
    assert np.abs(tmpl["p"]).max() < 2.0  # local scale
    assert np.abs(a.prims["p"][:, 0]).max(axis=1).min() > 65504.0  # every world primitive is far out
    ref, st = oracle.OracleScene(a).sample(SPP, SEED, with_stats=True)
    assert (ref[:, :3].sum(1) != 0).mean() > 0.05 and st[1] > 0 and st[2] > 0
