"""mfx_build_scene refuses what its builders cannot hold, before either BVH is built and before anything
reaches a GPU: NaN and +-inf in whatever a primitive's kind reads, in the light and in the create-time
camera, and extents past 2^126 (DESIGN.md §3 "Coordinate range"). Through abi.build_leaves, the host
build every context creation starts with; scene_digest's error lines pin the same texts and their order
under the sanitizers."""
import numpy as np
import pytest

from range_helpers import similar
from soup_helpers import soup_case

NAN, INF = float("nan"), float("inf")


def _soup():
    from mafrixraytracing_amd.abi import SceneArrays
    a = soup_case(777, 40000, 0, True)
    return SceneArrays(a.prims.copy(), a.albedo, dict(a.light), dict(a.camera), a.width, a.height, a.max_depth)


def _first(a, kind):
    return int(np.flatnonzero(a.prims["kind"] == kind)[0])


def _refused(a, text):
    from mafrixraytracing_amd.abi import MfxError, build_leaves
    with pytest.raises(MfxError) as e:
        build_leaves(a)
    assert "(-1)" in str(e.value) and text in str(e.value), str(e.value)


@pytest.mark.parametrize("value", [NAN, INF, -INF])
def test_non_finite_primitive_values_are_refused(value):
    a = _soup()
    t, r, s = _first(a, 0), _first(a, 1), _first(a, 2)
    for i, corner in ((t, 2), (r, 3)):
        b = _soup()
        b.prims["p"][i, corner, 1] = value
        _refused(b, f"primitive {i}: corner {corner} is not finite")
    b = _soup()
    b.prims["p"][s, 0, 2] = value
    _refused(b, f"primitive {s}: centre is not finite")
    b = _soup()
    b.prims["p"][s, 1, 0] = value
    _refused(b, f"primitive {s}: radius is not finite")


def test_the_first_offender_is_named_and_unread_values_are_not_looked_at():
    from mafrixraytracing_amd.abi import build_leaves
    a = _soup()
    t, s = _first(a, 0), _first(a, 2)
    want = build_leaves(a)
    a.prims["p"][t, 3] = NAN      # a triangle reads three corners
    a.prims["p"][s, 1, 1:] = INF  # a sphere its centre and p[1][0]
    a.prims["p"][s, 2:] = NAN
    got = build_leaves(a)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3]
    a.prims["p"][700, 0, 0] = NAN
    a.prims["p"][300, 0, 1] = INF
    what = "centre" if a.prims["kind"][300] == 2 else "corner 0"
    _refused(a, f"primitive 300: {what} is not finite")
    a.prims["material"][5] = -1  # an earlier primitive's material comes first, a later one's does not
    _refused(a, "primitive 5 has material index out of range")
    a.prims["material"][5] = 0
    a.prims["material"][301] = -1
    _refused(a, f"primitive 300: {what} is not finite")


@pytest.mark.parametrize("where,key,text", [("light", "p", "light corner 2"), ("light", "normal", "light normal"),
                                            ("light", "intensity", "light intensity"),
                                            ("camera", "position", "camera position"),
                                            ("camera", "direction", "camera direction")])
@pytest.mark.parametrize("value", [NAN, INF])
def test_non_finite_light_and_camera_are_refused(where, key, text, value):
    a = _soup()
    d = getattr(a, where)
    v = np.array(d[key], dtype=np.float64)
    v[(2, 1) if key == "p" else 1] = value
    d[key] = v.tolist()
    _refused(a, text + " is not finite")


@pytest.mark.parametrize("key", ["fov", "aspect"])
def test_non_finite_fov_and_aspect_are_refused(key):
    a = _soup()
    a.camera[key] = NAN
    _refused(a, f"camera {key} is not finite")


def test_primitives_come_before_the_light_and_the_light_before_the_camera():
    a = _soup()
    a.camera["position"] = [0.0, INF, 0.0]
    a.light["intensity"] = [1.0, 1.0, NAN]
    _refused(a, "light intensity is not finite")
    a.prims["p"][776, 0, 0] = NAN
    _refused(a, "primitive 776")


def test_extent_bound():
    """R + T <= 2^126 = 8.5e37: the 777 soup builds at s = 1e30 and at 1e36 and is refused at 1e38, as it is
    1e38 away (R alone is past the bound); the tree at 1e30 is the tree at 3e19 (SAH areas all +inf:
    positional splits) with fewer nodes than at unit scale."""
    from mafrixraytracing_amd.abi import build_leaves
    a = soup_case(777, 40000, 0, False)
    zero = (0.0, 0.0, 0.0)
    i30 = build_leaves(similar(a, 1e30, zero))[3]
    i19 = build_leaves(similar(a, 3e19, zero))[3]
    i1 = build_leaves(a)[3]
    assert i30 == i19 and i30["clusters"] == i1["clusters"] and i30["slots"] == i1["slots"]
    assert i30["nodes"] < i1["nodes"]
    i18 = build_leaves(similar(a, 1e18, zero))[3]  # areas finite, their products with the weights not all
    assert i18["clusters"] == i1["clusters"] and i18["slots"] == i1["slots"]
    build_leaves(similar(a, 1e36, zero))
    _refused(similar(a, 1e38, zero), "scene extent too large")
    _refused(similar(a, 1.0, (1e38, 0.0, 0.0)), "scene extent too large")
