"""Several area lights (mfx_create_lights), CPU side: the restatement of the oracle's path trace with the
light pick (tests/lights_helpers.py) is pinned to the oracle with one light, the inputs of the GPU tests
are shown to be telling, and the host-side parts of the feature (derived light table, pick bound, loader,
refusals) are checked. No GPU."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import SCENES, SEED, scene
from lights_helpers import film_paths, frame_of, light_sets, reference_paths

W, H = 24, 20


# ---- 1. the restatement with one light is the oracle ---------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "cube_cornell", "spot16_instanced"])
@pytest.mark.parametrize("depth", [0, 3, 5])
def test_restatement_with_one_light_is_the_oracle(oracle, name, depth):
    a = scene(name, W, H, max_depth=depth)
    osc = oracle.OracleScene(a)
    px, py, _ = film_paths(W, H, 3)
    smp = np.tile(np.array([0, 1, 2 ** 32 + 5], dtype=np.int64), W * H)
    want, st = osc.paths(px, py, smp, SEED)
    got, counts, picks, lit = reference_paths(a, [a.light], SEED, px, py, smp, depth, oscene=osc)
    assert np.array_equal(got, want)
    assert tuple(counts) == tuple(st[:3])
    assert picks[0] == counts[2] and 0 < lit[0] <= picks[0]


# ---- 2. the light sets are telling -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_sets(oracle):
    a = scene("cornell", W, H)
    return a, oracle.OracleScene(a), light_sets(a.light)


@pytest.mark.parametrize("which", ["N2", "N5"])
def test_every_light_is_picked_and_all_but_the_turned_one_light(cornell_sets, which):
    a, osc, sets = cornell_sets
    lights = sets[which]
    px, py, smp = film_paths(W, H, 3)
    rad, counts, picks, lit = reference_paths(a, lights, SEED, px, py, smp, 3, oscene=osc)
    assert picks.sum() == counts[2] and np.all(picks > 0)
    if which == "N5":
        assert lit[4] == 0 and np.all(lit[:4] > 0)  # the turned copy is picked and never lights
    else:
        assert np.all(lit > 0)
        one, _, _, _ = reference_paths(a, [a.light], SEED, px, py, smp, 3, oscene=osc)
        differ = np.any(frame_of(rad, W, H, 3) != frame_of(one, W, H, 3), axis=1)
        assert differ.mean() > 0.5  # most pixels see the second light


def test_linearity_bound_tells_the_literal_rule_apart(oracle):
    """The GPU linearity test's inputs (tests/test_gpu_lights.py): with the reference's literal pdf (no
    division by N) the restated [A, B] image is far outside 5 standard errors of oracle(A) + oracle(B), and
    with pdf_n it is inside. Without this the GPU test would prove nothing."""
    from lights_helpers import (LIN_BATCHES, LIN_SPP, linearity_bound, linearity_inputs, linearity_oracle_means,
                                mean_luminance)
    a, A, B, w, h = linearity_inputs()
    osc = oracle.OracleScene(a)
    other = linearity_oracle_means(oracle, a, A, B)
    sides = {False: [], True: []}
    for b in range(LIN_BATCHES):
        px, py, smp = film_paths(w, h, LIN_SPP, sample_base=LIN_SPP * b)
        for literal in (False, True):
            rad, _, _, _ = reference_paths(a, [A, B], SEED, px, py, smp, 3, literal=literal, oscene=osc)
            sides[literal].append(mean_luminance(frame_of(rad, w, h, LIN_SPP)))
    diff, bound = linearity_bound(sides[False], other)
    assert diff <= bound
    diff2, bound2 = linearity_bound(sides[True], other)
    assert diff2 > 4 * bound2  # the mean of the lights' sum is far more than 5 sigma from it


# ---- 3. the derived table ---------------------------------------------------------------------------------
def test_light_table_matches_numpy_bit_for_bit():
    from mafrixraytracing_amd.abi import light_table as native_table
    from mafrixraytracing_amd.lights import light_table
    rng = np.random.default_rng(7)
    twice = 0
    for n in (1, 2, 3, 5, 7, 64):
        lights = []
        for _ in range(n):
            p0 = rng.uniform(-3, 3, 3)
            e1, e2 = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
            lights.append({"p": (p0, p0 + e1, p0 + e1 + e2, p0 + e2), "normal": (0.0, -1.0, 0.0), "intensity": (1.0, 2.0, 3.0)})
        want, got = light_table(lights), native_table(lights)
        assert want.tobytes() == got.tobytes()
        assert np.all(got[:, 3] == 0.0) and np.all(got[:, 2] == (1.0 / got[:, 0]) / n)
        for area, pdf in zip(got[:, 0], got[:, 2]):  # two divisions are not one: some pdf_n is not the rounded 1 / (N area)
            exact = Fraction(1) / (Fraction(float(area)) * n)
            twice += float(exact) != float(pdf)
    assert twice > 0
    # one light: pdf is 1 / area itself (mfx_create's value)
    one = native_table([lights[0]])
    assert one[0, 2] == one[0, 1] == 1.0 / one[0, 0]


# ---- 4. the pick needs no clamp ---------------------------------------------------------------------------
def test_pick_stays_below_n():
    from mafrixraytracing_amd.lights import MAX_LIGHTS, pick
    top = 1.0 - 2.0 ** -53  # the largest draw: k * 2^-53 with k = 2^53 - 1
    assert MAX_LIGHTS == 64
    for n in range(2, 65):
        assert np.floor(np.float64(top) * np.float64(n)) == n - 1
        assert pick(top, n) == n - 1 and pick(0.0, n) == 0
        got = [pick(r, n) for r in np.linspace(0.0, top, 64 * n)]  # non-decreasing, every light reached
        assert got == sorted(got) and set(got) == set(range(n))


# ---- 5. structs, symbols, loader --------------------------------------------------------------------------
def test_symbols_and_constants():
    from mafrixraytracing_amd import abi
    lib = abi.load_library()
    for s in ("mfx_create_lights", "mfx_light_info", "mfx_light_table"):
        assert s in abi.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert abi.MFX_MAX_LIGHTS == 64 and lib.mfx_abi_version() == 6
    hdr = open(os.path.join(os.path.dirname(SCENES), "include", "mafrix_rt.h")).read()
    assert "#define MFX_MAX_LIGHTS 64" in hdr
    assert C.sizeof(abi.MfxQuadLight) == 18 * 8


def test_all_lights_gives_document_order_and_the_default_keeps_the_last():
    import re

    from mafrixraytracing_amd.scene_io import InitSceneState, MaterialManager
    text = open(os.path.join(SCENES, "cornell.xml")).read()
    first = text[text.index("<Light"):text.index("</Light>") + len("</Light>")]
    second = re.sub(r'(name="intensity" value=")[^"]*"', r'\g<1>1,2,3"', first)
    assert second != first
    two = text.replace(first, first + "\n" + second)
    st1 = InitSceneState(two, base_dir=SCENES, manager=MaterialManager())
    assert st1.lights is None and tuple(st1.light["intensity"]) == (1.0, 2.0, 3.0)  # the last <Light> wins
    st2 = InitSceneState(two, base_dir=SCENES, manager=MaterialManager(), all_lights=True)
    assert [tuple(L["intensity"]) for L in st2.lights] == [(10.0, 10.0, 10.0), (1.0, 2.0, 3.0)]
    assert tuple(st2.light["intensity"]) == (1.0, 2.0, 3.0)
    a = st2.arrays()
    assert len(a.lights) == 2 and len(a.with_film(8, 8).lights) == 2
    assert InitSceneState(text, base_dir=SCENES, manager=MaterialManager()).arrays().lights is None


# ---- 6. refusals on the host -------------------------------------------------------------------------------
def _create_lights(a, lights, nlights=None, flags=0):
    from mafrixraytracing_amd.abi import MfxOptions, load_library, quad_lights
    lib = load_library()
    d = a.desc()
    opt = MfxOptions(seed=1, device=0, flags=flags, part_index=0, part_count=1)
    h = C.c_void_p()
    arr = quad_lights(lights) if lights is not None else None
    rc = lib.mfx_create_lights(C.byref(d), arr, len(lights) if nlights is None else nlights, None, 0, C.byref(opt), C.byref(h))
    msg = lib.mfx_last_error().decode()
    if rc == 0:
        lib.mfx_destroy(h)
    return rc, msg


def test_refusals_need_no_device():
    from mafrixraytracing_amd.abi import MFX_F_COUNT_STATS, MFX_F_MEGAKERNEL
    a = scene("cornell", 8, 8)
    L0 = a.light
    sets = light_sets(L0)
    assert _create_lights(a, [L0], nlights=0)[0] == -1
    assert _create_lights(a, [L0] * 65)[0] == -1
    assert _create_lights(a, None, nlights=2)[0] == -1
    bad = dict(L0, p=(L0["p"][0], L0["p"][1], (0.0, float("nan"), 0.0), L0["p"][3]))
    rc, msg = _create_lights(a, [L0, L0, bad])
    assert rc == -1 and "light 2" in msg and "corner 2" in msg
    rc, msg = _create_lights(a, [L0, dict(L0, intensity=(1.0, float("inf"), 1.0))])
    assert rc == -1 and "light 1" in msg and "intensity" in msg
    flat = dict(L0, p=(L0["p"][0], L0["p"][0], L0["p"][0], L0["p"][0]))
    rc, msg = _create_lights(a, [L0, flat])
    assert rc == -1 and "light 1" in msg and "area" in msg
    for f in (MFX_F_MEGAKERNEL, MFX_F_COUNT_STATS):
        rc, msg = _create_lights(a, sets["N2"], flags=f)
        assert rc == -1 and "single light" in msg
