"""Albedo textures without a GPU: the library's host code (mfx_uv_table, mfx_texel_index, the refusals of
mfx_create_textured) against the Python statement of the rule (mafrixraytracing_amd/textures.py), the
restated path trace against the one the lights tests pinned to the oracle, and the loader."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import SEED, scene
from mafrixraytracing_amd import abi, textures as tx
from mafrixraytracing_amd.abi import PRIM_DTYPE, PRIM_UV_DTYPE

MFX_E_INVALID = -1


# ---- 1. the UV table -----------------------------------------------------------------------------------
def _soup(seed=5, n=60):
    """Triangles and rects with coordinates from 1e-3 to 1e4, UVs outside [0, 1] and negative, a collinear
    and a zero-area triangle, an untextured primitive and a sphere."""
    rng = np.random.default_rng(seed)
    prims = np.zeros(n, dtype=PRIM_DTYPE)
    uv = np.zeros(n, dtype=PRIM_UV_DTYPE)
    for i in range(n):
        scale = 10.0 ** rng.uniform(-3, 4)
        c = (rng.random(3) - 0.5) * scale
        e1, e2 = (rng.random(3) - 0.5) * scale, (rng.random(3) - 0.5) * scale
        prims[i]["kind"] = i % 2
        prims[i]["p"][0], prims[i]["p"][1], prims[i]["p"][2], prims[i]["p"][3] = c, c + e1, c + e1 + e2, c + e2
        uv[i]["texture"] = i % 3
        uv[i]["uv"] = rng.uniform(-3.0, 4.0, size=(3, 2))
    prims[0]["p"][0], prims[0]["p"][1], prims[0]["p"][2] = (1, 2, 3), (2, 4, 7), (3, 6, 11)  # collinear, exactly: det == 0
    prims[2]["p"][1] = prims[2]["p"][0]                                                # zero area
    prims[2]["p"][2] = prims[2]["p"][0]
    uv[4]["texture"] = -1
    prims[6]["kind"] = 2
    uv[6]["texture"] = -1
    return prims, uv


def test_uv_table_equals_the_statement():
    prims, uv = _soup()
    got, want = abi.uv_table(prims, uv), tx.uv_table(prims, uv)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the fallback record of the degenerate ones: the first corner's (u, v)
    for i in (0, 2):
        assert tuple(got[i]) == (0.0, 0.0, 0.0, uv[i]["uv"][0][0], 0.0, 0.0, 0.0, uv[i]["uv"][0][1]), i
    assert not got[4].any() and not got[6].any()
    # the definition: the record gives the corners their own (u, v) (a sanity check, not of bits)
    for i in range(len(prims)):
        if i in (0, 2, 4, 6):
            continue
        for k in range(3):
            p = prims[i]["p"][k]
            for w, off in ((0, 0), (1, 4)):
                val = float(np.dot(p, got[i][off:off + 3]) + got[i][off + 3])
                want_w = float(uv[i]["uv"][k][w])
                assert abs(val - want_w) <= 1e-9 * (1.0 + abs(want_w)), (i, k, w, val, want_w)


# ---- 2. the texel rule -----------------------------------------------------------------------------------
COORDS = [0.0, -0.0, 1.0, -1e-17, 0.5, 1.0 - 2.0 ** -53, 2.75, -2.25, 1e15 + 0.5]
DIMS = [1, 2, 3, 5, 256]


def test_texel_index_equals_the_statement():
    uv = np.array(list(itertools.product(COORDS, COORDS)))
    for w, h in itertools.product(DIMS, DIMS):
        sizes = [(3, 7), (h, w), (2, 2)]  # three textures: the bases matter
        for t in range(3):
            got = abi.texel_index(sizes, t, uv)
            want = np.array([tx.texel_index(sizes, t, u, v) for u, v in uv], dtype=np.uint32)
            assert np.array_equal(got, want), (w, h, t)
        base = 21
        ids = abi.texel_index(sizes, 1, np.array([[0.0, 0.0], [0.0, 1.0 - 2.0 ** -53], [-1e-17, 0.0], [0.5, 0.5]]))
        assert ids[0] == base + (h - 1) * w          # v = 0: the bottom row, column 0
        assert ids[1] == base                        # v just below 1: row 0
        assert ids[2] == base + (h - 1) * w + w - 1  # u = -1e-17: tu is exactly 1.0, clamped to column W - 1
        assert ids[3] == base + ((h - 1) - (h // 2 if h > 1 else 0)) * w + (w // 2 if w > 1 else 0)
        assert ids.max() < base + w * h and ids.min() >= base


# ---- 3. the refusals ---------------------------------------------------------------------------------------
def _create(a, textures, prim_uv, flags=0, lights=True, sizes=None, null_rgba=None):
    """mfx_create_textured's return code and message. sizes: (height, width) per texture with a dummy texel
    pointer (the size refusals are decided before any texel is read)."""
    lib = abi.load_library()
    desc = a.desc()
    L = abi.quad_lights([a.light])
    if sizes is not None:
        dummy = (C.c_uint8 * 4)()
        arr = (abi.MfxTexture * max(1, len(sizes)))()
        for k, (h, w) in enumerate(sizes):
            arr[k].rgba = C.cast(dummy, C.POINTER(C.c_uint8))
            arr[k].height, arr[k].width = h, w
        n, keep = len(sizes), dummy
    else:
        arr, keep = abi.texture_structs(textures)
        n = len(textures)
        if null_rgba is not None:
            arr[null_rgba].rgba = None
    up = prim_uv.ctypes.data_as(C.POINTER(abi.MfxPrimUv)) if prim_uv is not None else None
    opt = abi.MfxOptions(seed=SEED, device=0, flags=flags, part_index=0, part_count=1)
    h = C.c_void_p()
    rc = lib.mfx_create_textured(C.byref(desc), L if lights else None, 1, None, 0, arr if n or sizes is not None else None, n,
                                 up, C.byref(opt), C.byref(h))
    assert not h.value
    del keep
    return rc, (lib.mfx_last_error() or b"").decode()


def test_refusals_are_decided_on_the_host():
    c = scene("cornell", 8, 8)
    ball = np.zeros(1, dtype=PRIM_DTYPE)
    ball["kind"], ball["p"][0][0][1], ball["p"][0][1][0] = 2, 0.5, 0.1
    a = abi.SceneArrays(np.concatenate([c.prims, ball]), c.albedo, c.light, c.camera, 8, 8)
    n = len(a.prims)
    kinds = a.prims["kind"]
    flat = int(np.flatnonzero(kinds != 2)[0])
    sphere = int(np.flatnonzero(kinds == 2)[0])
    white = [np.full((2, 2, 4), 255, np.uint8), np.full((1, 3, 4), 255, np.uint8)]

    def maps(**at):
        m = np.zeros(n, dtype=PRIM_UV_DTYPE)
        m["texture"] = -1
        for i, t in at.get("tex", {}).items():
            m[i]["texture"] = t
            m[i]["uv"] = [[0, 0], [1, 0], [1, 1]]
        return m

    ok_maps = maps(tex={flat: 1})
    cases = {
        "null prim_uv": (dict(textures=white, prim_uv=None), "prim_uv"),
        "index above": (dict(textures=white, prim_uv=maps(tex={flat: 2})), f"primitive {flat} has texture 2"),
        "index below": (dict(textures=white, prim_uv=maps(tex={flat: -2})), f"primitive {flat} has texture -2"),
        "textured sphere": (dict(textures=white, prim_uv=maps(tex={sphere: 0})), f"primitive {sphere} is a textured sphere"),
        "null rgba": (dict(textures=white, prim_uv=ok_maps, null_rgba=1), "texture 1 has a null rgba"),
        "width 0": (dict(textures=None, prim_uv=ok_maps, sizes=[(4, 4), (4, 0)]), "texture 1 is 0 x 4"),
        "height 16385": (dict(textures=None, prim_uv=ok_maps, sizes=[(16385, 4)]), "texture 0 is 4 x 16385"),
        "too many textures": (dict(textures=None, prim_uv=ok_maps, sizes=[(1, 1)] * 4097), "ntextures 4097"),
        # 8 x 16384^2 = 2^31 texels: the eighth brings the total past 2^31 - 2
        "too many texels": (dict(textures=None, prim_uv=ok_maps, sizes=[(16384, 16384)] * 8), "texture 7 brings the texels"),
        "megakernel": (dict(textures=white, prim_uv=ok_maps, flags=abi.MFX_F_MEGAKERNEL), "MFX_F_MEGAKERNEL"),
        "count stats": (dict(textures=white, prim_uv=ok_maps, flags=abi.MFX_F_COUNT_STATS), "MFX_F_COUNT_STATS"),
    }
    for name, (kw, needle) in cases.items():
        rc, msg = _create(a, **kw)
        assert rc == MFX_E_INVALID, (name, rc, msg)
        assert needle in msg and msg.startswith("mfx_create_textured:"), (name, msg)
    bad = maps(tex={flat: 0})
    bad[flat]["uv"][2][1] = np.inf
    rc, msg = _create(a, textures=white, prim_uv=bad)
    assert rc == MFX_E_INVALID and f"primitive {flat} uv of corner 2 is not finite" in msg, msg
    # an untextured primitive's uv is not looked at
    free = maps(tex={flat: 0})
    other = int(np.flatnonzero(kinds != 2)[-1])
    assert other != flat
    free[other]["uv"][0][0] = np.nan
    free[flat]["uv"][0][0] = np.nan
    rc, msg = _create(a, textures=white, prim_uv=free)
    assert f"primitive {flat} uv of corner 0" in msg, msg
    # exactly 2^31 - 2 texels pass the size rule (the next refusal is the dummy pointer's business: none here,
    # so the call goes on to the device; not run). mfx_texel_index applies the same size rule on the host:
    lib = abi.load_library()
    with pytest.raises(abi.MfxError, match="brings the texels"):
        abi.texel_index([(16384, 16384)] * 8, 0, np.zeros((1, 2)))
    ids = abi.texel_index([(16384, 16384)] * 7 + [(16384, 16382), (2, 16383)], 8, np.array([[1.0 - 2.0 ** -53, 0.0]]))
    assert int(ids[0]) == 2 ** 31 - 3  # the last texel of the largest scene the rule admits
    with pytest.raises(abi.MfxError, match="outside 0"):
        abi.texel_index([(2, 2)], 1, np.zeros((1, 2)))
    assert lib.mfx_texture_info(None, None) == MFX_E_INVALID


# ---- 4. the tie to the oracle ----------------------------------------------------------------------------
def test_restatement_equals_the_lights_restatement(oracle):
    import lights_helpers as lh
    import texture_helpers as th
    a = scene("cornell", 16, 12)
    px, py, smp = lh.film_paths(16, 12, 4)
    osc = oracle.OracleScene(a)
    want, wc, _, _ = lh.reference_paths(a, [a.light], SEED, px, py, smp, 3, oscene=osc)
    got, gc = th.reference_paths(a, [a.light], SEED, px, py, smp, 3, None, oscene=osc)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(gc, wc)
    # an all-255 texture on every triangle and rect: a factor of exactly 1.0
    maps = th.random_prim_uv(a.prims, 2, seed=3, textured=1.0)
    white = th.TexSet(a.prims, [np.full((3, 5, 4), 255, np.uint8), np.full((1, 1, 4), 255, np.uint8)], maps)
    assert (maps["texture"] >= 0).sum() >= 10
    got, gc = th.reference_paths(a, [a.light], SEED, px, py, smp, 3, white, oscene=osc)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(gc, wc)
    # and a texture that is not white changes the image (the lookup is live)
    col = th.TexSet(a.prims, [tx.procedural(0, 3, 5), tx.procedural(1, 1, 1)], maps)
    got, gc = th.reference_paths(a, [a.light], SEED, px, py, smp, 3, col, oscene=osc)
    assert not np.array_equal(got, want) and np.array_equal(gc, wc)
    # the frame against the oracle itself, as the lights restatement is pinned
    assert np.array_equal(lh.frame_of(want, 16, 12, 4), osc.sample(4, SEED))


def test_procedural_texels_are_distinct():
    for k, (h, w) in enumerate(((1, 1), (5, 3), (64, 64), (256, 256))):
        t = tx.procedural(k, h, w)
        assert t.shape == (h, w, 4) and t.dtype == np.uint8 and (t[..., 3] == 255).all()
        codes = t[..., 0].astype(np.int64) | (t[..., 1].astype(np.int64) << 8) | (t[..., 2].astype(np.int64) << 16)
        assert len(np.unique(codes)) == h * w


# ---- 5. the loader -------------------------------------------------------------------------------------------
OBJ = """mtllib m.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0 0 1
vt 0.0 0.0
vt 1.0 0.0
vt 1.0 2.0
vt -0.5 1.0
g quad
usemtl painted
f 1/1 2/2 3/3 4/4
g tris
f 1/1 2/2 5/4
usemtl plain
f 2/2 3/3 5/1
usemtl painted
f 1 2 5
f -5/-4 -4/-3 -1/-1
"""
MTL = """newmtl painted
Ka 0.5 0.6 0.7
map_Kd -s 1 1 1 tex.npy
newmtl plain
Ka 0.1 0.2 0.3
"""


def test_loader_reads_vt_and_map_kd(tmp_path):
    from mafrixraytracing_amd.scene_io import MaterialManager, load_obj, prim_uv_array
    (tmp_path / "m.obj").write_text(OBJ)
    (tmp_path / "m.mtl").write_text(MTL)
    tex = tx.procedural(0, 4, 6)[..., :3]  # RGB: the loader adds alpha 255
    np.save(tmp_path / "tex.npy", tex)
    mgr = MaterialManager()
    st = load_obj(str(tmp_path / "m.obj"), mgr, textures=True)
    prims = st.groups["quad"] + st.groups["tris"]
    uv = prim_uv_array(prims)
    assert len(mgr.textures) == 1 and mgr.textures[0].shape == (4, 6, 4)
    assert np.array_equal(mgr.textures[0][..., :3], tex) and (mgr.textures[0][..., 3] == 255).all()
    assert list(uv["texture"]) == [0, 0, -1, -1, 0]  # plain has no map; the fourth painted face has no vt
    assert np.array_equal(uv["uv"][0], [[0, 0], [1, 0], [1, 2]])       # a quad: its first three corners
    assert np.array_equal(uv["uv"][1], [[0, 0], [1, 0], [-0.5, 1]])
    assert np.array_equal(uv["uv"][4], [[0, 0], [1, 0], [-0.5, 1]])    # negative indices count from the end
    assert not uv["uv"][2].any() and not uv["uv"][3].any()
    # without textures=True: today's arrays, and nothing of the textures is read
    (tmp_path / "tex.npy").unlink()
    m0, m1 = MaterialManager(), MaterialManager()
    plain = load_obj(str(tmp_path / "m.obj"), m0)
    assert m0.textures == [] and m0.materials == mgr.materials
    for g in st.groups:
        assert [(p.kind, p.pts, p.material) for p in plain.groups[g]] == [(p.kind, p.pts, p.material) for p in st.groups[g]]
        assert all(p.uv is None and p.texture == -1 for p in plain.groups[g])
    with pytest.raises(FileNotFoundError):
        load_obj(str(tmp_path / "m.obj"), m1, textures=True)


def test_scene_arrays_carry_textures_only_when_asked(tmp_path):
    from mafrixraytracing_amd.scene_io import load_scene_file
    (tmp_path / "m.obj").write_text(OBJ)
    (tmp_path / "m.mtl").write_text(MTL)
    np.save(tmp_path / "tex.npy", tx.procedural(0, 4, 6))
    (tmp_path / "s.xml").write_text("""<Scene version="0.1">
  <Models><Model name="m" type="obj"><arg name="filename" value="m.obj"/></Model></Models>
  <Materials><Material name="x" type="lambert"><arg name="albedo" value="0.9, 0.8, 0.7"/></Material></Materials>
  <Shapes>
    <Shape type="shapelist"><arg name="obj_ref" value="m.tris"/><arg name="material" value="2"/></Shape>
  </Shapes>
  <Light type="area"><arg name="shape_ref" value="m.quad"/><arg name="intensity" value="5, 5, 5"/></Light>
  <Film><arg name="width" value="8"/><arg name="height" value="8"/></Film>
</Scene>""")
    a0 = load_scene_file(str(tmp_path / "s.xml"))
    a1 = load_scene_file(str(tmp_path / "s.xml"), textures=True)
    assert a0.textures is None and a0.prim_uv is None
    assert np.array_equal(a0.prims, a1.prims) and np.array_equal(a0.albedo, a1.albedo)
    assert len(a1.textures) == 1 and a1.textures[0].shape == (4, 6, 4)
    assert list(a1.prim_uv["texture"]) == [0, -1, -1, 0]  # the shapelist replaces the material and keeps the map
    b = a1.with_film(4, 4)
    assert b.textures is not None and np.array_equal(b.prim_uv, a1.prim_uv)
