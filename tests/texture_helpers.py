"""Albedo textures: lights_helpers.reference_paths (the oracle's trace_ray stated in Python FP64, with the
light pick) stated once more with the albedo of a vertex replaced by the texel lookup of
include/mafrix_rt.h (mfx_create_textured), which it imports from mafrixraytracing_amd.textures; and the
scenes, textures and maps the texture tests share. With no textured primitive, and with an all-255
texture, this equals lights_helpers.reference_paths bit for bit (tests/test_textures_reference.py), which is
what ties it to the oracle.

Every arithmetic step is a Python float operation (IEEE double, one rounding each, nothing fused), in the
oracle's order. The queries (closest hit, any hit) and the draw streams are the oracle's own.
"""
from __future__ import annotations

import math

import numpy as np

from lights_helpers import DRAWS_PER_VERTEX, INVPI, TWOPI, _Light, _add, _dot, _f3, _len, _mul, _normalize, _sub
from mafrixraytracing_amd.abi import PRIM_DTYPE, PRIM_UV_DTYPE, SceneArrays
from mafrixraytracing_amd.lights import light_table, pick
from mafrixraytracing_amd.textures import procedural, texel_albedo, texture_bases, uv_table


class TexSet:
    """Textures ((H, W, 4) uint8) and the world primitives' maps, with what the lookup needs derived once."""

    def __init__(self, prims, textures, prim_uv):
        self.textures = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
        self.prim_uv = np.ascontiguousarray(prim_uv, dtype=PRIM_UV_DTYPE)
        self.sizes = [(t.shape[0], t.shape[1]) for t in self.textures]
        self.bases = texture_bases(self.sizes)
        self.records = uv_table(prims, self.prim_uv)
        self.ptex = [int(t) for t in self.prim_uv["texture"]]

    def albedo(self, mat_albedo, prim, hp):
        return texel_albedo(mat_albedo, self.textures, self.sizes, self.bases, self.ptex[prim], self.records[prim], hp)[0]


def reference_paths(arrays, lights, seed, px, py, samples, max_depth, tex: TexSet | None, oscene=None, first_albedo=None):
    """Radiance of the paths (px[k], py[k], samples[k]) of `arrays` (its world primitives) lit by `lights`,
    with the albedo at every vertex looked up through `tex` (None: the material's alone). Returns
    (radiance (K, 3), ray counts [primary, extension, shadow]). first_albedo: a (K, 4) array that receives
    the albedo at each path's first hit and 1.0 (a miss leaves zeros): mfx_aov's planes [4..7] per sample."""
    import pyoracle
    osc = oscene if oscene is not None else pyoracle.OracleScene(arrays)
    N = len(lights)
    tab = light_table(lights)
    LT = [_Light(L, tab[n, 2]) for n, L in enumerate(lights)]
    area = [float(tab[n, 0]) for n in range(N)]
    K = len(px)
    w, h = arrays.width, arrays.height
    cam = arrays.camera
    albedo = np.asarray(arrays.albedo, dtype=np.float64)
    prim_mat = arrays.prims["material"]
    ndraws = 2 + (max_depth + 1) * DRAWS_PER_VERTEX
    draws, pos = [], [2] * K
    o, d = [None] * K, [None] * K
    for k in range(K):
        i, j = int(px[k]), int(py[k])
        dr = pyoracle.rng_draws(seed, i * h + j, int(samples[k]), ndraws)
        draws.append(dr)
        u = (float(i) + dr[0]) / float(w)
        v = (float(j) + dr[1]) / float(h)
        oo, dd = pyoracle.kat_camera_ray(cam["position"], cam["direction"], cam["fov"], cam["aspect"], u, v)
        o[k], d[k] = _f3(oo), _f3(dd)
    counts = [K, 0, 0]
    verts = [[] for _ in range(K)]  # per path: (a_v, col) of every vertex, camera first
    live = list(range(K))
    depth = max_depth
    while live and depth >= 0:
        rays = np.array([o[k] + d[k] for k in live], dtype=np.float64)
        t, prim, nrm = osc.closest_hit(rays)
        cont, shadow_rays, shadow_tmax, pend = [], [], [], []
        for r, k in enumerate(live):
            if prim[r] < 0:
                continue
            tt = float(t[r])
            hp = _add(o[k], _mul(d[k], tt))  # Ray.PointAtParameter
            nm = _f3(nrm[r])
            a = albedo[prim_mat[prim[r]]]
            a = (float(a[0]), float(a[1]), float(a[2])) if tex is None else tex.albedo(a, int(prim[r]), hp)  # the lookup
            if first_albedo is not None and depth == max_depth:
                first_albedo[k] = (a[0], a[1], a[2], 1.0)
            dr, q = draws[k], pos[k]
            p = (20.0, 20.0, 20.0)
            while _dot(p, p) >= 1.0 or _dot(nm, p) <= 0.:  # GetRandomInUnitSphere (Material.fs:9-14)
                p = _sub(_mul((dr[q], dr[q + 1], dr[q + 2]), 2.0), (1.0, 1.0, 1.0))
                q += 3
            wi = _normalize(p)
            ei = _dot(nm, wi)
            col = tuple(TWOPI * (ei * (INVPI * a[c])) for c in range(3))
            n = 0
            if N >= 2:  # the pick: one more draw, only with several lights
                n = pick(dr[q], N)
                q += 1
            L = LT[n]
            sel = dr[q]
            tr = L.tris[0] if sel < 0.5 else L.tris[1]
            tu, tv = float(dr[q + 1]), float(dr[q + 2])
            q += 3
            pos[k] = q
            uu, vv = tu, tv
            if tu + tv > 1.:
                uu, vv = 1. - tu, 1. - tv
            e1, e2 = _sub(tr[1], tr[0]), _sub(tr[2], tr[0])
            sq = math.sqrt(1. - uu)
            s1, s2 = 1. - sq, vv * sq
            lp = _add(_add(tr[0], _mul(e1, s1)), _mul(e2, s2))
            to_light = _sub(lp, hp)
            dist = _len(to_light)
            unit = (to_light[0] / dist, to_light[1] / dist, to_light[2] / dist)
            counts[2] += 1
            shadow_rays.append(hp + unit)
            shadow_tmax.append(dist - 1e-6)
            pend.append((k, n, to_light, unit, nm, col))
            if depth - 1 >= 0:
                counts[1] += 1
                o[k], d[k] = hp, wi
                cont.append(k)
        if pend:
            occ = osc.any_hit(np.array(shadow_rays, dtype=np.float64), np.array(shadow_tmax, dtype=np.float64))
            for r, (k, n, to_light, unit, nm, col) in enumerate(pend):
                L = LT[n]
                if occ[r]:
                    l = (0.0, 0.0, 0.0)
                else:
                    cos_o = _dot(to_light, L.normal)  # NewAreaLight.L (Light.fs:48-56)
                    if cos_o < 0.:
                        dist2 = to_light[0] * to_light[0] + to_light[1] * to_light[1] + to_light[2] * to_light[2]
                        solid = math.fabs(cos_o) * area[n] / dist2
                        Lc = (solid * L.color[0], solid * L.color[1], solid * L.color[2])
                    else:
                        Lc = (0.0, 0.0, 0.0)
                    cs = _dot(unit, nm)
                    l = (cs * Lc[0], cs * Lc[1], cs * Lc[2])
                verts[k].append(((l[0] / L.pdf, l[1] / L.pdf, l[2] / L.pdf), col))
        live = cont
        depth -= 1
    rad = np.zeros((K, 3), dtype=np.float64)
    for k in range(K):
        f = (0.0, 0.0, 0.0)
        for a_v, col in reversed(verts[k]):  # (l / pdf_li + TraceRay(next)) * col / pdf, pdf = 1
            f = tuple(((a_v[c] + f[c]) * col[c]) / 1. for c in range(3))
        rad[k] = f
    return rad, np.array(counts, dtype=np.float64)


# ---- the textures and the mixed soup of the GPU tests -----------------------------------------------------
TEX_SIZES = ((1, 1), (5, 3), (64, 64))  # (height, width): 1 x 1, 3 wide by 5 high, 64 x 64


def soup_textures():
    return [procedural(k, h, w) for k, (h, w) in enumerate(TEX_SIZES)]


def random_prim_uv(prims, ntextures, seed, textured=0.7):
    """Maps for `prims`: about `textured` of the triangles and rects get a texture in turn and (u, v) in
    [-1.5, 2.5] (outside [0, 1] and negative: the wrap), the rest and every sphere stay untextured."""
    rng = np.random.default_rng(seed)
    out = np.zeros(len(prims), dtype=PRIM_UV_DTYPE)
    out["texture"] = -1
    k = 0
    for i in range(len(prims)):
        if int(prims["kind"][i]) == 2 or rng.random() >= textured:
            continue
        out[i]["texture"] = k % ntextures
        out[i]["uv"] = rng.uniform(-1.5, 2.5, size=(3, 2))
        k += 1
    return out


def soup_scene(w, h, max_depth=3, nmat=5, seed=11):
    """The Cornell box (its own rects and light) with a seeded soup of small triangles, rects and spheres
    inside it, textured and untextured primitives side by side in the same leaves."""
    from conftest import scene
    a = scene("cornell", w, h, max_depth=max_depth)
    rng = np.random.default_rng(seed)
    base = a.prims
    pts = base["p"][base["kind"] != 2][:, :3, :].reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    mid, ext = (lo + hi) * 0.5, (hi - lo)
    extra = np.zeros(36, dtype=PRIM_DTYPE)
    for i in range(len(extra)):
        c = mid + (rng.random(3) - 0.5) * ext * 0.7
        kind = i % 3
        extra[i]["kind"] = kind
        if kind == 2:
            extra[i]["p"][0] = c
            extra[i]["p"][1][0] = 0.04 + 0.04 * rng.random()
        else:
            e1, e2 = (rng.random(3) - 0.5) * 0.35, (rng.random(3) - 0.5) * 0.35
            extra[i]["p"][0], extra[i]["p"][1], extra[i]["p"][2] = c, c + e1, c + e1 + e2
            extra[i]["p"][3] = c + e2  # a parallelogram: v0, v1, v2, v3
    albedo = np.concatenate([a.albedo, 0.2 + 0.7 * rng.random((max(0, nmat - len(a.albedo)), 3))])
    extra["material"] = rng.integers(0, len(albedo), size=len(extra))
    prims = np.concatenate([base, extra])
    if nmat > 256:  # materials past k_resolve's LDS table on primitives the paths meet
        prims["material"][:len(base)] = 256 + rng.integers(0, nmat - 256, size=len(base))
    return SceneArrays(prims, albedo, a.light, a.camera, w, h, max_depth)
