"""The sky as a light: env_helpers.reference_paths stated once more with the rule of include/mafrix_rt.h
(mfx_set_environment_sampled): the pick over N + 1 lights, always drawn; for the pick N the four draws r1, r2,
ju, jv, the texel through the alias table, its direction, pdf_v and the direct term a_v = ((cs * E_t) * INVPI)
/ pdf_v; the shadow query to the extension ray's far bound; and the miss term for camera rays (nv = 0) only.
The table (q, alias, prob) is the library's, taken as data (environment.sample_table;
tests/test_sky_sampling_reference.py pins it). With all-zero area lights and a black map its image is black and its
ray counts are the oracle's wherever they do not depend on the draws the rule adds (depth 0, the furnace floor),
which is what ties it to the oracle.

Every arithmetic step is a Python float operation (IEEE double, one rounding each, nothing fused), in the
rule's order. The queries (closest hit, any hit) and the draw streams are the oracle's own.
"""
from __future__ import annotations

import math

import numpy as np

from env_helpers import sky_radiance
from lights_helpers import DRAWS_PER_VERTEX, INVPI, TWOPI, _Light, _add, _dot, _f3, _len, _mul, _normalize, _sub
from mafrixraytracing_amd.abi import PRIM_DTYPE, SceneArrays
from mafrixraytracing_amd.environment import sample_direction, sample_entry, sample_pdf, sample_table, sun_map
from mafrixraytracing_amd.lights import light_table, pick

SKY_FAR = 99999999.  # the extension ray's far bound (Integrators.fs:108)
_tables = {}


def table_of(env):
    """The library's sampling table of the map env, computed once per map: (q, alias, prob) as numpy arrays."""
    key = (env.shape, env.tobytes() if env.size <= 1 << 16 else (float(env.sum()), env[0, 0].tobytes()))
    if key not in _tables:
        _tables[key] = sample_table(env)
    return _tables[key]


def reference_paths(arrays, lights, seed, px, py, samples, max_depth, tex=None, oscene=None, env=None, info=None):
    """Radiance of the paths (px[k], py[k], samples[k]) of `arrays` lit by `lights` and the sampled sky `env` (an
    (S, S, 3) float32 map), the albedo looked up through `tex` (None: the material's). Returns (radiance (K, 3),
    ray counts [primary, extension, shadow]). info: a dict that receives `sky_picked`, `sky_lit`, `sky_occluded`
    and `sky_back` (cs <= 0): the sky vertices of each kind, and `camera_misses` and `later_misses`."""
    import pyoracle
    osc = oscene if oscene is not None else pyoracle.OracleScene(arrays)
    N = len(lights)
    assert N >= 1 and env is not None
    size = env.shape[0]
    texels = env.reshape(-1, 3)
    q_tab, alias_tab, prob_tab = table_of(env)
    tab = light_table(lights)
    # pdf_n = (1 / area_n) / (N + 1)
    LT = [_Light(L, float(tab[n, 1]) / float(N + 1)) for n, L in enumerate(lights)]
    area = [float(tab[n, 0]) for n in range(N)]
    K = len(px)
    w, h = arrays.width, arrays.height
    cam = arrays.camera
    albedo = np.asarray(arrays.albedo, dtype=np.float64)
    prim_mat = arrays.prims["material"]
    ndraws = 2 + (max_depth + 1) * (DRAWS_PER_VERTEX + 1)
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
    sky = [None] * K                # per path: E of the camera ray that missed
    stat = {"sky_picked": 0, "sky_lit": 0, "sky_occluded": 0, "sky_back": 0, "camera_misses": 0, "later_misses": 0}
    live = list(range(K))
    depth = max_depth
    while live and depth >= 0:
        rays = np.array([o[k] + d[k] for k in live], dtype=np.float64)
        t, prim, nrm = osc.closest_hit(rays)
        cont, shadow_rays, shadow_tmax, pend = [], [], [], []
        for r, k in enumerate(live):
            if prim[r] < 0:  # a camera ray's miss shows the background; a later miss is black (the pick has the sky)
                if not verts[k]:
                    sky[k] = sky_radiance(env, d[k])
                    stat["camera_misses"] += 1
                else:
                    stat["later_misses"] += 1
                continue
            tt = float(t[r])
            hp = _add(o[k], _mul(d[k], tt))  # Ray.PointAtParameter
            nm = _f3(nrm[r])
            a = albedo[prim_mat[prim[r]]]
            a = (float(a[0]), float(a[1]), float(a[2])) if tex is None else tex.albedo(a, int(prim[r]), hp)
            dr, q = draws[k], pos[k]
            p = (20.0, 20.0, 20.0)
            while _dot(p, p) >= 1.0 or _dot(nm, p) <= 0.:  # GetRandomInUnitSphere (Material.fs:9-14)
                p = _sub(_mul((dr[q], dr[q + 1], dr[q + 2]), 2.0), (1.0, 1.0, 1.0))
                q += 3
            wi = _normalize(p)
            ei = _dot(nm, wi)
            col = tuple(TWOPI * (ei * (INVPI * a[c])) for c in range(3))
            n = pick(dr[q], N + 1)  # the pick: always drawn
            q += 1
            if n == N:  # the sky
                r1, r2, ju, jv = float(dr[q]), float(dr[q + 1]), float(dr[q + 2]), float(dr[q + 3])
                q += 4
                pos[k] = q
                e = sample_entry(r1, size * size)
                tx = e if r2 < float(q_tab[e]) else int(alias_tab[e])
                unit, len2, ln = sample_direction(size, tx, ju, jv)
                cs = _dot(unit, nm)
                pdf_v = sample_pdf(float(prob_tab[tx]), size, len2, ln, N)
                stat["sky_picked"] += 1
                counts[2] += 1
                shadow_rays.append(hp + unit)
                shadow_tmax.append(SKY_FAR)
                pend.append((k, n, (tx, cs, pdf_v), unit, nm, col))
            else:
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
            for r, (k, n, what, unit, nm, col) in enumerate(pend):
                if n == N:
                    tx, cs, pdf_v = what
                    if not cs > 0.0:
                        stat["sky_back"] += 1
                        a_v = (0.0, 0.0, 0.0)
                    elif occ[r]:
                        stat["sky_occluded"] += 1
                        a_v = (0.0, 0.0, 0.0)
                    else:
                        stat["sky_lit"] += 1
                        E = texels[tx]
                        a_v = tuple(((cs * float(E[c])) * INVPI) / pdf_v for c in range(3))
                    verts[k].append((a_v, col))
                    continue
                L = LT[n]
                to_light = what
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
        f = sky[k] if sky[k] is not None else (0.0, 0.0, 0.0)
        for a_v, col in reversed(verts[k]):  # (l / pdf_li + TraceRay(next)) * col / pdf, pdf = 1
            f = tuple(((a_v[c] + f[c]) * col[c]) / 1. for c in range(3))
        rad[k] = f
    if info is not None:
        info.update(stat)
    return rad, np.array(counts, dtype=np.float64)


# ---- the unbiasedness pair: the furnace floor, one occluding sphere above it, black lights, a sun map ----------
PAIR_W, PAIR_H = 16, 12
PAIR_SUN_TEXEL = 16 * 6 + 9  # an upper-hemisphere texel of the 16 x 16 map (|a| + |b| < 1)


def pair_map():
    """The 16 x 16 sun map: one texel 2000, the rest 0.3."""
    return sun_map(16, PAIR_SUN_TEXEL, (2000.0, 2000.0, 2000.0), (0.3, 0.3, 0.3))


def pair_scene(max_depth):
    """env_helpers' furnace floor joined by one sphere above it (it occludes part of the sky), a light of
    intensity 0, a 16 x 12 film. The floor's corners run the other way round than there, so that its normal is
    +y and its hemisphere is the one the sphere and the sun are in."""
    prims = np.zeros(2, dtype=PRIM_DTYPE)
    prims[0]["kind"] = 1
    prims[0]["material"] = 0
    prims[0]["p"] = [(-1000.0, 0.0, -1000.0), (-1000.0, 0.0, 1000.0), (1000.0, 0.0, 1000.0), (1000.0, 0.0, -1000.0)]
    prims[1]["kind"] = 2  # a sphere: centre, radius
    prims[1]["material"] = 1
    prims[1]["p"][0] = (0.3, 1.2, 0.0)
    prims[1]["p"][1, 0] = 0.8
    light = {"p": [(-1.0, 50.0, -1.0), (1.0, 50.0, -1.0), (1.0, 50.0, 1.0), (-1.0, 50.0, 1.0)],
             "normal": (0.0, -1.0, 0.0), "intensity": (0.0, 0.0, 0.0)}
    camera = {"position": (0.0, 4.0, 6.0), "direction": (0.0, -1.0, -1.0), "fov": 40.0, "aspect": PAIR_W / PAIR_H}
    return SceneArrays(prims, np.array([(0.2, 0.5, 0.8), (0.6, 0.6, 0.6)]), light, camera, PAIR_W, PAIR_H, max_depth)


def film_stats(rad, npix, spp):
    """Of per-path radiances (npix * spp, 3), pixel-major: (film mean (3,), its standard error (3,) estimated from
    the per-pixel means, the mean over pixels of the per-pixel sample variance (3,))."""
    r = np.asarray(rad, dtype=np.float64).reshape(npix, spp, 3)
    pix = r.mean(axis=1)
    se = np.sqrt(pix.var(axis=0, ddof=1) / npix)
    return pix.mean(axis=0), se, r.var(axis=1, ddof=1).mean(axis=0)
