"""Shared by tests/test_temporal_reference.py, tests/test_gpu_temporal.py and tests/test_gpu_camera.py: a
scene under another camera, a per-pixel scalar statement of mfx_temporal's rule (plain Python floats) to
hold the numpy one against, and histories made by hand."""
import math

import numpy as np

from mafrixraytracing_amd.abi import SceneArrays
from mafrixraytracing_amd.temporal import History, camera_of


def with_camera(a, camera):
    """The SceneArrays `a` seen through another camera dict (position, direction, fov, aspect)."""
    b = SceneArrays(a.prims, a.albedo, a.light, dict(camera), a.width, a.height, a.max_depth, a.instancing, a.two_level)
    return b


def moved(camera, dpos=(0.0, 0.0, 0.0), ddir=(0.0, 0.0, 0.0)):
    """A camera dict shifted by dpos and turned by ddir (added to the direction)."""
    c = dict(camera)
    c["position"] = tuple(float(p) + float(d) for p, d in zip(camera["position"], dpos))
    c["direction"] = tuple(float(p) + float(d) for p, d in zip(camera["direction"], ddir))
    return c


def history_of(color, variance, count, features, camera):
    """A History whose view is `features` ((w*h, 8) as mfx_aov gives them) under `camera`."""
    f = np.asarray(features, dtype=np.float64)
    return History(color=np.array(np.asarray(color, dtype=np.float64)[:, :3]), variance=np.array(variance, dtype=np.float64),
                   count=np.array(count, dtype=np.float64), normal=np.array(f[:, 0:3]), depth=np.array(f[:, 3]),
                   hit=np.array(f[:, 7]), camera=camera_of(camera))


def scalar_temporal(color, variance, count, features, camera, history, w, h, cfg, restart=False):
    """The rule pixel by pixel in Python floats (IEEE binary64, one rounding per operation). Returns the
    (w*h, 4) frame, the (w*h,) variance and count, and the number of accepted pixels."""
    C = [[float(v) for v in row[:3]] for row in np.asarray(color)]
    V = [float(v) for v in np.asarray(variance)]
    Nn = [float(v) for v in np.asarray(count)]
    F = [[float(v) for v in row] for row in np.asarray(features)]
    cam = {k: [float(x) for x in v] for k, v in camera_of(camera).items()}

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def d2(a, b):
        return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])

    out, vout, nout, accepted = [], [], [], 0
    have = history is not None and not restart
    if have:
        hc = {k: [float(x) for x in v] for k, v in camera_of(history.camera).items()}
        HC, HV, HN = np.asarray(history.color), np.asarray(history.variance), np.asarray(history.count)
        HNm, HZ, HF = np.asarray(history.normal), np.asarray(history.depth), np.asarray(history.hit)
    for x in range(w):
        for y in range(h):
            p = x * h + y
            res = (C[p], V[p], Nn[p])
            if have and F[p][7] == 1.0:
                o, tl, r, d = cam["position"], cam["topleft"], cam["right"], cam["down"]
                u = (float(x) + 0.5) / float(w)
                v = (float(y) + 0.5) / float(h)
                target = [(tl[k] + r[k] * u) + d[k] * v for k in range(3)]
                t = [target[k] - o[k] for k in range(3)]
                ln = math.sqrt(dot(t, t))
                dr = [0.0, 0.0, 0.0] if ln == 0.0 else [t[k] / ln for k in range(3)]
                P = [o[k] + dr[k] * F[p][3] for k in range(3)]
                ho, htl, hr, hd = hc["position"], hc["topleft"], hc["right"], hc["down"]
                e = [P[k] - ho[k] for k in range(3)]
                a = [htl[k] - ho[k] for k in range(3)]
                nn = cross(hr, hd)
                den, num = dot(e, nn), dot(a, nn)
                if num * den > 0.0:
                    s = num / den
                    g = [e[k] * s - a[k] for k in range(3)]
                    hu = dot(g, hr) / dot(hr, hr)
                    hv = dot(g, hd) / dot(hd, hd)
                    if 0.0 <= hu < 1.0 and 0.0 <= hv < 1.0:
                        q = min(w - 1, int(math.floor(hu * float(w)))) * h + min(h - 1, int(math.floor(hv * float(h))))
                        if float(HF[q]) == 1.0:
                            ze = math.sqrt(dot(e, e))
                            dz = ze - float(HZ[q])
                            if dz * dz <= (cfg.tol_depth * cfg.tol_depth) * (ze * ze) and \
                                    d2(F[p][0:3], [float(z) for z in HNm[q]]) <= cfg.tol_normal2:
                                hn = float(HN[q])
                                nh = hn if hn < cfg.max_history else cfg.max_history
                                nt = Nn[p] + nh
                                wc, wh = Nn[p] / nt, nh / nt
                                res = ([wc * C[p][k] + wh * float(HC[q][k]) for k in range(3)],
                                       (wc * wc) * V[p] + (wh * wh) * float(HV[q]), nt)
                                accepted += 1
            out.append(res[0])
            vout.append(res[1])
            nout.append(res[2])
    frame = np.ones((w * h, 4))
    frame[:, :3] = np.array(out)
    return frame, np.array(vout), np.array(nout), accepted


def random_view(rng, w, h, camera, depth=(2.0, 6.0)):
    """Random features of a view: unit normals from a few directions, depths in a range, albedo, and a hit
    fraction that is 1.0 for most pixels, below 1 or 0 for the rest."""
    npix = w * h
    f = np.zeros((npix, 8))
    dirs = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.0, 0.8]])
    f[:, 0:3] = dirs[rng.integers(0, len(dirs), npix)]
    f[:, 3] = rng.uniform(depth[0], depth[1], npix)
    f[:, 4:7] = rng.uniform(0.0, 1.0, (npix, 3))
    f[:, 7] = np.where(rng.uniform(size=npix) < 0.85, 1.0, rng.choice([0.0, 0.25, 0.75], npix))
    return f
