"""Smooth shading: the rule of include/mafrix_rt.h (mfx_set_normals) stated in Python floats (IEEE double, one
rounding per operation, nothing fused), in the order the header gives.

Each smooth world primitive gets a normal record of 12 doubles, g_0[3], k_0, g_1[3], k_1, g_2[3], k_2, computed from
its corners v0, v1, v2 and their normals, so that component c of the interpolated normal is dot(p, g_c) + k_c on its
plane. At a path vertex the hit point's interpolated normal, normalized and put on the face normal's side, replaces
the face normal.

normal_table mirrors mfx_normal_table (the code mfx_set_normals runs), shading_normal mirrors mfx_shading_normal
(the code the kernels run). smooth_normals makes corner normals for a mesh that carries none.
"""
from __future__ import annotations

import math

import numpy as np

KIND_SPHERE = 2
KIND_RECT = 1


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _div(a: float, b: float) -> float:
    """IEEE a / b, division by zero included (Python raises where the hardware gives inf or nan)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)



def normal_record(v0, v1, v2, n) -> list:
    """The 12 doubles of one primitive: corners v0, v1, v2 (3 floats each), n[i] = the normal of corner i."""
    v0, v1, v2 = ([float(x) for x in v] for v in (v0, v1, v2))
    e1 = [v1[c] - v0[c] for c in range(3)]
    e2 = [v2[c] - v0[c] for c in range(3)]
    d11, d12, d22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    det = d11 * d22 - d12 * d12
    out = []
    for c in range(3):
        w0, w1, w2 = float(n[0][c]), float(n[1][c]), float(n[2][c])
        dw1, dw2 = w1 - w0, w2 - w0
        a = _div(d22 * dw1 - d12 * dw2, det)
        b = _div(d11 * dw2 - d12 * dw1, det)
        g = [e1[k] * a + e2[k] * b for k in range(3)]
        out += g + [w0 - _dot(v0, g)]
    if det == 0.0 or not all(math.isfinite(x) for x in out):
        return [0.0, 0.0, 0.0, float(n[0][0]), 0.0, 0.0, 0.0, float(n[0][1]), 0.0, 0.0, 0.0, float(n[0][2])]
    return out


def normal_table(prims, prim_normals) -> np.ndarray:
    """(n, 12) float64 records of prims (abi.PRIM_DTYPE) under prim_normals (abi.PRIM_NORMALS_DTYPE); zeros for a
    primitive with smooth == 0 or a sphere."""
    out = np.zeros((len(prims), 12), dtype=np.float64)
    for i in range(len(prims)):
        if int(prim_normals["smooth"][i]) == 0 or int(prims["kind"][i]) == KIND_SPHERE:
            continue
        p = prims["p"][i]
        out[i] = normal_record(p[0], p[1], p[2], prim_normals["n"][i])
    return out


def shading_normal(record, ng, hp) -> tuple:
    """Steps 1-4: the shading normal at hit point hp under `record` of a vertex whose normal is ng."""
    r = [float(x) for x in record]
    hp = [float(x) for x in hp]
    ng = [float(x) for x in ng]
    r0 = _dot(hp, r[0:3]) + r[3]
    r1 = _dot(hp, r[4:7]) + r[7]
    r2 = _dot(hp, r[8:11]) + r[11]
    q = (r0 * r0 + r1 * r1) + r2 * r2
    l = math.sqrt(q) if q >= 0.0 else math.nan  # (sqrt of nan: nan; of +inf: +inf)
    if l > 0.0 and math.isfinite(l):
        ns = [r0 / l, r1 / l, r2 / l]
    else:
        ns = list(ng)
    if _dot(ns, ng) < 0.0:
        ns = [-ns[0], -ns[1], -ns[2]]
    return (ns[0], ns[1], ns[2])


def shading_normals(records, ng, hp) -> np.ndarray:
    """shading_normal over (n, 12) records, (n, 3) normals and (n, 3) hit points."""
    return np.array([shading_normal(records[k], ng[k], hp[k]) for k in range(len(records))], dtype=np.float64).reshape(-1, 3)


def face_normals(prims) -> np.ndarray:
    """(n, 3) the triangles' and rects' unit face normals, (e1 x e2) / |e1 x e2| (zeros for a sphere or a face
    without area)."""
    p = prims["p"]
    a = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.sqrt((a * a).sum(axis=1))
    ok = (ln > 0.0) & (prims["kind"] != KIND_SPHERE)
    out = np.zeros((len(prims), 3))
    out[ok] = a[ok] / ln[ok, None]
    return out


def smooth_normals(prims, crease_deg: float = 60.0) -> np.ndarray:
    """abi.PRIM_NORMALS_DTYPE corner normals of a mesh that carries none: area-weighted vertex normals over the
    faces that share a position (welded where the three coordinates are bit-equal), a corner taking only the
    adjacent faces whose normal lies within crease_deg of its own face's, so that a hard edge stays hard. A rect
    counts with the area of its first three corners' parallelogram, and gets the normals of those corners. Spheres
    and faces without area keep smooth == 0."""
    from .abi import PRIM_NORMALS_DTYPE
    out = np.zeros(len(prims), dtype=PRIM_NORMALS_DTYPE)
    if len(prims) == 0:
        return out
    p = prims["p"]
    kind = prims["kind"]
    a = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])  # area-weighted face normals (twice a triangle's area)
    ln = np.sqrt((a * a).sum(axis=1))
    face_ok = (ln > 0.0) & (kind != KIND_SPHERE) & np.isfinite(ln)
    unit = np.zeros_like(a)
    unit[face_ok] = a[face_ok] / ln[face_ok, None]
    ncorner = np.where(kind == KIND_RECT, 4, 3)
    # weld: every corner's position -> a vertex id (bit-equal coordinates; -0.0 and 0.0 are one position)
    fidx, cidx = [], []
    for k in range(4):
        sel = np.nonzero(face_ok & (ncorner > k))[0]
        fidx.append(sel)
        cidx.append(np.full(len(sel), k))
    fidx, cidx = np.concatenate(fidx), np.concatenate(cidx)
    pos = p[fidx, cidx] + 0.0
    _, vid = np.unique(pos, axis=0, return_inverse=True)
    vid = np.asarray(vid).reshape(-1)
    order = np.argsort(vid, kind="stable")
    bounds = np.nonzero(np.diff(vid[order]))[0] + 1
    cos_crease = math.cos(math.radians(crease_deg))
    nrm = np.zeros((len(prims), 4, 3))
    for grp in np.split(order, bounds):
        f = fidx[grp]
        u = unit[f]
        within = (u @ u.T) >= cos_crease  # [corner's face, adjacent face]
        nrm[f, cidx[grp]] = within.astype(np.float64) @ a[f]
    out["n"][face_ok] = nrm[face_ok][:, :3]
    out["smooth"][face_ok] = 1
    return out
