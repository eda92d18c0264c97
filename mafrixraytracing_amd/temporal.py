"""mfx_temporal's rule on the host (numpy only, no GPU): what the library must return, bit for bit, for a
frame, its variance and counts, the current features and camera, and a history.

The rule (include/mafrix_rt.h). Per pixel p = (x, y), q = x*h + y: this frame's colour C,
variance of the mean luminance V and sample count n; the current features N (normal), Z (depth), F (hit
fraction) and camera (o, tl, r, d); the history's colour HC, variance HV, effective count HN, its view's
features HNm, HZ, HF and camera (o', tl', r', d'). FP64, one rounding per operation:

    dot(a, b) = (a0*b0 + a1*b1) + a2*b2     cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)
    d2(a, b) = ((a0-b0)*(a0-b0) + (a1-b1)*(a1-b1)) + (a2-b2)*(a2-b2)

    1. no history, or F != 1.0: reject
    2. u = (x + 0.5)/w, v = (y + 0.5)/h; target = (tl + r*u) + d*v; t = target - o; l = sqrt(dot(t, t));
       dir = t / l (0 when l == 0); P = o + dir*Z
    3. e = P - o', a = tl' - o', nn = cross(r', d'); den = dot(e, nn), num = dot(a, nn); reject unless
       num*den > 0; s = num/den; g = e*s - a; u' = dot(g, r')/dot(r', r'), v' = dot(g, d')/dot(d', d');
       reject unless 0 <= u' < 1 and 0 <= v' < 1; x' = min(w-1, int(floor(u'*w))), y' likewise, q' = x'*h + y'
    4. reject unless HF_q' == 1.0; ze = sqrt(dot(e, e)); dz = ze - HZ_q'; reject unless
       dz*dz <= (tol_depth*tol_depth)*(ze*ze); reject unless d2(N_p, HNm_q') <= tol_normal2
    5. accept: nh = HN_q' if HN_q' < max_history else max_history; nt = n + nh; wc = n/nt; wh = nh/nt;
       C'_c = wc*C_c + wh*HC_c; V' = (wc*wc)*V + (wh*wh)*HV; N' = nt.   reject: C' = C, V' = V, N' = n
    6. the new history is (C', V', N') with the current features and camera

The inverse of step 3 is exact for orthogonal r', d' (what the constructor gives); with skewed derived
axes it is the same arithmetic and only approximately the same point.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .abi import pinhole_derive  # noqa: F401  (the library's constructor: mfx_pinhole_derive)


@dataclass(frozen=True)
class TemporalConfig:
    tol_depth: float = 0.02
    tol_normal2: float = 0.01
    max_history: float = 64.0

    def __post_init__(self):
        for t in (self.tol_depth, self.tol_normal2):
            if not (np.isfinite(t) and t >= 0):
                raise ValueError("the tolerances must be finite and >= 0")
        if not (np.isfinite(self.max_history) and self.max_history > 0):
            raise ValueError("max_history must be finite and > 0")


def camera_of(info) -> dict:
    """The derived camera of NativeContext.camera_info() (its first twelve doubles), or of a
    pinhole_derive dict: position, topleft, right, down as (3,) float64 arrays."""
    if isinstance(info, dict):
        return {k: np.array(info[k], dtype=np.float64).reshape(3) for k in ("position", "topleft", "right", "down")}
    v = np.asarray(info, dtype=np.float64)
    return {"position": v[0:3].copy(), "topleft": v[3:6].copy(), "right": v[6:9].copy(), "down": v[9:12].copy()}


@dataclass
class History:
    """What mfx_temporal keeps between calls: the merged planes, x-major, and their view."""
    color: np.ndarray     # (w*h, 3)
    variance: np.ndarray  # (w*h,)
    count: np.ndarray     # (w*h,)
    normal: np.ndarray    # (w*h, 3)
    depth: np.ndarray     # (w*h,)
    hit: np.ndarray       # (w*h,)
    camera: dict          # position, topleft, right, down


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _d2(a, b):
    e0, e1, e2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (e0 * e0 + e1 * e1) + e2 * e2


def reference_temporal(color, variance, count, features, camera, history, w: int, h: int,
                       cfg: TemporalConfig = TemporalConfig(), restart: bool = False):
    """color: (w*h, >=3) x-major (alpha ignored); variance, count: (w*h,); features: (w*h, 8) as mfx_aov
    returns them; camera: the current derived camera (camera_of); history: a History or None.
    Returns (frame (w*h, 4) alpha 1.0, variance (w*h,), count (w*h,), accepted, the new History). All pixels
    advance together, operation by operation in the rule's order."""
    npix = w * h
    C = np.array(np.asarray(color, dtype=np.float64)[:, :3]).reshape(npix, 3)
    V = np.array(np.asarray(variance, dtype=np.float64)).reshape(npix)
    n = np.array(np.asarray(count, dtype=np.float64)).reshape(npix)
    Fe = np.asarray(features, dtype=np.float64).reshape(npix, -1)
    N, Z, F = Fe[:, 0:3], Fe[:, 3], Fe[:, 7]
    cam = camera_of(camera)
    Co, Vo, No = C.copy(), V.copy(), n.copy()
    acc = np.zeros(npix, dtype=bool)
    if history is not None and not restart:
        X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
        X, Y = X.reshape(npix).astype(np.float64), Y.reshape(npix).astype(np.float64)
        o, tl, r, d = cam["position"], cam["topleft"], cam["right"], cam["down"]
        hc = camera_of(history.camera)
        ho, htl, hr, hd = hc["position"], hc["topleft"], hc["right"], hc["down"]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            u = (X + 0.5) / float(w)
            v = (Y + 0.5) / float(h)
            target = (tl[None, :] + r[None, :] * u[:, None]) + d[None, :] * v[:, None]
            t = target - o[None, :]
            l = np.sqrt(_dot(t, t))
            dirv = np.where((l == 0.0)[:, None], 0.0, t / np.where(l == 0.0, 1.0, l)[:, None])
            P = o[None, :] + dirv * Z[:, None]
            e = P - ho[None, :]
            a = (htl - ho)[None, :]
            nn = _cross(hr, hd)[None, :]
            den = _dot(e, nn)
            num = _dot(a, nn)
            ok = (F == 1.0) & (num * den > 0.0)
            s = num / den
            g = e * s[:, None] - a
            hu = _dot(g, hr[None, :]) / _dot(hr, hr)
            hv = _dot(g, hd[None, :]) / _dot(hd, hd)
            ok = ok & (hu >= 0.0) & (hu < 1.0) & (hv >= 0.0) & (hv < 1.0)
            hx = np.minimum(w - 1, np.floor(np.where(ok, hu, 0.0) * float(w)).astype(np.int64))
            hy = np.minimum(h - 1, np.floor(np.where(ok, hv, 0.0) * float(h)).astype(np.int64))
            q = hx * h + hy
            ok = ok & (np.asarray(history.hit)[q] == 1.0)
            ze = np.sqrt(_dot(e, e))
            dz = ze - np.asarray(history.depth)[q]
            ok = ok & (dz * dz <= (cfg.tol_depth * cfg.tol_depth) * (ze * ze))
            ok = ok & (_d2(N, np.asarray(history.normal)[q]) <= cfg.tol_normal2)
            hn = np.asarray(history.count)[q]
            nh = np.where(hn < cfg.max_history, hn, cfg.max_history)
            nt = n + nh
            wc, wh = n / nt, nh / nt
            Cm = wc[:, None] * C + wh[:, None] * np.asarray(history.color)[q]
            Vm = (wc * wc) * V + (wh * wh) * np.asarray(history.variance)[q]
        acc = ok
        Co = np.where(acc[:, None], Cm, C)
        Vo = np.where(acc, Vm, V)
        No = np.where(acc, nt, n)
    frame = np.ones((npix, 4))
    frame[:, :3] = Co
    new = History(color=Co.copy(), variance=Vo.copy(), count=No.copy(), normal=np.array(N), depth=np.array(Z),
                  hit=np.array(F), camera=cam)
    return frame, Vo, No, int(acc.sum()), new
