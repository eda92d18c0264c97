"""The denoiser's rule on the host (numpy only, no GPU): what mfx_denoise must return, bit for bit, for
a colour image and the feature buffers mfx_aov gives.

The rule (include/mafrix_rt.h, DESIGN.md "Feature buffers and denoising"). C is the current colour,
N, Z, A the features' normal [0..2], depth [3] and albedo [4..6];

    d2(a, b) = ((a0-b0)*(a0-b0) + (a1-b1)*(a1-b1)) + (a2-b2)*(a2-b2)        k = [3/8, 1/4, 1/16]

For iteration i = 0 .. iterations-1 with step s = 2^i, for pixel p = (x, y): taps q = (x + dx*s,
y + dy*s), dy = -2..2 outside, dx = -2..2 inside, a tap outside the film skipped. g = 1.0, then in
this order, for each term whose sigma is > 0, g = g * (1.0 / (1.0 + term)):

    normal   term = d2(N_p, N_q) / (sn*sn)
    depth    dz = Z_p - Z_q; den = (sz*sz) * (Z_p*Z_p + Z_q*Z_q); term = (dz*dz)/den if den > 0 else 0
    albedo   term = d2(A_p, A_q) / (sa*sa)
    colour   term = d2(C_p, C_q) / ((sc*sc) * 0.25^i)

wt = (k[|dx|] * k[|dy|]) * g; num_c = num_c + wt * C_q[c], den = den + wt, both from +0.0 in tap order;
out_c = num_c / den. The next iteration reads this output. FP64, one rounding per operation; the
weights are rational, so numpy and the GPU agree to the bit. A sigma > 0 whose divisor is 0 in FP64
(sn*sn, sz*sz or sa*sa, or (sc*sc) * 0.25^i at an iteration that runs) is refused, here with ValueError
and by the library with MFX_E_INVALID: the centre tap's term would be 0/0.

The variance-guided rule (mfx_denoise_var, reference_denoise_var) carries a plane V, the variance of
the pixel's mean luminance, beside the colour; L(c) = (c0 + c1) + c2, k3 = [1/2, 1/4]. Per iteration and
pixel, when sigma_luma > 0:

    prefilter   pn = pd = +0.0; for dy = -1..1 outside, dx = -1..1 inside, q = (x + dx, y + dy) (one pixel
                apart whatever the step; outside the film skipped): kk = k3[|dx|] * k3[|dy|];
                pn = pn + kk * V_q; pd = pd + kk.  Vf = pn / pd;  lden = (sl*sl) * Vf + luma_floor

then the taps as above with the normal, depth and albedo terms and, last, if sigma_luma > 0,

    luminance   dl = L(C_p) - L(C_q); term = (dl*dl) / lden

and beside num and den, vn = vn + (wt*wt) * V_q; V'_p = vn / (den*den). The next iteration reads C' and
V'. With sigma_luma = 0 the colour is reference_denoise's with sigma_color = 0.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

K = (0.375, 0.25, 0.0625)  # the B3 spline's taps 3/8, 1/4, 1/16 at |d| = 0, 1, 2


def _zero_square(s: float) -> bool:
    """A sigma > 0 whose square, the divisor of its term, has underflowed to 0 (below about 1.5e-162):
    the centre tap's term would be 0/0 and every pixel NaN. mfx_denoise and mfx_denoise_var refuse it."""
    s = float(s)
    return s > 0.0 and s * s == 0.0


@dataclass(frozen=True)
class DenoiseConfig:
    iterations: int = 3
    sigma_normal: float = 0.1
    sigma_depth: float = 0.02
    sigma_albedo: float = 0.05
    sigma_color: float = 0.0

    def __post_init__(self):
        if not 1 <= self.iterations <= 8:
            raise ValueError("need 1 <= iterations <= 8")
        for s in (self.sigma_normal, self.sigma_depth, self.sigma_albedo, self.sigma_color):
            if not (np.isfinite(s) and s >= 0):
                raise ValueError("every sigma must be finite and >= 0")
        for s in (self.sigma_normal, self.sigma_depth, self.sigma_albedo):
            if _zero_square(s):
                raise ValueError("a sigma > 0 must have a non-zero square")
        if self.sigma_color > 0:  # the colour term divides by sc2 * 0.25^i: the loop's own products
            sc2 = float(self.sigma_color) * float(self.sigma_color)
            quarter = 1.0
            for _ in range(self.iterations):
                if sc2 * quarter == 0.0:
                    raise ValueError("sigma_color > 0 must keep (sigma_color^2) * 0.25^i non-zero at every iteration")
                quarter = quarter * 0.25


def _d2(a, b):
    """d2 of two (..., 3) arrays, in the rule's order."""
    e0, e1, e2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (e0 * e0 + e1 * e1) + e2 * e2


def reference_denoise(color: np.ndarray, features: np.ndarray, w: int, h: int,
                      cfg: DenoiseConfig = DenoiseConfig()) -> np.ndarray:
    """color: (w*h, >=3) x-major (pixel x*h + y; alpha ignored); features: (w*h, >=7) as mfx_aov
    returns them. Returns the (w*h, 4) filtered image, alpha 1.0. All pixels advance together, one tap
    at a time: every accumulator takes its additions in tap order (never np.sum, which sums pairwise)."""
    C = np.array(np.asarray(color, dtype=np.float64)[:, :3]).reshape(w, h, 3)
    F = np.asarray(features, dtype=np.float64).reshape(w, h, -1)
    N, Z, A = F[..., 0:3], F[..., 3], F[..., 4:7]
    sn2 = cfg.sigma_normal * cfg.sigma_normal
    sz2 = cfg.sigma_depth * cfg.sigma_depth
    sa2 = cfg.sigma_albedo * cfg.sigma_albedo
    sc2 = cfg.sigma_color * cfg.sigma_color
    X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    quarter = 1.0  # 0.25^i
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(cfg.iterations):
            s = 1 << i
            num = np.zeros((w, h, 3))
            den = np.zeros((w, h))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    xq, yq = X + dx * s, Y + dy * s
                    ok = (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
                    if not ok.any():
                        continue
                    xq, yq = np.clip(xq, 0, w - 1), np.clip(yq, 0, h - 1)  # (a skipped tap's value is unused)
                    Cq = C[xq, yq]
                    g = np.ones((w, h))
                    if cfg.sigma_normal > 0:
                        g = g * (1.0 / (1.0 + _d2(N, N[xq, yq]) / sn2))
                    if cfg.sigma_depth > 0:
                        Zq = Z[xq, yq]
                        dz = Z - Zq
                        dd = sz2 * (Z * Z + Zq * Zq)
                        pos = dd > 0
                        term = np.where(pos, (dz * dz) / np.where(pos, dd, 1.0), 0.0)
                        g = g * (1.0 / (1.0 + term))
                    if cfg.sigma_albedo > 0:
                        g = g * (1.0 / (1.0 + _d2(A, A[xq, yq]) / sa2))
                    if cfg.sigma_color > 0:
                        g = g * (1.0 / (1.0 + _d2(C, Cq) / (sc2 * quarter)))
                    wt = (K[abs(dx)] * K[abs(dy)]) * g
                    num = np.where(ok[..., None], num + wt[..., None] * Cq, num)
                    den = np.where(ok, den + wt, den)
            C = num / den[..., None]
            quarter = quarter * 0.25
    out = np.ones((w * h, 4))
    out[:, :3] = C.reshape(w * h, 3)
    return out


K3 = (0.5, 0.25)  # the variance prefilter's taps 1/2, 1/4 at |d| = 0, 1


@dataclass(frozen=True)
class DenoiseVarConfig:
    iterations: int = 3
    sigma_normal: float = 0.1
    sigma_depth: float = 0.02
    sigma_albedo: float = 0.05
    sigma_luma: float = 4.0
    luma_floor: float = 1e-6

    def __post_init__(self):
        if not 1 <= self.iterations <= 8:
            raise ValueError("need 1 <= iterations <= 8")
        for s in (self.sigma_normal, self.sigma_depth, self.sigma_albedo, self.sigma_luma):
            if not (np.isfinite(s) and s >= 0):
                raise ValueError("every sigma must be finite and >= 0")
        for s in (self.sigma_normal, self.sigma_depth, self.sigma_albedo):  # (sigma_luma's square is added to luma_floor > 0)
            if _zero_square(s):
                raise ValueError("a sigma > 0 must have a non-zero square")
        if not (np.isfinite(self.luma_floor) and self.luma_floor > 0):
            raise ValueError("luma_floor must be finite and > 0")


def variance_of_mean(S1, S2, n) -> np.ndarray:
    """The variance of a pixel's mean luminance from its moments S1 = sum Y, S2 = sum Y*Y over n >= 2
    samples (n a number, or per pixel): d = S2 - (S1*S1)/n; (d if d > 0 else +0.0) / (n*(n - 1.0)). The
    adaptive sampler's tile check computes the same v_p."""
    S1 = np.asarray(S1, dtype=np.float64)
    S2 = np.asarray(S2, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    d = S2 - (S1 * S1) / n
    return np.where(d > 0.0, d, 0.0) / (n * (n - 1.0))


def reference_denoise_var(color: np.ndarray, variance: np.ndarray, features: np.ndarray, w: int, h: int,
                          cfg: DenoiseVarConfig = DenoiseVarConfig()) -> tuple[np.ndarray, np.ndarray]:
    """color: (w*h, >=3) x-major (alpha ignored); variance: (w*h,) x-major, >= 0; features: (w*h, >=7)
    as mfx_aov returns them. Returns the (w*h, 4) filtered image, alpha 1.0, and the (w*h,) variance the
    last iteration leaves. All pixels advance together, one tap at a time, as in reference_denoise."""
    C = np.array(np.asarray(color, dtype=np.float64)[:, :3]).reshape(w, h, 3)
    V = np.array(np.asarray(variance, dtype=np.float64)).reshape(w, h)
    F = np.asarray(features, dtype=np.float64).reshape(w, h, -1)
    N, Z, A = F[..., 0:3], F[..., 3], F[..., 4:7]
    sn2 = cfg.sigma_normal * cfg.sigma_normal
    sz2 = cfg.sigma_depth * cfg.sigma_depth
    sa2 = cfg.sigma_albedo * cfg.sigma_albedo
    sl2 = cfg.sigma_luma * cfg.sigma_luma
    X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")

    def tap(dx, dy):
        xq, yq = X + dx, Y + dy
        ok = (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
        return ok, np.clip(xq, 0, w - 1), np.clip(yq, 0, h - 1)  # (a skipped tap's value is unused)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(cfg.iterations):
            s = 1 << i
            if cfg.sigma_luma > 0:
                pn = np.zeros((w, h))
                pd = np.zeros((w, h))
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        ok, xq, yq = tap(dx, dy)
                        kk = K3[abs(dx)] * K3[abs(dy)]
                        pn = np.where(ok, pn + kk * V[xq, yq], pn)
                        pd = np.where(ok, pd + kk, pd)
                lden = sl2 * (pn / pd) + cfg.luma_floor
                Lp = (C[..., 0] + C[..., 1]) + C[..., 2]
            num = np.zeros((w, h, 3))
            den = np.zeros((w, h))
            vn = np.zeros((w, h))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ok, xq, yq = tap(dx * s, dy * s)
                    if not ok.any():
                        continue
                    Cq = C[xq, yq]
                    g = np.ones((w, h))
                    if cfg.sigma_normal > 0:
                        g = g * (1.0 / (1.0 + _d2(N, N[xq, yq]) / sn2))
                    if cfg.sigma_depth > 0:
                        Zq = Z[xq, yq]
                        dz = Z - Zq
                        dd = sz2 * (Z * Z + Zq * Zq)
                        pos = dd > 0
                        term = np.where(pos, (dz * dz) / np.where(pos, dd, 1.0), 0.0)
                        g = g * (1.0 / (1.0 + term))
                    if cfg.sigma_albedo > 0:
                        g = g * (1.0 / (1.0 + _d2(A, A[xq, yq]) / sa2))
                    if cfg.sigma_luma > 0:
                        dl = Lp - ((Cq[..., 0] + Cq[..., 1]) + Cq[..., 2])
                        g = g * (1.0 / (1.0 + (dl * dl) / lden))
                    wt = (K[abs(dx)] * K[abs(dy)]) * g
                    num = np.where(ok[..., None], num + wt[..., None] * Cq, num)
                    den = np.where(ok, den + wt, den)
                    vn = np.where(ok, vn + (wt * wt) * V[xq, yq], vn)
            C = num / den[..., None]
            V = vn / (den * den)
    out = np.ones((w * h, 4))
    out[:, :3] = C.reshape(w * h, 3)
    return out, V.reshape(w * h)
