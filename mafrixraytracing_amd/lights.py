"""Several area lights, one picked per path vertex: the rule of include/mafrix_rt.h
(mfx_create_lights) stated in numpy FP64, one rounding per operation.

A context has lights L_0 .. L_{N-1}, 1 <= N <= MAX_LIGHTS. At a path vertex, with N >= 2, one draw r
picks light n = floor(r * N); that light's Sample_Li gives the shadow ray, and the direct term is
divided by pdf_n = (1 / area_n) / N. The division by N is where this departs from the reference's
RandomDirectLightIntegrator (Integrators.fs:57-78), which returns the picked light's own pdf and so
renders the mean of the lights; here the image is their sum.

light_table mirrors mfx_light_table (the code context creation runs), pick mirrors the kernels' pick.
"""
from __future__ import annotations

import numpy as np

MAX_LIGHTS = 64


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, v):
    return (a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0])


def _len(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def quad_area(p) -> np.float64:
    """Rect.area of the quad p[0..4): its two triangles' areas (p0 p1 p2), (p0 p2 p3), each half the
    cross product's length (Trangle.fs:114), added in that order."""
    q = [tuple(np.float64(c) for c in p[k]) for k in range(4)]
    area = np.float64(0.0)
    for t, (a, b, c) in enumerate(((q[0], q[1], q[2]), (q[0], q[2], q[3]))):
        ta = _len(_cross(_sub(b, a), _sub(c, a))) * np.float64(0.5)
        area = ta if t == 0 else area + ta
    return area


def light_table(lights) -> np.ndarray:
    """(N, 4) float64: area, 1 / area, pdf_n = (1 / area) / N, 0 of every light (dicts with "p": the
    four corners). Two divisions, in that order."""
    n = len(lights)
    if not 1 <= n <= MAX_LIGHTS:
        raise ValueError(f"1 <= len(lights) <= {MAX_LIGHTS}")
    out = np.zeros((n, 4), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, L in enumerate(lights):
            area = quad_area(L["p"])
            inv = np.float64(1.0) / area
            out[k, 0] = area
            out[k, 1] = inv
            out[k, 2] = inv / np.float64(n)
    return out


def _lerp(a, b, s):
    return tuple(float(a[c]) + (float(b[c]) - float(a[c])) * s for c in range(3))


def strips(light: dict, n: int) -> list:
    """`light` cut into n strips along its first edge (p0 -> p1 and p3 -> p2): the same surface as n
    lights (tests and scripts/lights_bench.py use it; the image is not the whole light's, since
    NewAreaLight.L grows with a light's own area: DESIGN.md §9e)."""
    p = light["p"]
    out = []
    for k in range(n):
        s0, s1 = k / n, (k + 1) / n
        out.append({"p": (_lerp(p[0], p[1], s0), _lerp(p[0], p[1], s1), _lerp(p[3], p[2], s1), _lerp(p[3], p[2], s0)),
                    "normal": tuple(light["normal"]), "intensity": tuple(light["intensity"])})
    return out


def pick(r: float, n: int) -> int:
    """The light a draw r in [0, 1) picks among n: floor(r * n), the product rounded once. No clamp: a
    draw is k * 2^-53 with k < 2^53, so r <= 1 - 2^-53 and the exact product is at most n - n * 2^-53.
    With 2^e <= n < 2^(e+1) the doubles below n are 2^(e-52) apart (2^(e-53) when n = 2^e), and
    n * 2^-53 >= 2^(e-53) with equality only for n = 2^e: then the product is the double just below n
    itself, and otherwise it lies more than half a spacing below n, so rounding to nearest gives the
    double below n, never n (rounding is monotone: smaller draws stay below too)."""
    return int(np.floor(np.float64(r) * np.float64(n)))
