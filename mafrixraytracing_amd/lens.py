"""The thin lens (mfx_set_lens) in Python floats: the lens record of a derived camera and the camera ray through
the lens, by the rule of include/mafrix_rt.h. Every arithmetic step is one Python float operation (IEEE double,
one rounding each, nothing fused) in the order the rule writes it, and the draws are 64-bit integer arithmetic,
so these agree bit for bit with the library's host calls (abi.lens_derive, abi.lens_rays) and with the kernels,
which compile one header (csrc/mfx_lens.h).

A derived camera is a dict of position, topleft, right, down (abi.pinhole_derive makes one of a scene-file camera).
"""
from __future__ import annotations

import math

_M64 = 0xFFFFFFFFFFFFFFFF
GOLDEN = 0x9E3779B97F4A7C15
LENS_COUNTER0 = 1 << 31  # the lens stream: counters 2^31 + 1, 2^31 + 2, ... of the path's own key


def mix64(z: int) -> int:
    z &= _M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z


def path_key(seed: int, pixel: int, sample: int) -> int:
    """The key of (pixel = x * height + y, sample) under `seed`, as the kernels derive it."""
    return mix64((seed & _M64) ^ mix64(((pixel << 32) & _M64) | (sample & 0xFFFFFFFF)))


def draw(key: int, m: int) -> float:
    """Draw m of `key`: rng_unit(mix64(key + m * GOLDEN)), rng_next with counter m (m = 1 is a path's first draw)."""
    z = mix64((key + m * GOLDEN) & _M64)
    return float(z >> 11) * (1.0 / 9007199254740992.0)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _f3(x):
    return (float(x[0]), float(x[1]), float(x[2]))


def derive(cam, aperture: float, focus: float):
    """The lens record of derived camera `cam`: (U, V, s), and the forward axis f and dplane beside it. ValueError
    names the field the library refuses."""
    P0, TL, R, D = _f3(cam["position"]), _f3(cam["topleft"]), _f3(cam["right"]), _f3(cam["down"])
    aperture, focus = float(aperture), float(focus)
    if not (aperture >= 0.0) or not math.isfinite(aperture):
        raise ValueError("aperture must be finite and >= 0")
    if not (focus > 0.0) or not math.isfinite(focus):
        raise ValueError("focus must be finite and > 0")
    lr, ld = math.sqrt(_dot(R, R)), math.sqrt(_dot(D, D))
    if not (lr > 0.0) or not math.isfinite(lr):
        raise ValueError("lr")
    if not (ld > 0.0) or not math.isfinite(ld):
        raise ValueError("ld")
    U = tuple((R[c] / lr) * aperture for c in range(3))
    V = tuple((D[c] / ld) * aperture for c in range(3))
    n = (R[1] * D[2] - R[2] * D[1], R[2] * D[0] - R[0] * D[2], R[0] * D[1] - R[1] * D[0])
    ln = math.sqrt(_dot(n, n))
    if not (ln > 0.0) or not math.isfinite(ln):
        raise ValueError("ln")
    f = (n[0] / ln, n[1] / ln, n[2] / ln)
    dplane = _dot((TL[0] - P0[0], TL[1] - P0[1], TL[2] - P0[2]), f)
    if not (dplane > 0.0) or not math.isfinite(dplane):
        raise ValueError("dplane")
    s = focus / dplane
    if not math.isfinite(s):
        raise ValueError("s")
    return {"U": U, "V": V, "s": s, "f": f, "dplane": dplane}


def ray(cam, rec, key: int, u: float, v: float):
    """The camera ray of (u, v), the path's first two draws, through the lens `rec` of derived camera `cam`:
    (o, d, a, b, trials, fp): origin, unit direction, the accepted disk point, the trials it took, the focus point."""
    P0, TL, R, D = _f3(cam["position"]), _f3(cam["topleft"]), _f3(cam["right"]), _f3(cam["down"])
    U, V, s = rec["U"], rec["V"], rec["s"]
    m, trials = LENS_COUNTER0, 0
    while True:
        r1, r2 = draw(key, m + 1), draw(key, m + 2)
        m += 2
        trials += 1
        a = r1 * 2.0 - 1.0
        b = r2 * 2.0 - 1.0
        if (a * a + b * b) < 1.0:
            break
    o, fp, w = [0.0] * 3, [0.0] * 3, [0.0] * 3
    for c in range(3):
        target = (TL[c] + R[c] * u) + D[c] * v
        pin = target - P0[c]
        o[c] = (P0[c] + U[c] * a) + V[c] * b
        fp[c] = P0[c] + pin * s
        w[c] = fp[c] - o[c]
    l = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    d = (0.0, 0.0, 0.0) if l == 0.0 else (w[0] / l, w[1] / l, w[2] / l)
    return tuple(o), d, a, b, trials, tuple(fp)


def path_ray(cam, rec, seed: int, width: int, height: int, x: int, y: int, sample: int):
    """ray() of sample `sample` of pixel (x, y) of a width x height film under `seed`."""
    key = path_key(seed, x * height + y, sample)
    u = (float(x) + draw(key, 1)) / float(width)
    v = (float(y) + draw(key, 2)) / float(height)
    return ray(cam, rec, key, u, v)
