"""The sky (mfx_set_environment, mfx_set_environment_sampled): a square octahedral map of linear RGB radiance that rays leaving the scene
return instead of black. The rule is the contract in include/mafrix_rt.h; `texel_index` states it in Python
floats (IEEE doubles, one rounding per operation, in the order written), so it agrees bit for bit with
csrc/mfx_environment.h, which the host and the gfx950 kernels compile. +y is the pole.

Maps are (S, S, 3) float32 arrays, row yi after row yi - 1: map[yi, xi] is texel id yi * S + xi.
`constant`, `gradient` and `from_latlong` make them on the host; none of that needs bit-exactness, only the
lookup does."""
from __future__ import annotations

import math

import numpy as np

MAX_SIZE = 4096  # MFX_MAX_ENV_SIZE


def _sg(x: float) -> float:
    return 1.0 if x >= 0.0 else -1.0


def _coord(w: float, n: int) -> int:
    f = math.floor(w * float(n))
    return 0 if not f >= 0 else (n - 1 if f >= n else int(f))


def texel_index(d, size: int) -> int:
    """The texel id of unit direction d = (dx, dy, dz) in a size x size map: the header's rule, step by step."""
    dx, dy, dz = float(d[0]), float(d[1]), float(d[2])
    s = (abs(dx) + abs(dy)) + abs(dz)
    px = dx / s
    pz = dz / s
    if dy >= 0.0:  # (-0.0 included)
        a, b = px, pz
    else:
        a = (1.0 - abs(pz)) * _sg(px)
        b = (1.0 - abs(px)) * _sg(pz)
    u = a * 0.5 + 0.5
    v = b * 0.5 + 0.5
    return _coord(v, size) * size + _coord(u, size)


def texel_direction(size: int) -> np.ndarray:
    """(size, size, 3) float64: the unit direction of every texel's centre ([yi, xi]), the inverse of the rule."""
    c = (np.arange(size, dtype=np.float64) + 0.5) / size * 2.0 - 1.0
    a, b = np.meshgrid(c, c)  # a varies with xi (columns), b with yi (rows)
    upper = np.abs(a) + np.abs(b) <= 1.0
    sga = np.where(a >= 0.0, 1.0, -1.0)
    sgb = np.where(b >= 0.0, 1.0, -1.0)
    px = np.where(upper, a, (1.0 - np.abs(b)) * sga)
    pz = np.where(upper, b, (1.0 - np.abs(a)) * sgb)
    py = np.where(upper, 1.0 - np.abs(a) - np.abs(b), -(np.abs(a) + np.abs(b) - 1.0))
    d = np.stack([px, py, pz], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def constant(rgb) -> np.ndarray:
    """A constant sky: the 1 x 1 map of radiance rgb."""
    return np.asarray(rgb, dtype=np.float32).reshape(1, 1, 3).copy()


def gradient(size: int, zenith, horizon, ground) -> np.ndarray:
    """A size x size map that runs linearly in dy from `horizon` (dy = 0) to `zenith` (dy = 1) above and to
    `ground` (dy = -1) below, at every texel's centre."""
    dy = texel_direction(size)[..., 1:2]
    z, h, g = (np.asarray(v, dtype=np.float64).reshape(1, 1, 3) for v in (zenith, horizon, ground))
    up = h + (z - h) * np.clip(dy, 0.0, 1.0)
    down = h + (g - h) * np.clip(-dy, 0.0, 1.0)
    return np.where(dy >= 0.0, up, down).astype(np.float32)


def from_latlong(image, size: int) -> np.ndarray:
    """Resample a latitude-longitude image ((H, W, 3), row 0 at the +y pole, columns running with the azimuth
    atan2(dz, dx) from -pi to pi) into a size x size octahedral map: the nearest pixel at every texel's centre."""
    img = np.asarray(image)
    if img.ndim != 3 or img.shape[2] < 3:
        raise ValueError(f"from_latlong: expected an (H, W, 3) image, got shape {img.shape}")
    H, W = img.shape[0], img.shape[1]
    d = texel_direction(size)
    theta = np.arccos(np.clip(d[..., 1], -1.0, 1.0))  # from the pole
    phi = np.arctan2(d[..., 2], d[..., 0])
    row = np.clip(np.floor(theta / math.pi * H).astype(np.int64), 0, H - 1)
    col = np.clip(np.floor((phi / (2.0 * math.pi) + 0.5) * W).astype(np.int64), 0, W - 1)
    return np.ascontiguousarray(img[row, col, :3], dtype=np.float32)


# ---- the sky as a light (mfx_set_environment_sampled): the header's rule in Python floats -------------------
INVPI = 1. / 3.141592653589793


def sample_table(m):
    """The sampling table the library builds from the map m: (q float32 (n,), alias uint32 (n,), prob float64
    (n,)). The construction is the library's (mfx_env_sample_table); the rule takes the three arrays as data."""
    from .abi import env_sample_table
    return env_sample_table(m)


def sample_entry(r1: float, n: int) -> int:
    """Step 2's entry: floor(r1 * n) clamped into [0, n - 1]."""
    return _coord(r1, n)


def sample_direction(size: int, texel: int, ju: float, jv: float):
    """Step 3: the direction of (texel, ju, jv) in a size x size map: ((ux, uy, uz), len2, len)."""
    xi, yi = int(texel) % size, int(texel) // size
    u = (float(xi) + ju) / float(size)
    a = u * 2.0 - 1.0
    v = (float(yi) + jv) / float(size)
    b = v * 2.0 - 1.0
    py = (1.0 - abs(a)) - abs(b)
    if (abs(a) + abs(b)) <= 1.0:
        px, pz = a, b
    else:
        px = (1.0 - abs(b)) * _sg(a)
        pz = (1.0 - abs(a)) * _sg(b)
    len2 = (px * px + py * py) + pz * pz
    ln = math.sqrt(len2)
    return (px / ln, py / ln, pz / ln), len2, ln


def sample_pdf(prob_t: float, size: int, len2: float, ln: float, nlights: int) -> float:
    """Step 5: pdf_v of a sky vertex of a context with nlights area lights."""
    return (((prob_t * float(size * size)) * 0.25) * (len2 * ln)) / float(nlights + 1)


def sun_map(size: int, sun_texel: int, sun, rest) -> np.ndarray:
    """A size x size map of radiance `rest` (a value or three) with the one texel `sun_texel` at `sun`."""
    m = np.empty((size, size, 3), dtype=np.float32)
    m[:] = np.asarray(rest, dtype=np.float32)
    m.reshape(-1, 3)[int(sun_texel)] = np.asarray(sun, dtype=np.float32)
    return m
