"""Albedo textures: the rule of include/mafrix_rt.h (mfx_create_textured) stated in Python floats (IEEE
double, one rounding per operation, nothing fused), in the order the header gives.

Each world primitive with a texture gets a UV record of 8 doubles, gu[3], cu, gv[3], cv, computed from its
corners v0, v1, v2 and their (u, v), so that u = dot(p, gu) + cu on its plane. At a path vertex the hit
point's (u, v) gives one texel of the primitive's texture by the nearest-texel rule (wrap by u - floor(u),
OBJ's v pointing up), and the vertex's albedo is the material's times texel / 255 per channel.

uv_table mirrors mfx_uv_table (the code context creation runs), texel_index mirrors mfx_texel_index (the
code the kernels run), texel_albedo is the albedo at a hit point. procedural makes textures whose every
texel is a distinct hash of (texture, x, y), so that a wrong index shows as a wrong colour.
"""
from __future__ import annotations

import math

import numpy as np

TEXEL_NONE = 0xFFFFFFFF      # a vertex's texel id on an untextured primitive
MAX_TEXTURES = 4096
MAX_TEXTURE_DIM = 16384
MAX_TEXELS = 2 ** 31 - 2
KIND_SPHERE = 2


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _div(a: float, b: float) -> float:
    """IEEE a / b, division by zero included (Python raises where the hardware gives inf or nan)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def uv_record(v0, v1, v2, uv) -> list:
    """The 8 doubles of one primitive: corners v0, v1, v2 (3 floats each), uv[i] = (u, v) of corner i."""
    v0, v1, v2 = ([float(x) for x in v] for v in (v0, v1, v2))
    e1 = [v1[c] - v0[c] for c in range(3)]
    e2 = [v2[c] - v0[c] for c in range(3)]
    d11, d12, d22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    det = d11 * d22 - d12 * d12
    out = []
    for k in range(2):
        w0, w1, w2 = float(uv[0][k]), float(uv[1][k]), float(uv[2][k])
        dw1, dw2 = w1 - w0, w2 - w0
        a = _div(d22 * dw1 - d12 * dw2, det)
        b = _div(d11 * dw2 - d12 * dw1, det)
        g = [e1[c] * a + e2[c] * b for c in range(3)]
        out += g + [w0 - _dot(v0, g)]
    if det == 0.0 or not all(math.isfinite(x) for x in out):
        return [0.0, 0.0, 0.0, float(uv[0][0]), 0.0, 0.0, 0.0, float(uv[0][1])]
    return out


def uv_table(prims, prim_uv) -> np.ndarray:
    """(n, 8) float64 records of prims (abi.PRIM_DTYPE) under prim_uv (abi.PRIM_UV_DTYPE); zeros for an
    untextured primitive or a sphere."""
    out = np.zeros((len(prims), 8), dtype=np.float64)
    for i in range(len(prims)):
        if int(prim_uv["texture"][i]) < 0 or int(prims["kind"][i]) == KIND_SPHERE:
            continue
        p = prims["p"][i]
        out[i] = uv_record(p[0], p[1], p[2], prim_uv["uv"][i])
    return out


def _coord(w: float, n: int) -> int:
    t = w - math.floor(w)
    f = math.floor(t * float(n))
    return min(max(int(f), 0), n - 1)


def texture_bases(sizes) -> list:
    """First texel of each texture in the concatenation; sizes: (height, width) per texture."""
    bases, total = [], 0
    for h, w in sizes:
        bases.append(total)
        total += int(h) * int(w)
    return bases


def texel_index(sizes, texture: int, u: float, v: float) -> int:
    """The texel id of (u, v) in texture `texture`: base + row * W + xi with row = (H - 1) - yi."""
    h, w = int(sizes[texture][0]), int(sizes[texture][1])
    xi, yi = _coord(float(u), w), _coord(float(v), h)
    return texture_bases(sizes)[texture] + ((h - 1) - yi) * w + xi


def hit_uv(record, hp):
    """(u, v) of hit point hp under a UV record."""
    r = [float(x) for x in record]
    hp = [float(x) for x in hp]
    return _dot(hp, r[0:3]) + r[3], _dot(hp, r[4:7]) + r[7]


def texel_albedo(albedo, textures, sizes, bases, texture: int, record, hp):
    """The albedo at hit point hp of a primitive: `albedo` (3 floats, the material's) on an untextured one
    (texture < 0), else albedo[c] * (texel[c] / 255.0). Returns (a0, a1, a2), texel id or TEXEL_NONE."""
    a = (float(albedo[0]), float(albedo[1]), float(albedo[2]))
    if texture < 0:
        return a, TEXEL_NONE
    u, v = hit_uv(record, hp)
    h, w = sizes[texture]
    xi, yi = _coord(u, int(w)), _coord(v, int(h))
    row = (int(h) - 1) - yi
    t = textures[texture][row, xi]
    return tuple(a[c] * (float(int(t[c])) / 255.0) for c in range(3)), bases[texture] + row * int(w) + xi


def procedural(texture: int, height: int, width: int) -> np.ndarray:
    """(height, width, 4) uint8: every texel's 24 colour bits a bijective hash of its 24-bit position code
    (texture * 2^14 + y * width + x folded into 24 bits), so two texels of one texture of up to 2^24 texels
    never share a colour and neighbouring texels look unrelated. Alpha is 255."""
    y, x = np.mgrid[0:height, 0:width]
    code = (np.uint64(texture) * np.uint64(0x3FFF) + (y * width + x).astype(np.uint64)) & np.uint64(0xFFFFFF)
    # an odd multiplier and xor-shifts: each step is a bijection of 24-bit words
    h = (code * np.uint64(0x9E3779)) & np.uint64(0xFFFFFF)
    h ^= h >> np.uint64(11)
    h = (h * np.uint64(0x85EBCB)) & np.uint64(0xFFFFFF)
    h ^= h >> np.uint64(13)
    out = np.empty((height, width, 4), dtype=np.uint8)
    out[..., 0] = (h & np.uint64(0xFF)).astype(np.uint8)
    out[..., 1] = ((h >> np.uint64(8)) & np.uint64(0xFF)).astype(np.uint8)
    out[..., 2] = ((h >> np.uint64(16)) & np.uint64(0xFF)).astype(np.uint8)
    out[..., 3] = 255
    return out


def planar_prim_uv(prims, texture: int, axes=(0, 1), lo=None, hi=None, scale: float = 1.0):
    """abi.PRIM_UV_DTYPE maps that project every triangle and rect of `prims` onto the plane of two
    coordinate axes of their bounding box [lo, hi] (computed when not given): u, v = scale * (p - lo) /
    (hi - lo). Spheres stay untextured."""
    from .abi import PRIM_UV_DTYPE
    out = np.zeros(len(prims), dtype=PRIM_UV_DTYPE)
    out["texture"] = -1
    flat = prims["kind"] != KIND_SPHERE
    if not flat.any():
        return out
    pts = prims["p"][flat][:, :3, :]
    lo = pts.reshape(-1, 3).min(axis=0) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = pts.reshape(-1, 3).max(axis=0) if hi is None else np.asarray(hi, dtype=np.float64)
    ext = np.where(hi > lo, hi - lo, 1.0)
    uv = np.zeros((len(prims), 3, 2))
    for k, ax in enumerate(axes):
        uv[:, :, k] = scale * (prims["p"][:, :3, ax] - lo[ax]) / ext[ax]
    out["uv"][flat] = uv[flat]
    out["texture"][flat] = texture
    return out
