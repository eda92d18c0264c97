"""Shared by tests/test_denoise_var_reference.py and tests/test_gpu_denoise_var.py: a per-pixel scalar
statement of the variance-guided denoiser's rule (plain Python floats) to hold the numpy one against,
and the luminance moments the adaptive sampler keeps, composed from the CPU oracle's one-sample frames."""
import numpy as np

from conftest import SEED, scene

_lum = {}


def oracle_sample_frames(oracle, name, w, h, n):
    """(n, w*h, 4): the oracle's one-sample frames of global samples 0..n-1, computed once per case
    (extended when a later test asks for more) and left unchanged."""
    world = name.replace("@2l", "")  # the same world scene however it is traced
    key = (world, w, h)
    if key not in _lum or len(_lum[key]) < n:
        o = oracle.OracleScene(scene(world, w, h))
        have = list(_lum.get(key, ()))
        f = np.stack(have + [o.sample(1, SEED, sample_base=s) for s in range(len(have), n)])
        f.setflags(write=False)
        _lum[key] = f
    return _lum[key][:n]


def pixel_counts(tile_spp, w, h):
    """(w*h,) x-major: every pixel's own 8x8 tile's sample count."""
    x, y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    return np.asarray(tile_spp)[y >> 3, x >> 3].reshape(w * h)


def mean_and_moments(frames, counts):
    """What the adaptive sampler holds for per-pixel sample counts `counts` ((w*h,), or one number): the
    (w*h, 4) mean (the sum of a pixel's first n samples in sample order, divided once by n; alpha 1.0) and
    the moments S1 = sum Y, S2 = sum Y*Y of Y = (fx + fy) + fz, in sample order from +0.0."""
    npix = frames.shape[1]
    n = np.broadcast_to(np.asarray(counts), (npix,))
    acc = np.zeros((npix, 3))
    S1 = np.zeros(npix)
    S2 = np.zeros(npix)
    for s in range(int(n.max())):
        on = s < n
        f = frames[s][:, :3]
        y = (f[:, 0] + f[:, 1]) + f[:, 2]
        acc = np.where(on[:, None], acc + f, acc)
        S1 = np.where(on, S1 + y, S1)
        S2 = np.where(on, S2 + y * y, S2)
    mean = np.ones((npix, 4))
    mean[:, :3] = acc / n.astype(np.float64)[:, None]
    return mean, S1, S2


def scalar_denoise_var(color, variance, features, w, h, cfg):
    """The rule pixel by pixel in Python floats (IEEE binary64, one rounding per operation). Returns the
    (w*h, 4) image and the (w*h,) variance."""
    K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
    K3 = (1.0 / 2.0, 1.0 / 4.0)
    C = [[float(v) for v in row[:3]] for row in np.asarray(color)]
    V = [float(v) for v in np.asarray(variance)]
    F = [[float(v) for v in row] for row in np.asarray(features)]

    def d2(a, b):
        return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])

    def lum(c):
        return (c[0] + c[1]) + c[2]

    for i in range(cfg.iterations):
        s = 2 ** i
        out, vout = [], []
        for x in range(w):
            for y in range(h):
                p = x * h + y
                lden = None
                if cfg.sigma_luma > 0:
                    pn, pd = 0.0, 0.0
                    for dy in range(-1, 2):
                        for dx in range(-1, 2):
                            xq, yq = x + dx, y + dy
                            if not (0 <= xq < w and 0 <= yq < h):
                                continue
                            kk = K3[abs(dx)] * K3[abs(dy)]
                            pn = pn + kk * V[xq * h + yq]
                            pd = pd + kk
                    vf = pn / pd
                    lden = (cfg.sigma_luma * cfg.sigma_luma) * vf + cfg.luma_floor
                num, den, vn = [0.0, 0.0, 0.0], 0.0, 0.0
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        xq, yq = x + dx * s, y + dy * s
                        if not (0 <= xq < w and 0 <= yq < h):
                            continue
                        q = xq * h + yq
                        g = 1.0
                        if cfg.sigma_normal > 0:
                            g = g * (1.0 / (1.0 + d2(F[p][0:3], F[q][0:3]) / (cfg.sigma_normal * cfg.sigma_normal)))
                        if cfg.sigma_depth > 0:
                            zp, zq = F[p][3], F[q][3]
                            dz = zp - zq
                            dd = (cfg.sigma_depth * cfg.sigma_depth) * (zp * zp + zq * zq)
                            g = g * (1.0 / (1.0 + ((dz * dz) / dd if dd > 0 else 0.0)))
                        if cfg.sigma_albedo > 0:
                            g = g * (1.0 / (1.0 + d2(F[p][4:7], F[q][4:7]) / (cfg.sigma_albedo * cfg.sigma_albedo)))
                        if cfg.sigma_luma > 0:
                            dl = lum(C[p]) - lum(C[q])
                            g = g * (1.0 / (1.0 + (dl * dl) / lden))
                        wt = (K[abs(dx)] * K[abs(dy)]) * g
                        for c in range(3):
                            num[c] = num[c] + wt * C[q][c]
                        den = den + wt
                        vn = vn + (wt * wt) * V[q]
                out.append([num[0] / den, num[1] / den, num[2] / den])
                vout.append(vn / (den * den))
        C, V = out, vout
    r = np.ones((w * h, 4))
    r[:, :3] = np.array(C)
    return r, np.array(V)
