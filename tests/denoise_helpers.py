"""Shared by tests/test_denoise_reference.py and tests/test_gpu_denoise.py: the feature buffers mfx_aov
must return, composed on the host from calls the CPU oracle already has, and a per-pixel scalar
statement of the denoiser's rule (plain Python floats) to hold the numpy one against."""
import numpy as np

from conftest import SEED, scene

_features = {}
_frames = {}


def scene_features(oracle, a, spp, base, seed=SEED):
    """(w*h, 8) x-major features of a SceneArrays: for pixel (i, j) and global sample s the path's own
    camera ray (key pixel i*h + j, draws 0 and 1 -> u, v -> PinholeCamera.GetRay) and its Bvh.Hit;
    normal, t, the hit primitive's material's albedo and 1.0 per hit, summed in sample order from +0.0
    (a miss adds nothing), divided once by float(spp)."""
    w, h = a.width, a.height
    cam = a.camera
    o = oracle.OracleScene(a)
    acc = np.zeros((w * h, 8))
    for s in range(base, base + spp):
        rays = np.zeros((w * h, 6))
        for i in range(w):
            for j in range(h):
                p = i * h + j
                d = oracle.rng_draws(seed, p, s, 2)
                u, v = (i + d[0]) / w, (j + d[1]) / h
                ro, rd = oracle.kat_camera_ray(cam["position"], cam["direction"], cam["fov"], cam["aspect"], u, v)
                rays[p, :3], rays[p, 3:] = ro, rd
        t, prim, nrm = o.closest_hit(rays)
        hit = prim >= 0
        alb = a.albedo[a.prims["material"][np.where(hit, prim, 0)]]
        add = np.concatenate([nrm, t[:, None], alb, np.ones((w * h, 1))], axis=1)
        acc = np.where(hit[:, None], acc + add, acc)
    return acc / float(spp)


def oracle_features(oracle, name, w, h, spp, base, seed=SEED):
    """scene_features of scenes/<name>.xml at w x h. Computed once per case and left unchanged."""
    world = name.replace("@2l", "")  # the same world scene however it is traced
    key = (world, w, h, spp, base, seed)
    if key in _features:
        return _features[key]
    f = scene_features(oracle, scene(world, w, h), spp, base, seed)
    f.setflags(write=False)
    _features[key] = f
    return f


def oracle_frame(oracle, name, w, h, spp, base=0):
    """The oracle's Sample(spp) from sample `base`, computed once per case and left unchanged."""
    world = name.replace("@2l", "")
    key = (world, w, h, spp, base)
    if key not in _frames:
        f = oracle.OracleScene(scene(world, w, h)).sample(spp, SEED, sample_base=base)
        f.setflags(write=False)
        _frames[key] = f
    return _frames[key]


def scalar_denoise(color, features, w, h, cfg):
    """The rule pixel by pixel in Python floats (IEEE binary64, one rounding per operation)."""
    K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
    C = [[float(v) for v in row[:3]] for row in np.asarray(color)]
    F = [[float(v) for v in row] for row in np.asarray(features)]

    def d2(a, b):
        return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])

    for i in range(cfg.iterations):
        s = 2 ** i
        out = []
        for x in range(w):
            for y in range(h):
                p = x * h + y
                num, den = [0.0, 0.0, 0.0], 0.0
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
                        if cfg.sigma_color > 0:
                            g = g * (1.0 / (1.0 + d2(C[p], C[q]) / ((cfg.sigma_color * cfg.sigma_color) * 0.25 ** i)))
                        wt = (K[abs(dx)] * K[abs(dy)]) * g
                        for c in range(3):
                            num[c] = num[c] + wt * C[q][c]
                        den = den + wt
                out.append([num[0] / den, num[1] / den, num[2] / den])
        C = out
    r = np.ones((w * h, 4))
    r[:, :3] = np.array(C)
    return r


def smallest_with_a_square():
    """The smallest double s > 0 with s*s != 0.0 (about 1.5e-162), by bisection over the bit patterns."""
    lo, hi = np.array([1e-170]).view(np.int64)[0], np.array([1e-150]).view(np.int64)[0]
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        s = float(np.array([mid]).view(np.float64)[0])
        if s * s != 0.0:
            hi = mid
        else:
            lo = mid
    s, below = (float(np.array([b]).view(np.float64)[0]) for b in (hi, lo))
    assert s * s != 0.0 and below * below == 0.0 and 1e-163 < s < 1e-161
    return s, below
