"""The adaptive sampler's rule on the host (numpy only, no GPU): what mfx_sample_adaptive must return,
computed from per-sample images such as the CPU oracle's one-sample frames.

The rule (include/mafrix_rt.h, DESIGN.md "Adaptive sampling"). Tiles are the film's 8x8 pixel tiles,
tiles_x = ceil(w/8), tiles_y = ceil(h/8); a tile's valid pixels are those inside the film, m of them.
For one sample of a pixel with radiance (fx, fy, fz), Y = (fx + fy) + fz. Per pixel, in sample order
and FP64: S1 = sum Y, S2 = sum Y*Y. After n samples of every pixel of a tile

    v_p = max(0, S2_p - S1_p*S1_p/n) / (n*(n-1))
    E = sum_valid v_p          M = sum_valid S1_p/n
    converged  <=>  E*m <= rel_error^2 * (|M| + abs_floor*m)^2

Every tile gets min_spp samples and is checked; an unconverged tile gets step_spp more, clipped at
max_spp, and is checked again; it stops at the first check it passes, or at max_spp.

mfx_sample_adaptive_resume continues such a result (reference_resume): every tile is checked at its
own count under the call's threshold, and the tiles that fail go on from their own counts.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class AdaptiveConfig:
    min_spp: int
    max_spp: int
    step_spp: int
    rel_error: float
    abs_floor: float

    def __post_init__(self):
        if not (2 <= self.min_spp <= self.max_spp and self.step_spp >= 1):
            raise ValueError("need 2 <= min_spp <= max_spp and step_spp >= 1")
        if not (np.isfinite(self.rel_error) and self.rel_error >= 0 and np.isfinite(self.abs_floor) and self.abs_floor >= 0):
            raise ValueError("rel_error and abs_floor must be finite and >= 0")


@dataclass(frozen=True)
class ResumeConfig:
    """mfx_adaptive_resume: the budget, the pass limit (0: none) and the threshold of a resume."""
    max_spp: int
    step_spp: int
    rel_error: float
    abs_floor: float
    max_passes: int = 0

    def __post_init__(self):
        if not (self.max_spp >= 2 and self.step_spp >= 1 and self.max_passes >= 0):
            raise ValueError("need max_spp >= 2, step_spp >= 1 and max_passes >= 0")
        if not (np.isfinite(self.rel_error) and self.rel_error >= 0 and np.isfinite(self.abs_floor) and self.abs_floor >= 0):
            raise ValueError("rel_error and abs_floor must be finite and >= 0")


def tile_grid(w: int, h: int) -> tuple[int, int]:
    """(tiles_y, tiles_x) of a w x h film."""
    return (h + 7) // 8, (w + 7) // 8


def tile_pixels(w: int, h: int, tx: int, ty: int) -> np.ndarray:
    """x-major indices (x*h + y) of a tile's valid pixels."""
    xs = np.arange(tx * 8, min(tx * 8 + 8, w))
    ys = np.arange(ty * 8, min(ty * 8 + 8, h))
    return (xs[None, :] * h + ys[:, None]).ravel()


def luminance(frames: np.ndarray) -> np.ndarray:
    """Y = (fx + fy) + fz of per-sample images frames[s, pixel, 0..2]."""
    f = np.asarray(frames, dtype=np.float64)
    return (f[..., 0] + f[..., 1]) + f[..., 2]


def check_sides(S1: np.ndarray, S2: np.ndarray, n: int, cfg: AdaptiveConfig) -> tuple[float, float]:
    """(E*m, rel_error^2 (|M| + abs_floor m)^2) of one tile from its valid pixels' moments."""
    m = float(len(S1))
    nf = float(n)
    v = np.maximum(0.0, S2 - S1 * S1 / nf) / (nf * (nf - 1.0))
    E = float(np.sum(v))
    M = float(np.sum(S1 / nf))
    t = abs(M) + cfg.abs_floor * m
    return E * m, (cfg.rel_error * cfg.rel_error) * (t * t)


def reference_tile_spp(Y: np.ndarray, w: int, h: int, cfg: AdaptiveConfig) -> tuple[np.ndarray, float]:
    """Y[s, x*h + y]: the luminance of sample s (s < max_spp) of every pixel. Returns the
    (tiles_y, tiles_x) int32 sample counts and the smallest relative gap |lhs - rhs| / max(lhs, rhs)
    between the two sides of the test at any check, the one at max_spp included (lhs = rhs = 0 — a
    black tile with abs_floor 0 — holds in any summation order and does not count). A tile whose
    gap is near the rounding error of the sums
    (~1e-9) could fall either way on a device that sums E and M in another order."""
    Y = np.asarray(Y, dtype=np.float64)
    assert Y.shape == (cfg.max_spp, w * h), Y.shape
    ty_n, tx_n = tile_grid(w, h)
    spp = np.zeros((ty_n, tx_n), dtype=np.int32)
    S1 = np.zeros(w * h)
    S2 = np.zeros(w * h)
    active = [(ty, tx) for ty in range(ty_n) for tx in range(tx_n)]
    pix = {t: tile_pixels(w, h, t[1], t[0]) for t in active}
    gap = float("inf")
    done = 0
    while active:
        ns = cfg.min_spp if done == 0 else min(cfg.step_spp, cfg.max_spp - done)
        ap = np.concatenate([pix[t] for t in active])
        for s in range(done, done + ns):  # sample order, one rounding per operation
            y = Y[s, ap]
            S1[ap] = S1[ap] + y
            S2[ap] = S2[ap] + y * y
        done += ns
        go_on = []
        for t in active:
            lhs, rhs = check_sides(S1[pix[t]], S2[pix[t]], done, cfg)
            if max(lhs, rhs) > 0.0:
                gap = min(gap, abs(lhs - rhs) / max(lhs, rhs))
            if lhs <= rhs or done >= cfg.max_spp:
                spp[t] = done
            else:
                go_on.append(t)
        active = go_on
    return spp, gap


def reference_moments(Y: np.ndarray, w: int, h: int, tile_spp: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(S1, S2) of every pixel after its tile's count of samples: Y[s] and Y[s]*Y[s] summed in sample
    order from 0.0, s = 0 .. n - 1 (the moment planes a result with these counts holds)."""
    Y = np.asarray(Y, dtype=np.float64)
    ty_n, tx_n = tile_grid(w, h)
    assert tile_spp.shape == (ty_n, tx_n)
    S1 = np.zeros(w * h)
    S2 = np.zeros(w * h)
    for ty in range(ty_n):
        for tx in range(tx_n):
            p = tile_pixels(w, h, tx, ty)
            for s in range(int(tile_spp[ty, tx])):
                y = Y[s, p]
                S1[p] = S1[p] + y
                S2[p] = S2[p] + y * y
    return S1, S2


def reference_resume(Y: np.ndarray, w: int, h: int, spp_in: np.ndarray, S1: np.ndarray, S2: np.ndarray,
                     cfg: ResumeConfig) -> tuple[np.ndarray, int, float, np.ndarray, np.ndarray]:
    """mfx_sample_adaptive_resume's rule (include/mafrix_rt.h) on a result with counts spp_in
    ((tiles_y, tiles_x)) and moment planes S1, S2 ((w*h,)); Y[s, x*h + y] is the luminance of the
    sample at offset s from B, the result's first sample (rows up to the largest count reached).
    Entry check: every tile at its own count n under cfg's threshold, active iff it fails and
    n < max_spp. A pass: every active tile gets cnt = min(step_spp, max_spp - n) samples, offsets
    n .. n + cnt - 1, added to S1 and S2 in sample order, then n += cnt and the tile is checked again.
    Passes repeat until no tile is active or max_passes passes have run.
    Returns (spp_out, active, gap, S1, S2): the new counts, the number of tiles that would go on
    (0 without a pass limit), the smallest relative gap between the two sides of the test at any
    check, the entry check included (as reference_tile_spp's), and the new moment planes (copies)."""
    Y = np.asarray(Y, dtype=np.float64)
    ty_n, tx_n = tile_grid(w, h)
    assert spp_in.shape == (ty_n, tx_n) and S1.shape == (w * h,) and S2.shape == (w * h,)
    spp = np.array(spp_in, dtype=np.int32)
    S1 = np.array(S1, dtype=np.float64)
    S2 = np.array(S2, dtype=np.float64)
    tiles = [(ty, tx) for ty in range(ty_n) for tx in range(tx_n)]
    pix = {t: tile_pixels(w, h, t[1], t[0]) for t in tiles}
    thr = AdaptiveConfig(2, 2, 1, cfg.rel_error, cfg.abs_floor)  # check_sides reads the threshold only
    gap = float("inf")

    def check(ts):
        nonlocal gap
        go_on = []
        for t in ts:
            n = int(spp[t])
            lhs, rhs = check_sides(S1[pix[t]], S2[pix[t]], n, thr)
            if max(lhs, rhs) > 0.0:
                gap = min(gap, abs(lhs - rhs) / max(lhs, rhs))
            if not (lhs <= rhs) and n < cfg.max_spp:
                go_on.append(t)
        return go_on

    active = check(tiles)
    passes = 0
    while active and (cfg.max_passes == 0 or passes < cfg.max_passes):
        for t in active:
            n = int(spp[t])
            cnt = min(cfg.step_spp, cfg.max_spp - n)
            p = pix[t]
            for s in range(n, n + cnt):  # sample order, one rounding per operation
                y = Y[s, p]
                S1[p] = S1[p] + y
                S2[p] = S2[p] + y * y
            spp[t] = n + cnt
        active = check(active)
        passes += 1
    return spp, len(active), gap, S1, S2


def reference_mean(frames: np.ndarray, tile_spp: np.ndarray, w: int, h: int) -> np.ndarray:
    """The image mfx_sample_adaptive (or a resume) must return for these counts: frames[s] is the one-sample image of
    global sample s as (w*h, >=3) x-major; a pixel is the sum of its first n samples in sample order
    (from 0.0, a black sample adding nothing) divided once by n, n its tile's count; alpha 1.0."""
    frames = np.asarray(frames, dtype=np.float64)
    ty_n, tx_n = tile_grid(w, h)
    assert tile_spp.shape == (ty_n, tx_n)
    out = np.zeros((w * h, 4))
    out[:, 3] = 1.0
    for ty in range(ty_n):
        for tx in range(tx_n):
            p = tile_pixels(w, h, tx, ty)
            n = int(tile_spp[ty, tx])
            acc = np.zeros((len(p), 3))
            for s in range(n):
                acc = acc + frames[s][p, :3]
            out[p, :3] = acc / float(n)
    return out
