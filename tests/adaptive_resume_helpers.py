"""Shared by tests/test_adaptive_resume_reference.py and tests/test_gpu_adaptive_resume.py: the host
statement of mfx_sample_adaptive_resume (mafrixraytracing_amd/adaptive.py, reference_resume) applied to
the CPU oracle's one-sample frames, one pass at a time, so that a test can see every pass's tiles."""
import numpy as np

from denoise_var_helpers import oracle_sample_frames

_first = {}


def first_result(oracle, name, w, h, cfg):
    """(frames, Y, spp, S1, S2, gap) of mfx_sample_adaptive(cfg) on a fresh context: the oracle's
    one-sample frames 0 .. 63 (shared, read-only), their luminance, and the counts and moment planes
    the call leaves. Computed once per case."""
    from mafrixraytracing_amd.adaptive import luminance, reference_moments, reference_tile_spp
    key = (name.replace("@2l", ""), w, h, cfg)
    if key not in _first:
        frames = oracle_sample_frames(oracle, name, w, h, 64)
        Y = luminance(frames)
        Y.setflags(write=False)
        spp, gap = reference_tile_spp(Y[:cfg.max_spp], w, h, cfg)
        S1, S2 = reference_moments(Y, w, h, spp)
        for a in (spp, S1, S2):
            a.setflags(write=False)
        _first[key] = (frames, Y, spp, S1, S2, gap)
    return _first[key]


def one_pass_chain(Y, w, h, spp, S1, S2, rcfg):
    """reference_resume with max_passes = 1 repeated until nothing is active. Returns the list of
    (spp_before, spp_after, active) of every call (the last one runs no pass unless the budget ends
    the chain), the final (spp, S1, S2) and the smallest gap over all its checks."""
    from dataclasses import replace

    from mafrixraytracing_amd.adaptive import reference_resume
    one = replace(rcfg, max_passes=1)
    calls, gap = [], float("inf")
    while True:
        out, active, g, S1, S2 = reference_resume(Y, w, h, spp, S1, S2, one)
        gap = min(gap, g)
        calls.append((spp, out, active))
        spp = out
        if active == 0:
            return calls, (spp, S1, S2), gap


def added_paths_stats(o, spp_before, spp_after, w, h, seed):
    """The oracle's ray statistics over exactly the (pixel, sample) set a resume added: samples
    spp_before .. spp_after - 1 of every pixel of every tile."""
    from mafrixraytracing_amd.adaptive import tile_pixels
    px, py, ps = [], [], []
    for ty in range(spp_after.shape[0]):
        for tx in range(spp_after.shape[1]):
            p = tile_pixels(w, h, tx, ty)
            s = np.arange(int(spp_before[ty, tx]), int(spp_after[ty, tx]))
            px.append(np.repeat(p // h, len(s)))
            py.append(np.repeat(p % h, len(s)))
            ps.append(np.tile(s, len(p)))
    px, py, ps = np.concatenate(px), np.concatenate(py), np.concatenate(ps)
    if len(px) == 0:
        return (0, 0, 0)
    return tuple(int(v) for v in o.paths(px, py, ps, seed)[1][:3])
