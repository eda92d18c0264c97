"""A context gives back what it took (a GPU resource is a member of the context).

One process creates, uses and destroys contexts over and over: every call that allocates at its first
use runs in each cycle (render-ahead, mfx_sample's staging, adaptive sampling, the feature buffers and
the denoiser, a ray query, mfx_film_mean) and then the repeated-device path of a device list (its
staging buffer and events; no RCCL communicator). The device's free memory after cycle 24 is compared
with that after cycle 4, when the runtime is warm.

cube_cornell at 512x288: the smallest per-film buffer (the RGBA8 frame, 4 * npix = 576 KiB) leaked once
per cycle would lose 11.25 MiB over the 20 cycles; the bound allows half of that, 10 * 4 * npix =
5.6 MiB, on top of the runtime's own drift. That drift was measured by running this file three times
against the parent commit's library (the one with free_ctx's hand-kept lists, chosen with
MFX_LIB_PATH) on an MI355X: 0, 0 and 0 bytes (PARENT_DRIFTS; 308,239,400,960 bytes free after cycle 4
and after cycle 24 in every run), so the film is large enough to discriminate and the bound is 5.6 MiB.
"""
import numpy as np
import pytest

from conftest import SEED, scene

pytestmark = pytest.mark.gpu

W, H = 512, 288
CYCLES = 24
PARENT_DRIFTS = (0, 0, 0)  # free_after_4 - free_after_24 of three runs on the parent's library
BOUND = max(PARENT_DRIFTS) + 10 * 4 * W * H


def _cycle(a, rays):
    """One create / use / destroy of each kind of context; every call's output, in call order."""
    from mafrixraytracing_amd.native import NativeContext
    out = []
    with NativeContext(a, seed=SEED, render_ahead=8) as c:
        for _ in range(3):
            out.append(c.render_rgba8(1))
        out.append(c.sample(2))
        out.extend(c.sample_adaptive(2, 4, 2, 0.1, 1e-3))
        out.append(c.aov(1))
        out.extend(c.denoise(None, count=4.0, want_rgba=True))
        out.extend(c.closest_hit(rays))
        out.append(c.film_mean())
    with NativeContext(a, seed=SEED, devices=[0, 0]) as m:  # a repeated device: reduced by device-ordered adds
        m.trace_accumulate(2, 0)
        m.accum_reduce()
        out.append(m.accum_read_mean(2.0))
    return out


def test_contexts_give_back_their_memory(gpu):
    import torch
    a = scene("cube_cornell", W, H)
    rng = np.random.default_rng(7)
    rays = np.concatenate([np.tile([0.0, 0.0, -3.0], (64, 1)), rng.normal(size=(64, 3))], axis=1)
    torch.cuda.mem_get_info()  # the first call sets up torch's own share of the device
    first = last = None
    free = {}
    for k in range(1, CYCLES + 1):
        last = _cycle(a, rays)
        if k == 1:
            first = last
        if k in (4, CYCLES):
            torch.cuda.synchronize()
            free[k] = torch.cuda.mem_get_info()[0]
    drift = free[4] - free[CYCLES]
    print(f"lifetime: free after cycle 4 {free[4]} B, after cycle {CYCLES} {free[CYCLES]} B, drift {drift} B "
          f"(bound {BOUND} B)")
    assert len(first) == len(last)
    for x, y in zip(first, last):  # bit for bit (the bytes, so a NaN or a -0.0 compares as itself)
        assert x.shape == y.shape and np.array_equal(np.ravel(x).view(np.uint8), np.ravel(y).view(np.uint8))
    assert drift <= BOUND
