"""The library's post (post_byte in mfx_trace_common.h: ACES curve, clamp, sqrt, 255.99 scale,
truncation) at the inputs where a one-ulp error moves a byte: tests/post_helpers.py's 510 windows of 16
consecutive doubles around every byte boundary of both branches of the curve, and the specials. Every
comparison is array_equal: the bytes are the CPU oracle's post of the same FP64 frame.

post_byte is inlined into four kernels in three translation units. Covered here at the boundaries:
k_dn_post (mfx_denoise.hip), reached through mfx_denoise and mfx_denoise_var from a host frame with
configurations that hand the frame on almost untouched, and adaptive_mean_kernel (mfx_kernels.hip),
reached through a caller-owned accumulator; film_post_kernel shares that translation unit, its flags and
the inlined function. The render-ahead batch post in mfx_wavefront.hip takes no caller data and stays
covered as before: its frames are compared with the film post's on natural inputs
(tests/test_gpu_render_ahead.py). tests/test_post_reference.py shows on the host that a contraction or a
reciprocal multiply in the chain changes bytes on these inputs, and none on uniform ones."""
import numpy as np
import pytest

from conftest import SEED, scene
from post_helpers import FILM, FRAME_SEED, ISOLATE, ISOLATE_VAR, boundary_frame, straddled_windows

pytestmark = pytest.mark.gpu

W, H = FILM


def _ctx(a, **kw):
    from mafrixraytracing_amd.native import NativeContext
    return NativeContext(a, seed=SEED, **kw)


@pytest.fixture(scope="module")
def framed():
    frame, slots = boundary_frame(W, H, FRAME_SEED)
    frame.setflags(write=False)
    return frame, slots


def test_dn_post_through_denoise(gpu, oracle, framed):
    from mafrixraytracing_amd.denoise import reference_denoise
    frame, slots = framed
    with _ctx(scene("cornell", W, H)) as ctx:
        feat = ctx.aov(1)
        got, rgba = ctx.denoise(frame, cfg=ISOLATE, want_rgba=True)
    ref = reference_denoise(frame, feat, W, H, ISOLATE)
    assert np.isfinite(ref).all()
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    assert np.array_equal(rgba, oracle.post_rgba8(got, W, H)), int((rgba != oracle.post_rgba8(got, W, H)).sum())
    assert straddled_windows(got, slots) == 510  # the inputs have not drifted off the boundaries


def test_dn_post_through_denoise_var(gpu, oracle, framed):
    from mafrixraytracing_amd.denoise import reference_denoise_var
    frame, slots = framed
    zeros = np.zeros(W * H)
    with _ctx(scene("cornell", W, H)) as ctx:
        feat = ctx.aov(1)
        got, rgba, gvar = ctx.denoise_var(frame, variance=zeros, cfg=ISOLATE_VAR, want_rgba=True, want_variance=True)
    ref, rvar = reference_denoise_var(frame, zeros, feat, W, H, ISOLATE_VAR)
    assert np.isfinite(ref).all() and np.isfinite(rvar).all()
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    assert np.array_equal(gvar, rvar)
    assert np.array_equal(rgba, oracle.post_rgba8(got, W, H)), int((rgba != oracle.post_rgba8(got, W, H)).sum())
    assert straddled_windows(got, slots) == 510


def test_adaptive_mean_post_through_an_attached_accumulator(gpu, oracle, framed):
    """A caller-owned accumulator, worked on in place: after an adaptive result with n = 2 in every tile
    the caller overwrites it with 2*x (exact, so accum / n is x to the bit), and a resume whose budget
    every tile has reached runs no pass but still launches adaptive_mean_kernel on the accumulator."""
    import torch
    frame, slots = framed
    npix = W * H
    planes = np.ascontiguousarray(frame[:, :3].T)  # plane-major, x-major pixels: accum[c*npix + x*h + y]
    with _ctx(scene("cornell", W, H)) as ctx:
        acc = torch.zeros(3 * npix, dtype=torch.float64, device="cuda:0")
        ctx.accum_attach(acc.data_ptr(), acc.numel() * acc.element_size())
        try:
            _, tiles = ctx.sample_adaptive(2, 2, 1, 0.25, 0.01)
            assert (tiles == 2).all()
            ctx.sync()
            acc.copy_(torch.from_numpy(planes.reshape(-1)).to("cuda:0") * 2.0)
            torch.cuda.synchronize()
            assert np.array_equal(acc.cpu().numpy().reshape(3, npix) / 2.0, planes)
            got, tiles, rgba, active = ctx.sample_adaptive_resume(2, 1, 0.25, 0.01, want_rgba=True)
            rays = ctx.ray_counts()
            ctx.sync()
        finally:
            ctx.accum_attach(None)  # before the tensor dies
    assert active == 0 and (tiles == 2).all()
    assert np.array_equal(rays, np.zeros(16))  # no pass ran
    assert np.array_equal(got, frame)
    assert np.array_equal(rgba, oracle.post_rgba8(frame, W, H)), int((rgba != oracle.post_rgba8(frame, W, H)).sum())
    assert straddled_windows(got, slots) == 510
