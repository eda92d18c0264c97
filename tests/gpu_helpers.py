"""Shared by tests/test_gpu_path_depth.py and tests/test_gpu_rng_keys.py: a context created under
environment settings, cached oracle frames, and the comparisons both files repeat."""
import os

import numpy as np

from conftest import SEED, scene

# tests/test_gpu_ray_queue.py's QCHUNKS: the default chunks, and small queue / large pool chunks
QCHUNKS = [{}, {"MFX_QCHUNK": "64", "MFX_CHUNK": "1024"}]

_frames = {}


def ctx_env(a, env=None, seed=SEED, **kw):
    """A NativeContext created with `env` set (the library reads its variables at context creation)."""
    from mafrixraytracing_amd.native import NativeContext
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return NativeContext(a, seed=seed, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def oracle_frame(oracle, name, w, h, depth, spp, base=0, seed=SEED):
    """(the oracle's Sample(spp) from global sample `base`, its ray counts [0..2]); computed once per
    case and left unchanged."""
    world = name.replace("@2l", "")  # the same world scene however it is traced
    key = (world, w, h, depth, spp, base, seed)
    if key not in _frames:
        f, st = oracle.OracleScene(scene(world, w, h, max_depth=depth)).sample(spp, seed, sample_base=base, with_stats=True)
        f.setflags(write=False)
        _frames[key] = (f, tuple(st[:3]))
    return _frames[key]


def assert_frame(ctx, img, ref, what=""):
    """img and the context's last ray counts equal an oracle_frame, bit for bit."""
    frame, st = ref
    c = ctx.ray_counts()
    assert (c[0], c[1], c[2]) == st, (what, c[:3], st)
    assert np.array_equal(img, frame), (what, int(np.any(img != frame, axis=1).sum()), np.abs(img - frame).max())


def assert_megakernel_frame(ctx, img, ref, spp, what=""):
    """tests/test_gpu_parity.py's rule for the megakernel: bit for bit at one sample per pixel; above,
    its FP64 atomics add a pixel's paths in arrival order: within 1e-12 * max(1, |ref|max), inside
    the 1e-4 per-channel RMSE gate. Ray counts equal either way."""
    frame, st = ref
    c = ctx.ray_counts()
    assert (c[0], c[1], c[2]) == st, (what, c[:3], st)
    diff = np.abs(img[:, :3] - frame[:, :3])
    assert np.all(np.sqrt((diff ** 2).mean(axis=0)) <= 1e-4), what
    if spp == 1:
        assert np.array_equal(img, frame), (what, diff.max())
    else:
        assert diff.max() <= 1e-12 * max(1.0, np.abs(frame).max()), (what, diff.max())
    assert np.all(img[:, 3] == 1.0)


def assert_render_ahead(oracle, ctx, name, w, h, depth, calls, seed=SEED):
    """`calls` one-sample render calls against the oracle's Film.AddSample + post, byte for byte, and the
    film (tests/test_gpu_render_ahead.py test_render_ahead_matches_oracle_film)."""
    from mafrixraytracing_amd.abi import dptr
    npix = w * h
    accum, target, fc = np.zeros((npix, 4)), np.zeros((npix, 4)), np.zeros(1)
    for k in range(calls):
        rgba = ctx.render_rgba8(1)
        fr = np.array(oracle_frame(oracle, name, w, h, depth, 1, k, seed)[0])
        oracle.lib().oracle_film_add(dptr(accum), dptr(target), dptr(fc), dptr(fr), npix)
        assert np.array_equal(rgba, oracle.post_rgba8(target, w, h)), (name, depth, k)
    assert np.array_equal(ctx.film_mean()[:, :3], target[:, :3]), (name, depth)
