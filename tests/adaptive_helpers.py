"""Shared by the GPU tests of mfx_sample_adaptive (tests/test_gpu_adaptive.py, test_gpu_path_depth.py,
test_gpu_rng_keys.py): what the call must return, from the rule stated on the host
(mafrixraytracing_amd/adaptive.py) applied to the CPU oracle's one-sample frames, and the comparison."""
import numpy as np

from conftest import SEED, scene

_frames = {}
_refs = {}


def reference(oracle, name, w, h, cfg, depth=3, seed=SEED):
    """(tile_spp, mean, rgba8, ray statistics) the call must return: computed once per case, shared."""
    from mafrixraytracing_amd.adaptive import luminance, reference_mean, reference_tile_spp, tile_pixels
    world = name.replace("@2l", "")  # the same world scene however it is traced
    key = (world, w, h, cfg, depth, seed)
    if key in _refs:
        return _refs[key]
    o = oracle.OracleScene(scene(world, w, h, max_depth=depth))
    fk = (world, w, h, depth, seed)
    if fk not in _frames or len(_frames[fk]) < cfg.max_spp:
        f = np.stack([o.sample(1, seed, sample_base=s) for s in range(max(32, cfg.max_spp))])
        f.setflags(write=False)
        _frames[fk] = f
    frames = _frames[fk][:cfg.max_spp]
    spp, gap = reference_tile_spp(luminance(frames), w, h, cfg)
    print(f"{name} {w}x{h} depth {depth} seed {seed:#x} {cfg}: smallest gap {gap:.3g}, mean spp {spp.mean():.2f}")
    assert gap > 1e-6, (name, gap)  # the condition on the inputs: no tile near a tie
    mean = reference_mean(frames, spp, w, h)
    px, py, ps = [], [], []
    for ty in range(spp.shape[0]):
        for tx in range(spp.shape[1]):
            p = tile_pixels(w, h, tx, ty)
            n = int(spp[ty, tx])
            px.append(np.repeat(p // h, n))
            py.append(np.repeat(p % h, n))
            ps.append(np.tile(np.arange(n), len(p)))
    st = o.paths(np.concatenate(px), np.concatenate(py), np.concatenate(ps), seed)[1][:3]
    r = (spp, mean, oracle.post_rgba8(mean, w, h), st)
    for a in r:
        a.setflags(write=False)
    _refs[key] = r
    return r


def run(ctx, cfg, want_rgba=True):
    return ctx.sample_adaptive(cfg.min_spp, cfg.max_spp, cfg.step_spp, cfg.rel_error, cfg.abs_floor, want_rgba=want_rgba)


def check_parity(ctx, ref, what=""):
    """ref: reference(...) + (cfg,). Every output of the call equals it, bit for bit."""
    spp, mean, rgba, st = ref[:4]
    cfg = ref[4]
    frame, tiles, out8 = run(ctx, cfg)
    c = ctx.ray_counts()
    assert np.array_equal(tiles, spp), (what, tiles.tolist(), spp.tolist())
    assert np.array_equal(frame, mean), (what, np.abs(frame - mean).max())
    assert np.array_equal(frame[:, 3], np.ones(len(frame)))
    assert np.array_equal(out8, rgba), what
    assert (c[0], c[1], c[2]) == (st[0], st[1], st[2]), (what, c[:3], st)
    assert c[3] == c[0]
    return frame, tiles, out8, c
