"""k_atrous and k_atrous_var at the host inputs that rendered frames never bring: a dynamic range of 300
decades, differences whose squares overflow, neighbours that are exactly equal, weights that underflow to
subnormals and to 0, a step past the film on every side (iterations = 8), and variance planes of zeros,
1e-300 and 1e300. Cornell at 44x36 (edge tiles on both sides, seven blocks) and at 5x3 (every tap row and
column cut), features from mfx_aov. Every comparison is array_equal against the numpy statement of the
rule (mafrixraytracing_amd/denoise.py) on the same frame and features: the frame, the variance and the
RGBA8 post. Before the GPU is asked, each case asserts on the host that the reference is finite and that
the input does what the case is named for."""
import numpy as np
import pytest

from conftest import SEED, scene

pytestmark = pytest.mark.gpu

FILMS = [(44, 36), (5, 3)]
K = (0.375, 0.25, 0.0625)


@pytest.fixture(scope="module", params=FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
def film(gpu, request):
    """One context per film for the module: (ctx, w, h, features of aov(4), the 4-spp frame)."""
    from mafrixraytracing_amd.native import NativeContext
    w, h = request.param
    with NativeContext(scene("cornell", w, h), seed=SEED) as ctx:
        feat = ctx.aov(4)
        frame = ctx.sample(4)
        feat.setflags(write=False)
        frame.setflags(write=False)
        yield ctx, w, h, feat, frame


def _cfg(**kw):
    from mafrixraytracing_amd.denoise import DenoiseConfig
    return DenoiseConfig(**kw)


def _vcfg(**kw):
    from mafrixraytracing_amd.denoise import DenoiseVarConfig
    return DenoiseVarConfig(**kw)


def _rgba_frame(rgb):
    f = np.ones((len(rgb), 4))
    f[:, :3] = rgb
    return f


def _decades(n, seed, top):
    """(n, 4) frame whose channels are +-10^U(-top, top)."""
    rng = np.random.default_rng(seed)
    return _rgba_frame(rng.choice([-1.0, 1.0], (n, 3)) * 10.0 ** rng.uniform(-top, top, (n, 3)))


def _check(film, oracle, frame, cfg, post=True):
    from mafrixraytracing_amd.denoise import reference_denoise
    ctx, w, h, feat, _ = film
    ref = reference_denoise(frame, feat, w, h, cfg)
    assert np.isfinite(ref).all(), cfg
    got, rgba = ctx.denoise(frame, cfg=cfg, want_rgba=True)
    assert np.array_equal(got, ref), (cfg, int((got != ref).sum()))
    if post:
        assert np.array_equal(rgba, oracle.post_rgba8(ref, w, h)), cfg


def _check_var(film, oracle, frame, var, cfg, post=True):
    from mafrixraytracing_amd.denoise import reference_denoise_var
    ctx, w, h, feat, _ = film
    ref, rvar = reference_denoise_var(frame, var, feat, w, h, cfg)
    assert np.isfinite(ref).all() and np.isfinite(rvar).all(), cfg
    got, rgba, gvar = ctx.denoise_var(frame, variance=var, cfg=cfg, want_rgba=True, want_variance=True)
    assert np.array_equal(got, ref), (cfg, int((got != ref).sum()))
    assert np.array_equal(gvar, rvar), (cfg, int((gvar != rvar).sum()))
    if post:
        assert np.array_equal(rgba, oracle.post_rgba8(ref, w, h)), cfg


def _taps(w, h, step=1):
    """For each of the 25 taps (dy outer, dx inner): (dx, dy, ok, xq, yq) as the rule walks them."""
    X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            xq, yq = X + dx * step, Y + dy * step
            ok = (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
            yield dx, dy, ok, np.clip(xq, 0, w - 1), np.clip(yq, 0, h - 1)


def _first_iteration_d2(frame, w, h):
    """d2(C_p, C_q) of the first iteration's taps inside the film, in the rule's order of operations."""
    from mafrixraytracing_amd.denoise import _d2
    C = np.asarray(frame)[:, :3].reshape(w, h, 3)
    with np.errstate(over="ignore"):
        return np.concatenate([_d2(C, C[xq, yq])[ok] for dx, dy, ok, xq, yq in _taps(w, h)])


def _first_iteration_weights(feat, w, h, cfg):
    """wt of the first iteration's taps inside the film from the feature terms alone (normal, depth,
    albedo, in the rule's order and operations)."""
    from mafrixraytracing_amd.denoise import _d2
    F = np.asarray(feat).reshape(w, h, -1)
    N, Z, A = F[..., 0:3], F[..., 3], F[..., 4:7]
    out = []
    with np.errstate(all="ignore"):
        for dx, dy, ok, xq, yq in _taps(w, h):
            g = np.ones((w, h))
            if cfg.sigma_normal > 0:
                g = g * (1.0 / (1.0 + _d2(N, N[xq, yq]) / (cfg.sigma_normal * cfg.sigma_normal)))
            if cfg.sigma_depth > 0:
                Zq = Z[xq, yq]
                dz = Z - Zq
                dd = (cfg.sigma_depth * cfg.sigma_depth) * (Z * Z + Zq * Zq)
                pos = dd > 0
                g = g * (1.0 / (1.0 + np.where(pos, (dz * dz) / np.where(pos, dd, 1.0), 0.0)))
            if cfg.sigma_albedo > 0:
                g = g * (1.0 / (1.0 + _d2(A, A[xq, yq]) / (cfg.sigma_albedo * cfg.sigma_albedo)))
            out.append(((K[abs(dx)] * K[abs(dy)]) * g)[ok])
    return np.concatenate(out)


TINY = np.finfo(np.float64).tiny  # the smallest normal double


# ---- dynamic range --------------------------------------------------------------------------------------
def test_dynamic_range(film, oracle):
    """Channels +-10^U(-150, 150): every product and sum of the filter and of the post stays finite
    (|x| <= 1e150, so d2 <= 1.2e301 and the post's x*(a*x + b) <= 2.6e300), and the colour term's weight
    spans the whole exponent range."""
    _, w, h, _, _ = film
    frame = _decades(w * h, 21, 150)
    frame[0, 0], frame[1, 1], frame[2, 2] = 1e150, -1e150, 1e-150  # both ends of the range, in neighbours
    d2 = _first_iteration_d2(frame, w, h)
    assert np.isfinite(d2).all() and d2.max() >= 1e300
    g = 1.0 / (1.0 + d2)
    assert (g > 0).all() and g.min() <= 1e-300 and (g == 1.0).any()  # 300 decades of weights; the centre taps
    _check(film, oracle, frame, _cfg())
    _check(film, oracle, frame, _cfg(sigma_color=1.0))
    var = np.random.default_rng(22).uniform(0.0, 0.05, w * h)
    _check_var(film, oracle, frame, var, _vcfg())


def test_overflowing_differences(film, oracle):
    """Channels +-10^U(-160, 160): (a - b)*(a - b) overflows, d2 is inf, 1 / (1 + inf) is exactly 0 and
    the tap adds 0 * C_q = 0. The post is not asked for: its x*x overflows above about 1e154, the curve is
    inf/inf there and the oracle's (int)NaN is undefined C."""
    _, w, h, _, _ = film
    frame = _decades(w * h, 23, 160)
    d2 = _first_iteration_d2(frame, w, h)
    assert np.isinf(d2).any() and not np.isnan(d2).any()
    _check(film, oracle, frame, _cfg(sigma_color=1.0), post=False)
    _check(film, oracle, frame, _cfg(iterations=5, sigma_color=1.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
           post=False)
    # the luminance term: dl*dl overflows the same way
    _check_var(film, oracle, frame, np.full(w * h, 0.01), _vcfg(), post=False)


# ---- exactly equal neighbours ---------------------------------------------------------------------------
def test_exactly_equal_neighbours(film, oracle):
    """8x8 blocks of one colour each with one 1e150 outlier per block: with sigma_color = 1e-3 a tap's
    colour weight is exactly 1 (d2 = 0) or almost 0."""
    _, w, h, _, _ = film
    rng = np.random.default_rng(24)
    bx, by = (w + 7) // 8, (h + 7) // 8
    colour = rng.uniform(0.0, 2.0, (bx, by, 3))
    X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    rgb = colour[X >> 3, Y >> 3]
    for i in range(bx):
        for j in range(by):
            x = min(i * 8 + int(rng.integers(0, 8)), w - 1)
            y = min(j * 8 + int(rng.integers(0, 8)), h - 1)
            rgb[x, y, int(rng.integers(0, 3))] = 1e150
    frame = _rgba_frame(rgb.reshape(w * h, 3))
    d2 = _first_iteration_d2(frame, w, h)
    assert (d2 == 0.0).mean() > 0.5 and (d2 >= 9e299).any() and np.isfinite(d2).all()
    for cfg in (_cfg(sigma_color=1e-3), _cfg(sigma_color=1e-3, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)):
        _check(film, oracle, frame, cfg)
    # the luminance term with the smallest floor and no variance: dl = 0 exactly, or a weight of almost 0
    _check_var(film, oracle, frame, np.zeros(w * h), _vcfg(luma_floor=1e-300))


# ---- underflowing weights -------------------------------------------------------------------------------
def test_underflowing_weights(film, oracle):
    """sigma_normal = 1e-150 and sigma_albedo = 1e-5 push a tap across a wall to a subnormal weight;
    sigma_depth = 1e-10 on top pushes it to exactly 0."""
    _, w, h, feat, frame = film
    sub = _cfg(sigma_normal=1e-150, sigma_albedo=1e-5)
    zero = _cfg(sigma_normal=1e-150, sigma_albedo=1e-5, sigma_depth=1e-10)
    wt = _first_iteration_weights(feat, w, h, sub)
    assert ((wt > 0) & (wt < TINY)).any() and (wt >= 1.0 / 256.0).any()
    wt = _first_iteration_weights(feat, w, h, zero)
    assert (wt == 0.0).any() and (wt >= 1.0 / 256.0).any()
    var = np.random.default_rng(25).uniform(0.0, 0.05, w * h)
    for cfg in (sub, zero):
        _check(film, oracle, frame, cfg)
        _check_var(film, oracle, frame, var, _vcfg(sigma_normal=cfg.sigma_normal, sigma_depth=cfg.sigma_depth,
                                                   sigma_albedo=cfg.sigma_albedo))


# ---- a step past the film on every side -----------------------------------------------------------------
def test_eight_iterations(film, oracle):
    """Step 128 passes every edge of both films: only the centre tap is left, out = (9/64 C) / (9/64)."""
    _, w, h, _, frame = film
    assert 128 >= max(w, h)
    var = np.random.default_rng(26).uniform(0.0, 0.05, w * h)
    var[::5] = 0.0
    for cfg in (_cfg(iterations=8), _cfg(iterations=8, sigma_color=1.0)):
        _check(film, oracle, frame, cfg)
    for cfg in (_vcfg(iterations=8), _vcfg(iterations=8, sigma_luma=0.0)):
        _check_var(film, oracle, frame, var, cfg)
    _check(film, oracle, _decades(w * h, 27, 150), _cfg(iterations=8, sigma_color=1.0))


# ---- variance planes ------------------------------------------------------------------------------------
def test_variance_planes(film, oracle):
    """All zeros; zeros mixed with 1e-300 and 1e300; the smallest luma_floor with each."""
    _, w, h, _, frame = film
    rng = np.random.default_rng(28)
    mixed = rng.choice([0.0, 1e-300, 1e300], w * h)
    assert all((mixed == v).any() for v in (0.0, 1e-300, 1e300))
    for var in (np.zeros(w * h), mixed):
        for cfg in (_vcfg(), _vcfg(luma_floor=1e-300), _vcfg(iterations=5, luma_floor=1e-300, sigma_luma=1e-170)):
            _check_var(film, oracle, frame, var, cfg)
