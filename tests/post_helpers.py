"""Shared by tests/test_post_reference.py and tests/test_gpu_post_boundaries.py: a numpy statement of
the post chain (ACES curve, clamp, sqrt, 255.99 scale, truncation: the oracle's oracle_post_rgba8, the
library's post_byte), the inputs at which a one-ulp error in that chain moves a byte, a frame that
carries them, and the denoiser configurations that hand such a frame to the post almost untouched.

Eight roundings precede the truncation, so a contraction, a reciprocal multiply or a shortened sqrt
changes a byte only where the value sits on a byte boundary; natural frames never do. The chain is not
monotone at the ulp level, so two doubles beside each crossing are not enough: each boundary gets a
window of 16 consecutive doubles around it."""
from fractions import Fraction

import numpy as np

import conftest  # noqa: F401  (puts the repository root on sys.path)
from mafrixraytracing_amd.denoise import DenoiseConfig, DenoiseVarConfig

A, B, C, D, E = 2.51, 0.03, 2.43, 0.59, 0.14  # Scene.fs:280-289
WINDOW = 16   # doubles per window
BELOW = 7     # of them, those before the pair's lower one
SPECIALS = (0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-3, 1.0, -1.0, 100.0, 1e6, -1e6, 1e150, -1e150)
# (non-finite values and |x| > 1e150 are left out: there the curve is inf/inf, and the oracle's (int)NaN
# is undefined C)


# ---- the chain ----------------------------------------------------------------------------------------
def _tail(col):
    """clamp01, sqrt, 255.99 scale, (uint8)(int): what follows the division."""
    col = np.where(col < 0.0, 0.0, np.where(col > 1.0, 1.0, col))
    return (255.99 * np.sqrt(col)).astype(np.int32).astype(np.uint8)


def post_bytes(x):
    """The byte of every channel value in x (any shape), in oracle_post_rgba8's operation order: FP64,
    one rounding per operation."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        num = x * (A * x + B)
        den = x * (C * x + D) + E
        return _tail(num / den)


def post_rgba8(frame, w, h):
    """oracle.post_rgba8's output from post_bytes: (w*h, >=3) x-major in, w*h*4 bytes y-major out."""
    b = post_bytes(np.asarray(frame, dtype=np.float64)[:, :3]).reshape(w, h, 3)
    out = np.full((h, w, 4), 255, dtype=np.uint8)
    out[..., :3] = b.transpose(1, 0, 2)
    return out.reshape(-1)


def _fma(a, b, c):
    """fma(a, b, c) of finite doubles, exactly: the rational a*b + c rounded once (int / int is correctly
    rounded, so is float(Fraction))."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _chain(x, num_of, den_of, div):
    x = np.asarray(x, dtype=np.float64)
    flat = [float(v) for v in x.ravel()]
    num = np.array([num_of(v) for v in flat])
    den = np.array([den_of(v) for v in flat])
    with np.errstate(all="ignore"):
        return _tail(div(num, den)).reshape(x.shape)


def _num(v):
    return v * (A * v + B)


def _den(v):
    return v * (C * v + D) + E


# What a compiler or a "fast" rewrite would make of the chain, one liberty each. name -> post_bytes' twin.
MUTANTS = {
    # a*x + b contracted to one fma
    "fma_num": lambda x: _chain(x, lambda v: v * _fma(A, v, B), _den, lambda n, d: n / d),
    # x*(c*x + d) + e contracted: the inner and the outer multiply-add are one fma each
    "fma_den": lambda x: _chain(x, _num, lambda v: _fma(v, _fma(C, v, D), E), lambda n, d: n / d),
    # n * (1/d) instead of n / d
    "rcp_div": lambda x: _chain(x, _num, _den, lambda n, d: n * (1.0 / d)),
}


# ---- the inputs ---------------------------------------------------------------------------------------
def _crossings(lo, hi):
    """For k = 1..255 the adjacent pair of doubles (below, at_least) with post_bytes(below) < k <=
    post_bytes(at_least), bisected by value midpoints from (lo, hi) until the midpoint is one of the two.
    (The chain is not monotone at the ulp level, so there can be several such pairs within a few dozen
    ulps; this is the one the midpoints from these starting points reach.)"""
    k = np.arange(1, 256)
    a, b = np.full(255, float(lo)), np.full(255, float(hi))
    assert (post_bytes(a) < k).all() and (post_bytes(b) >= k).all()
    while True:
        mid = (a + b) / 2
        move = (mid != a) & (mid != b)
        if not move.any():
            return a, b
        up = post_bytes(mid) >= k
        b = np.where(move & up, mid, b)
        a = np.where(move & ~up, mid, a)


_values = None


def boundary_values():
    """(values, window): 510 windows of 16 consecutive doubles, each starting 7 doubles before the lower
    one of the pair at which the byte first reaches k = 1..255 (window j: k = j % 255 + 1; j < 255 on the
    positive branch, bisected from [0, 100], the last crossing near 5.864; j >= 255 on the negative branch,
    bisected from [-0.03/2.51, -100]: the unclamped cosine makes negative radiance real, and below -0.012
    the curve rises again, its crossings in about [-0.2399, -0.01202]), then SPECIALS with window -1.
    8,173 values. Computed once and left unchanged."""
    global _values
    if _values is None:
        vals, win = [], []
        for j0, (lo, hi) in enumerate(((0.0, 100.0), (-B / A, -100.0))):
            below, _ = _crossings(lo, hi)
            # magnitudes of one sign order as their bit patterns do; in order of magnitude `below` is the
            # window's entry 7 and its partner entry 8 on both branches (for x < 0 that is the same set
            # as 7 doubles below the pair's lower one and 8 above)
            first = np.abs(below).view(np.int64) - BELOW
            bits = first[:, None] + np.arange(WINDOW)[None, :]
            vals.append(np.copysign(bits.view(np.float64), lo if lo else 1.0).ravel())
            win.append(np.repeat(np.arange(255) + 255 * j0, WINDOW))
        vals.append(np.array(SPECIALS))
        win.append(np.full(len(SPECIALS), -1))
        v, wdw = np.concatenate(vals), np.concatenate(win)
        v.setflags(write=False)
        wdw.setflags(write=False)
        _values = (v, wdw)
    return _values


def window_k(j):
    return j % 255 + 1


def boundary_frame(w, h, seed):
    """(frame, slots): a (w*h, 4) x-major frame, alpha 1.0, whose 3*w*h channel slots (slot = 3*pixel +
    channel) hold boundary_values() in a seeded shuffle, the rest filled with repeats of them;
    slots[i] is the slot of value i."""
    vals, _ = boundary_values()
    n = 3 * w * h
    assert n >= len(vals)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    slots = perm[:len(vals)]
    chan = np.empty(n)
    chan[slots] = vals
    chan[perm[len(vals):]] = vals[rng.integers(0, len(vals), n - len(vals))]
    frame = np.ones((w * h, 4))
    frame[:, :3] = chan.reshape(w * h, 3)
    return frame, slots


def at_slots(frame, slots):
    """The channel values of a (w*h, >=3) frame at boundary_frame's slots."""
    return np.asarray(frame)[:, :3].reshape(-1)[slots]


def straddled_windows(frame, slots):
    """How many of the 510 windows still straddle their boundary in `frame`: among the bytes of the
    window's 16 values as the frame now holds them, both k-1 and k occur."""
    _, win = boundary_values()
    b = post_bytes(at_slots(frame, slots)).astype(np.int64)
    n = 0
    for j in range(510):
        got = b[win == j]
        k = window_k(j)
        n += int((got == k - 1).any() and (got == k).any())
    return n


# ---- the isolating configurations ---------------------------------------------------------------------
# mfx_denoise as (almost) the identity: one iteration, no feature terms, and a colour term whose
# sc2 = 1e-160^2 is the subnormal 1e-320, so a tap whose colour differs at all gets a weight of at most
# about 1e-288 (exactly 0 where d2 / sc2 overflows). The pixel comes out as (9/64 * C) / (9/64).
ISOLATE = DenoiseConfig(iterations=1, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, sigma_color=1e-160)
# The same for mfx_denoise_var, used with a variance plane of zeros: lden = 1.0 * 0 + 1e-300.
ISOLATE_VAR = DenoiseVarConfig(iterations=1, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, sigma_luma=1.0,
                               luma_floor=1e-300)

FILM = (62, 45)  # 8,370 slots; both sides leave edge tiles
FRAME_SEED = 1


def random_features(n, seed=2):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1.0, 1.0, (n, 8))
    f[:, 3] = rng.uniform(0.5, 9.0, n)
    return f
