"""The post chain at its byte boundaries, host side (no GPU): the numpy statement of the chain equals the
CPU oracle's post, the boundary inputs (tests/post_helpers.py) survive the isolating denoiser
configurations on their way to the post kernels, and a contraction or a reciprocal multiply anywhere in
the chain changes bytes on them. The last is what shows that tests/test_gpu_post_boundaries.py can fail."""
import numpy as np
import pytest

from post_helpers import (FILM, FRAME_SEED, ISOLATE, ISOLATE_VAR, MUTANTS, SPECIALS, at_slots, boundary_frame,
                          boundary_values, post_bytes, post_rgba8, random_features, straddled_windows, window_k)

W, H = FILM


@pytest.fixture(scope="module")
def framed():
    frame, slots = boundary_frame(W, H, FRAME_SEED)
    frame.setflags(write=False)
    return frame, slots


@pytest.fixture(scope="module")
def filtered(framed):
    """The frame after reference_denoise with ISOLATE and after reference_denoise_var with ISOLATE_VAR and
    a variance plane of zeros, on seeded random features (every feature sigma is 0: they are not read)."""
    from mafrixraytracing_amd.denoise import reference_denoise, reference_denoise_var
    frame, _ = framed
    feat = random_features(W * H)
    plain = reference_denoise(frame, feat, W, H, ISOLATE)
    var, vout = reference_denoise_var(frame, np.zeros(W * H), feat, W, H, ISOLATE_VAR)
    return plain, var, vout


def test_boundary_values():
    vals, win = boundary_values()
    assert len(vals) == 510 * 16 + len(SPECIALS) == 8173
    assert np.isfinite(vals).all() and (np.abs(vals) <= 1e150).all()
    b = post_bytes(vals).astype(int)
    unsorted = 0
    for j in range(510):
        v, k = vals[win == j], window_k(j)
        bits = np.abs(v).view(np.int64)
        assert len(v) == 16 and (np.diff(bits) == 1).all()  # consecutive doubles
        assert (v > 0).all() if j < 255 else (v < 0).all()
        got = b[win == j]
        assert got[7] < k <= got[8]  # the bisected pair
        assert set(got) <= {k - 1, k}
        unsorted += int((np.diff(got) < 0).any())
    print(f"windows whose bytes are not sorted: {unsorted} of 510")
    assert unsorted > 0  # the chain is not monotone at the ulp level: the reason for windows
    assert 5.86 < vals[win == 254][7] < 5.87
    assert -0.2399 < vals[win == 509][7] and vals[win == 255][7] < -0.01201


def test_boundary_frame(framed):
    frame, slots = framed
    vals, _ = boundary_values()
    assert frame.shape == (W * H, 4) and 3 * W * H == 8370
    assert len(set(slots.tolist())) == len(vals) and slots.min() >= 0 and slots.max() < 3 * W * H
    assert np.array_equal(at_slots(frame, slots).view(np.int64), vals.view(np.int64))  # the bits, -0.0 included
    assert np.array_equal(frame[:, 3], np.ones(W * H))
    assert np.isin(frame[:, :3], vals).all()  # the rest: repeats
    assert straddled_windows(frame, slots) == 510
    again, s2 = boundary_frame(W, H, FRAME_SEED)
    assert np.array_equal(again, frame) and np.array_equal(s2, slots)


def test_numpy_statement_equals_the_oracle(oracle, framed, filtered):
    frame, _ = framed
    for f in (frame,) + filtered[:2]:
        assert np.array_equal(post_rgba8(f, W, H), oracle.post_rgba8(f, W, H))
    rng = np.random.default_rng(5)
    nat = np.ones((W * H, 4))
    nat[:, :3] = rng.uniform(-0.5, 3.0, (W * H, 3))
    assert np.array_equal(post_rgba8(nat, W, H), oracle.post_rgba8(nat, W, H))


def test_isolation_keeps_every_window_on_its_boundary(framed, filtered):
    """What the GPU test's inputs rest on: after the reference filter all 510 windows still hold both
    bytes k-1 and k. (The share of channels that come back bit-identical is printed, not asserted.)"""
    frame, slots = framed
    plain, var, vout = filtered
    for name, f in (("ISOLATE", plain), ("ISOLATE_VAR", var)):
        assert np.isfinite(f).all(), name
        same = float((f[:, :3] == frame[:, :3]).mean())
        n = straddled_windows(f, slots)
        print(f"{name}: {same:.4f} of the channels bit-identical, {n} of 510 windows straddled")
        assert n == 510, name
    assert np.array_equal(vout, np.zeros(W * H))


def test_every_mutant_changes_bytes(framed, filtered):
    """An exact fma in a*x + b, exact fmas in x*(c*x + d) + e, and n * (1/d) for n / d: each changes at
    least one byte on the filtered boundary values, and (printed only) next to none on uniform ones."""
    _, slots = framed
    uniform = np.random.default_rng(6).uniform(0.0, 3.0, 20000)
    for fname, f in (("ISOLATE", filtered[0]), ("ISOLATE_VAR", filtered[1])):
        chan = f[:, :3].reshape(-1)
        want = post_bytes(chan)
        for name, mutant in MUTANTS.items():
            changed = int((mutant(chan) != want).sum())
            print(f"{fname}, {name}: {changed} of {len(chan)} bytes changed")
            assert changed >= 1, (fname, name)
    want = post_bytes(uniform)
    for name, mutant in MUTANTS.items():
        print(f"uniform [0, 3), {name}: {int((mutant(uniform) != want).sum())} of {len(uniform)} bytes changed")
