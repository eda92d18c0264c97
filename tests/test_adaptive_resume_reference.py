"""The host statement of mfx_sample_adaptive_resume (mafrixraytracing_amd/adaptive.py,
reference_resume) against the one-call rule (reference_tile_spp), on seeded synthetic luminances and on
the CPU oracle's one-sample frames of the cornell 44x36 film: a call equals its first pass followed by
a resume, and the chain of one-pass resumes; a repeated resume, a looser threshold and a budget below
a tile's count change nothing; and hand-made cases on one 5x3 tile whose counts can be written down.
Every comparison of counts and moments is array_equal."""
import numpy as np
import pytest

from adaptive_resume_helpers import first_result, one_pass_chain

W, H = 44, 36


def _synthetic(w, h, n, seed):
    """Tiles of differing noise around differing means, so that they stop at differing counts."""
    from mafrixraytracing_amd.adaptive import tile_grid, tile_pixels
    rng = np.random.default_rng(seed)
    Y = np.empty((n, w * h))
    ty_n, tx_n = tile_grid(w, h)
    for ty in range(ty_n):
        for tx in range(tx_n):
            p = tile_pixels(w, h, tx, ty)
            mean, noise = rng.uniform(0.2, 2.0), rng.uniform(0.05, 3.0)
            Y[:, p] = mean + noise * rng.standard_normal((n, len(p)))
    return Y


def _cases(oracle):
    from mafrixraytracing_amd.adaptive import AdaptiveConfig
    out = []
    for seed, (w, h), cfg in [(1, (44, 36), AdaptiveConfig(4, 32, 4, 0.25, 0.01)), (2, (19, 9), AdaptiveConfig(2, 30, 8, 0.2, 0.0)),
                              (3, (16, 16), AdaptiveConfig(3, 17, 5, 0.3, 0.05))]:
        out.append((f"synthetic{seed}", _synthetic(w, h, 64, seed), w, h, cfg))
    for rel in (0.25, 0.4):
        cfg = AdaptiveConfig(4, 32, 4, rel, 0.01)
        out.append((f"cornell{rel}", first_result(oracle, "cornell", W, H, cfg)[1], W, H, cfg))
    return out


def _split(Y, w, h, cfg):
    """min = max = min_spp: the first pass alone, and the resume's configuration for the rest."""
    from mafrixraytracing_amd.adaptive import AdaptiveConfig, ResumeConfig, reference_moments, reference_tile_spp
    spp0, _ = reference_tile_spp(Y[:cfg.min_spp], w, h, AdaptiveConfig(cfg.min_spp, cfg.min_spp, cfg.step_spp, cfg.rel_error, cfg.abs_floor))
    assert np.array_equal(spp0, np.full_like(spp0, cfg.min_spp))
    S1, S2 = reference_moments(Y, w, h, spp0)
    return spp0, S1, S2, ResumeConfig(cfg.max_spp, cfg.step_spp, cfg.rel_error, cfg.abs_floor)


def test_one_call_is_first_pass_plus_resume(oracle):
    from mafrixraytracing_amd.adaptive import reference_moments, reference_resume, reference_tile_spp
    for name, Y, w, h, cfg in _cases(oracle):
        want, gap = reference_tile_spp(Y[:cfg.max_spp], w, h, cfg)
        assert len(set(want.ravel().tolist())) > 1, name  # several passes and stops
        spp0, S1, S2, rcfg = _split(Y, w, h, cfg)
        got, active, rgap, R1, R2 = reference_resume(Y, w, h, spp0, S1, S2, rcfg)
        assert np.array_equal(got, want), name
        assert active == 0 and rgap == gap, (name, rgap, gap)  # the same checks, so the same smallest gap
        M1, M2 = reference_moments(Y, w, h, want)
        assert np.array_equal(R1, M1) and np.array_equal(R2, M2), name


def test_one_call_is_the_chain_of_one_pass_resumes(oracle):
    from mafrixraytracing_amd.adaptive import reference_moments, reference_tile_spp
    for name, Y, w, h, cfg in _cases(oracle):
        want, gap = reference_tile_spp(Y[:cfg.max_spp], w, h, cfg)
        spp0, S1, S2, rcfg = _split(Y, w, h, cfg)
        calls, (got, R1, R2), cgap = one_pass_chain(Y, w, h, spp0, S1, S2, rcfg)
        assert np.array_equal(got, want) and cgap == gap, name
        M1, M2 = reference_moments(Y, w, h, want)
        assert np.array_equal(R1, M1) and np.array_equal(R2, M2), name
        # every call but the last ran one pass; the chain's length is the one-call schedule's pass count
        # after the first: counts min, min + step, ... up to the largest count reached
        passes = sum(1 for b, a, _ in calls if not np.array_equal(a, b))
        assert passes == -(-(int(want.max()) - cfg.min_spp) // cfg.step_spp), name
        assert len(calls) in (passes, passes + 1) and calls[-1][2] == 0
        for b, a, active in calls[:-1]:
            assert active > 0 and not np.array_equal(a, b)


def test_idempotence_looser_threshold_and_small_budget(oracle):
    from mafrixraytracing_amd.adaptive import ResumeConfig, reference_resume
    for name, Y, w, h, cfg in _cases(oracle):
        spp0, S1, S2, rcfg = _split(Y, w, h, cfg)
        spp, _, _, S1, S2 = reference_resume(Y, w, h, spp0, S1, S2, rcfg)
        for c in (rcfg,  # the same again
                  ResumeConfig(cfg.max_spp, cfg.step_spp, cfg.rel_error * 2, cfg.abs_floor),  # looser
                  ResumeConfig(cfg.max_spp, cfg.step_spp, cfg.rel_error, cfg.abs_floor + 1.0),
                  ResumeConfig(cfg.min_spp, 1, 0.0, 0.0)):  # the strictest threshold, but no budget
            out, active, _, T1, T2 = reference_resume(Y, w, h, spp, S1, S2, c)
            assert np.array_equal(out, spp) and active == 0, (name, c)
            assert np.array_equal(T1, S1) and np.array_equal(T2, S2), (name, c)
        # a budget below some tiles' counts and above others', threshold 0: the tiles at or above it are
        # left alone, the others go up to the budget at most (exactly, unless E = 0: a black tile)
        mid = int(np.sort(spp.ravel())[spp.size // 2])
        assert mid > int(spp.min()), name
        out, active, _, _, _ = reference_resume(Y, w, h, spp, S1, S2, ResumeConfig(mid, 3, 0.0, 0.0))
        assert active == 0 and np.array_equal(out[spp >= mid], spp[spp >= mid]), name
        assert (out[spp < mid] <= mid).all() and (out[spp < mid] == mid).any(), name


def test_hand_made_cases_on_one_tile():
    """One 5x3 tile (m = 15). Every pixel's samples are +a, -a, +a, ...: after an even n S1 = 0 and
    S2 = n a^2, so E m = 225 a^2 / (n - 1) and the right side is rel^2 (abs_floor 15)^2: with
    abs_floor = 1 the tile converges at the first even n with a^2 / (n - 1) <= rel^2."""
    from mafrixraytracing_amd.adaptive import ResumeConfig, reference_resume
    w, h, a = 5, 3, 2.0
    Y = np.empty((64, w * h))
    Y[0::2] = a
    Y[1::2] = -a
    spp = np.array([[4]], dtype=np.int32)
    S1 = np.zeros(w * h)
    S2 = np.full(w * h, 4 * a * a)

    def resume(spp, S1, S2, **kw):
        d = dict(max_spp=64, step_spp=2, rel_error=0.5, abs_floor=1.0)
        d.update(kw)
        return reference_resume(Y, w, h, spp, S1, S2, ResumeConfig(**d))

    # a^2 / (n - 1) <= 0.25 <=> n >= 17: steps of 2 from 4 stop at 18
    out, active, gap, T1, T2 = resume(spp, S1, S2)
    assert out.tolist() == [[18]] and active == 0
    assert np.array_equal(T1, np.zeros(15)) and np.array_equal(T2, np.full(15, 18 * a * a))
    # the smallest gap is at n = 16 (E m = 60, the right side 56.25) or at 18 (52.94..., 56.25)
    assert gap == pytest.approx(min((60.0 - 56.25) / 60.0, (56.25 - 225 * 4.0 / 17.0) / 56.25), rel=1e-12)
    # steps of 6: 4, 10, 16, 22; a pass limit of 2 stops at 16 with the tile still active
    assert resume(spp, S1, S2, step_spp=6)[0].tolist() == [[22]]
    out, active, _, T1, T2 = resume(spp, S1, S2, step_spp=6, max_passes=2)
    assert out.tolist() == [[16]] and active == 1 and np.array_equal(T2, np.full(15, 16 * a * a))
    out, active, _, _, _ = resume(out, T1, T2, step_spp=6, max_passes=2)  # and goes on from there
    assert out.tolist() == [[22]] and active == 0
    # the budget clips the last pass: 4, 10, 15 (an odd count: S1 = a, still unconverged, stopped by the budget)
    out, active, _, T1, _ = resume(spp, S1, S2, step_spp=6, max_spp=15)
    assert out.tolist() == [[15]] and active == 0 and np.array_equal(T1, np.full(15, a))
    # a looser threshold (a^2 / 3 <= 4), or a budget at the count, runs no pass
    out, active, _, _, T2 = resume(spp, S1, S2, rel_error=2.0)
    assert out.tolist() == [[4]] and active == 0 and np.array_equal(T2, S2)
    assert resume(spp, S1, S2, max_spp=4)[0].tolist() == [[4]] and resume(spp, S1, S2, max_spp=2)[0].tolist() == [[4]]


def test_config_validation():
    from mafrixraytracing_amd.adaptive import ResumeConfig
    for bad in (dict(max_spp=1), dict(step_spp=0), dict(max_passes=-1), dict(rel_error=-0.1), dict(rel_error=float("nan")),
                dict(abs_floor=float("inf"))):
        d = dict(max_spp=8, step_spp=4, rel_error=0.1, abs_floor=0.01)
        d.update(bad)
        with pytest.raises(ValueError):
            ResumeConfig(**d)
