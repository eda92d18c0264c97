"""bench.py's plain run: the line's headline fields, nothing measured beside them without --full, and
--dump-outputs writing the last timed step's accumulator (the same file run after run, and the
accumulator a context here traces for that step's samples)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, SEED

pytestmark = pytest.mark.gpu

STEPS, WARMUP, SPP = 2, 1, 2
EXTRAS = ("roofline", "render_api", "sample_api", "strong_share", "cpu_baseline")


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines  # the JSON line alone on stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    common = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--spp", str(SPP)]
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench(common + ["--dump-outputs", d1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and line["rays_per_step"] > 0
    # value = rays per second over the timed steps (both rounded on the line: 3 and 2 decimals)
    assert line["value"] == pytest.approx(line["rays_per_step"] / line["ms_per_step"] / 1e3, rel=2e-2)
    for k in EXTRAS:  # measured with --full only
        assert line[k] is None, k
    assert os.listdir(d1) == ["accum.npy"]
    acc = np.load(os.path.join(d1, "accum.npy"))
    w, h = line["config"]["width"], line["config"]["height"]
    assert acc.dtype == np.float64 and acc.shape == (3, w * h) and acc.nbytes <= 64e6
    # the same arguments, the same outputs
    _bench(common + ["--dump-outputs", d2])
    assert np.array_equal(acc, np.load(os.path.join(d2, "accum.npy")))
    # it is the last timed step's frame: that step's samples traced by a context of this process
    from mafrixraytracing_amd.native import NativeContext
    from mafrixraytracing_amd.scene_io import load_scene_file
    with NativeContext(load_scene_file(os.path.join(SCENES, "spot.xml")), seed=SEED) as ctx:
        ctx.accum_clear()
        ctx.trace_accumulate(SPP, (WARMUP + STEPS - 1) * SPP)
        m = ctx.accum_read_mean(1.0)
    assert acc.any() and np.array_equal(acc, m[:, :3].T)
