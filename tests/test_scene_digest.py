"""The bytes of the host-built scene image (mfx_scene.cpp, no GPU): the host tool
mafrixraytracing_amd/csrc/build/scene_digest (scene_digest.cpp, built by `make`) prints one line per
scene (FNV digests of the device images, the reference leaf grouping and the light, the shape
counters, eps and tslack) and one per bad description (its error text), then half_dir's self-check
against a table of all finite halves, the FP16 node image of every scene and soup_600 scaled and moved
past and below the binary16 range (shares of +-inf and subnormal planes, planes not rounded outward);
every line must equal the recorded one. tests/test_gpu_build.py pins the GPU-built image to the host-built one; this pins the
host-built one itself."""
import json
import os
import subprocess

from conftest import ROOT

TOOL = os.path.join(ROOT, "mafrixraytracing_amd", "csrc", "build", "scene_digest")
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_digests.json")


def test_host_scene_digests_match_golden():
    assert os.path.isfile(TOOL), f"{TOOL} is missing: run build() (make -C mafrixraytracing_amd/csrc)"
    with open(GOLDEN) as f:
        want = json.load(f)["lines"]
    r = subprocess.run([TOOL], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), (got[len(want):], want[len(got):])
