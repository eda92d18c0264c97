#!/usr/bin/env python3
"""k_camera's phase split from a stamp build (-DMFX_DIAG -DMFX_DIAG_STAMPS=3): the shares of its waves'
cycles in the window scan, the camera ray, node steps (cut entries included), leaf tests and result writes,
and the node steps per window, from counters 10..15 of one trace.
Usage: camera_phases.py LIB.so [SCENE] [SPP]    (MFX_CAMERA_CUTS=0 in the environment: from the root)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mafrixraytracing_amd.abi as abi  # noqa: E402

lib = sys.argv[1]
abi._lib = abi.load_library(lib, strict=False)
from mafrixraytracing_amd.native import DEFAULT_SEED, NativeContext  # noqa: E402
from mafrixraytracing_amd.scene_io import load_scene_file  # noqa: E402

scene = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "scenes", "spot.xml")
spp = int(sys.argv[3]) if len(sys.argv) > 3 else 64
a = load_scene_file(scene)
ctx = NativeContext(a, seed=DEFAULT_SEED)
for k in range(2):  # the second trace: the cut table is the camera's already
    ctx.accum_clear()
    ctx.trace_accumulate(spp, k * spp)
    ctx.sync()
c = ctx.ray_counts()
ph = dict(zip(["window_scan", "camera_ray", "node_steps", "leaf_tests", "result_writes"], c[10:15]))
tot = sum(ph.values())
windows = ((a.width + 7) // 8) * ((a.height + 7) // 8) * spp
tt = ctx.trace_timing()
print(os.path.basename(lib), os.path.basename(scene), "spp", spp,
      json.dumps({k: round(v / tot, 4) for k, v in ph.items()}), "wave-cycles %.4g" % tot,
      "node steps / window %.3f" % (c[15] / windows),
      "k_camera %.3f ms" % tt["camera_ms"], json.dumps(getattr(ctx, "launch_info", dict)()))
