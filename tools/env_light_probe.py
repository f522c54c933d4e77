"""What the environment light costs (dev tool, GPU box).

1. The table build: khp_set_env_light of a 2048 x 1024 map already in device memory, a host clock around
   the call (copy, check, build, two waits), 2 warm-up and TIMED timed calls.
2. The metric row (config 3, 1920 x 1080, 8 spp, depth 5, the 1M-strand hairball) with the light off, and
   with a 512 x 256 sky_map in place of env.color with nee 1 and nee 0, alternated in one session: 2 warm-up
   rounds, then TIMED rounds of one synchronous khp_render each, a host clock around a call that returns
   when the frame is complete.  Then one instrumented pass per setting (khp_render with statistics, the
   wavefront with counting kernels: its times are not the metric's) for the shade and shadow stages.
One JSON line.
usage: python tools/env_light_probe.py [timed=5]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, scenes  # noqa: E402
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer  # noqa: E402

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H, D, SPP = 1920, 1080, 5, 8
ctx = HipContext(0)
big = scenes.sky_map(2048, 1024)
buf = DeviceBuffer.from_array(ctx, big)
build_ms = []
for _ in range(2 + TIMED):
    t0 = time.perf_counter()
    ctx.set_env_light(buf, device_shape=big.shape[:2])
    build_ms.append((time.perf_counter() - t0) * 1e3)
ctx.clear_env_light()
buf.free()

sd = scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()
sky = scenes.sky_map(512, 256)
settings = {"off": None, "nee1": True, "nee0": False}


def apply(nee):
    if nee is None:
        ctx.clear_env_light()
    else:
        ctx.set_env_light(sky, nee=nee)


ms = {k: [] for k in settings}
for _round in range(2 + TIMED):                                  # alternated: every setting once per round
    for k, nee in settings.items():
        apply(nee)
        t0 = time.perf_counter()
        ctx.render(W, H, SPP, D, readback=False)
        ms[k].append((time.perf_counter() - t0) * 1e3)
inst = {}
for k, nee in settings.items():
    apply(nee)
    ctx.render(W, H, SPP, D, readback=False, stats=True)
    st = ctx.stats()
    inst[k] = {key: (round(v, 3) if isinstance(v, float) else v) for key, v in st.items()
               if key in ("extend_ms", "shade_ms", "shadow_ms", "shadow_finish_ms", "extend_rays", "shadow_rays")}
med = {k: statistics.median(t[2:]) for k, t in ms.items()}
print(json.dumps({"timed": TIMED,
                  "table_build_2048x1024_ms": {"median": round(statistics.median(build_ms[2:]), 3),
                                               "min": round(min(build_ms[2:]), 3), "max": round(max(build_ms[2:]), 3)},
                  "median_ms": {k: round(t, 3) for k, t in med.items()},
                  "min_ms": {k: round(min(t[2:]), 3) for k, t in ms.items()},
                  "max_ms": {k: round(max(t[2:]), 3) for k, t in ms.items()},
                  "Msamples_per_s": {k: round(W * H * SPP / t / 1e3, 2) for k, t in med.items()},
                  "instrumented": inst}))
ctx.close()
