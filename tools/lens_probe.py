"""What the thin-lens camera costs (dev tool, GPU box): at the metric row (config 3, 1920 x 1080, 8 spp,
depth 5, the 1M-strand hairball) render with the lens off and with KIRK's lens (khp_lens_from_kirk(0.0415,
1.8, .): radius 0.0692) focused on the hairball's centre, at half and at twice that distance, alternated in
one session: 2 warm-up rounds, then TIMED rounds of one synchronous khp_render each, a host clock around a
call that returns when the frame is complete.  Then one instrumented pass per setting (khp_render with
statistics, the wavefront with counting kernels: its times are not the metric's) for the per-bounce extend
time, node visits and lane use.  One JSON line.
usage: python tools/lens_probe.py [timed=5]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, lens_from_kirk, scenes  # noqa: E402

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H, D, SPP = 1920, 1080, 5, 8
ctx = HipContext(0)
sd = scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()
dist = float(np.linalg.norm(np.array(list(sd.cam.position), np.float64) - np.array([0.0, 1.0, 0.0])))
settings = {"off": dict(radius=0.0)}
for name, f in (("focus_centre", 1.0), ("focus_half", 0.5), ("focus_twice", 2.0)):
    settings[name] = lens_from_kirk(0.0415, 1.8, dist * f)
ms = {k: [] for k in settings}
for _round in range(2 + TIMED):                                  # alternated: every setting once per round
    for k, lens in settings.items():
        ctx.set_lens(**lens)
        t0 = time.perf_counter()
        ctx.render(W, H, SPP, D, readback=False)
        ms[k].append((time.perf_counter() - t0) * 1e3)
inst = {}
for k, lens in settings.items():
    ctx.set_lens(**lens)
    ctx.render(W, H, SPP, D, readback=False, stats=True)
    st = ctx.stats()
    busy = [b / (64.0 * i) if i else 0.0 for b, i in zip(st["bounce_lanes_busy"][:D], st["bounce_wave_iters"][:D])]
    inst[k] = {"bounce_extend_ms": [round(v, 3) for v in st["bounce_extend_ms"][:D]],
               "bounce_nodes_per_ray": [round(n / r, 2) if r else 0.0
                                        for n, r in zip(st["bounce_nodes"][:D], st["bounce_rays"][:D])],
               "bounce_lane_use": [round(v, 3) for v in busy], "extend_ms": round(st["extend_ms"], 3)}
med = {k: statistics.median(t[2:]) for k, t in ms.items()}
print(json.dumps({"timed": TIMED, "camera_to_centre": round(dist, 4),
                  "lens": {k: {a: round(b, 5) for a, b in v.items()} for k, v in settings.items()},
                  "median_ms": {k: round(t, 3) for k, t in med.items()},
                  "min_ms": {k: round(min(t[2:]), 3) for k, t in ms.items()},
                  "max_ms": {k: round(max(t[2:]), 3) for k, t in ms.items()},
                  "Msamples_per_s": {k: round(W * H * SPP / t / 1e3, 2) for k, t in med.items()},
                  "instrumented": inst}))
ctx.close()
