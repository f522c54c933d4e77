"""What BSDF kind 11 costs (dev tool, GPU box): at the metric row (config 3, 1920 x 1080, 8 spp, depth 5, the
1M-strand hairball) render the fur with KIRK's Marschner material and with a ChiangHairBSDF material of the same
colour, alternated in one session: 2 warm-up rounds, then TIMED rounds of one synchronous khp_render each, a host
clock around a call that returns when the frame is complete.  Two contexts hold the two scenes, so nothing is
rebuilt between the calls.  Then the furnace figure DESIGN.md §22 records: the mean of a 200-strand white
hairball in a white environment at depth 8 and at depth 64.  One JSON line.
usage: python tools/hair_probe.py [timed=5] [strands=1000000]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, scenes  # noqa: E402

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STRANDS = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
W, H, D, SPP = 1920, 1080, 5, 8


def metric_ctx(chiang):
    sd = scenes.config3(W, H, n_strands=STRANDS)
    if chiang:
        for i, m in enumerate(sd.materials):
            if m.bsdf == 9:
                sd.materials[i] = scenes.hair_material(tuple(m.diffuse), ior=m.ior)
    ctx = HipContext(0)
    ctx.set_scene(sd)
    ctx.build_accel()
    return ctx


ctxs = {"marschner": metric_ctx(False), "chiang": metric_ctx(True)}
ms = {k: [] for k in ctxs}
for _round in range(2 + TIMED):                                  # alternated: each material once per round
    for k, ctx in ctxs.items():
        t0 = time.perf_counter()
        ctx.render(W, H, SPP, D, readback=False)
        ms[k].append((time.perf_counter() - t0) * 1e3)
finite = {k: bool(np.isfinite(c.read_framebuffer(W, H)).all()) for k, c in ctxs.items()}
for c in ctxs.values():
    c.close()

fw, fh = 64, 48
sd = scenes.SceneData(name="white_hairball")
pos, rad = scenes.hairball(200, (0.0, 0.5, 0.0), 0.25)
sd.add_fibers(pos, rad, sd.add_material(scenes.hair_material((1.0, 1.0, 1.0))))
sd.cam = scenes.config2(fw, fh, n_strands=1).cam
sd.lights, sd.env_color, sd.env_ambient = [], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
ctx = HipContext(0)
ctx.set_scene(sd)
ctx.build_accel()
furnace = {}
for depth in (8, 64):
    img = ctx.render(fw, fh, 256, depth)
    furnace[f"depth_{depth}"] = {"mean": round(float(img.astype(np.float64).mean()), 6), "max": round(float(img.max()), 6)}
ctx.close()

med = {k: statistics.median(t[2:]) for k, t in ms.items()}
print(json.dumps({"timed": TIMED, "strands": STRANDS, "median_ms": {k: round(t, 3) for k, t in med.items()},
                  "min_ms": {k: round(min(t[2:]), 3) for k, t in ms.items()},
                  "max_ms": {k: round(max(t[2:]), 3) for k, t in ms.items()},
                  "ms_per_pass": {k: round(t / SPP, 3) for k, t in med.items()},
                  "Msamples_per_s": {k: round(W * H * SPP / t / 1e3, 2) for k, t in med.items()},
                  "frame_finite": finite, "white_hairball_furnace": furnace}))
