"""khp_denoise_var timing (dev tool, GPU box): at the metric row (config 3, 1920 x 1080) with the
moments on render 16 spp, take the planes of khp_render_aov, the moments' mean, m2 and count into
device buffers and time, alternated in one session, khp_denoise (the yardstick: the same frame,
the same run) and khp_denoise_var with the context's moments as the noise and with device planes,
prefilter 1 and 0 -- default parameters (5 iterations), 2 warm-up rounds, 7 timed.  One JSON line.
Under `rocprofv3 --kernel-trace --stats -- python tools/denoise_var_probe.py` the per-kernel times
are k_dn_prepare / k_dn_atrous and k_dnv_prepare / k_dnv_atrous.
usage: [KHP_LIB=variants/libkirk_x.so] python tools/denoise_var_probe.py [timed=7] [iterations=5]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, native, scenes  # noqa: E402
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer  # noqa: E402

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ITER = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, D, SPP = 1920, 1080, 5, 16
ctx = HipContext(0)
scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()
ctx.set_moments(True)
ctx.render(W, H, SPP // 2, D, readback=False)
ctx.render(W, H, SPP // 2, D, first_sample=SPP // 2, readback=False)
aov = ctx.render_aov(W, H, SPP)
planes = {ch: DeviceBuffer.from_array(ctx, aov[ch]) for ch in native.AOV_CHANNELS}
raw = ctx.read_framebuffer(W, H)
m = ctx.read_moments(W, H, device=True, planes=("mean", "m2", "count"))
mean = m["mean"].to_array((H, W, 3), np.float32)
fb = DeviceBuffer.from_array(ctx, raw)
out = DeviceBuffer(ctx, W * H * 12)
outv = DeviceBuffer(ctx, W * H * 4)
calls = {
    "denoise": lambda: ctx.denoise(W, H, planes, m["mean"], out=out, device=True, iterations=ITER),
    "var_context_prefilter1": lambda: ctx.denoise_var(W, H, planes, out=out, device=True, iterations=ITER, prefilter=1),
    "var_context_prefilter0": lambda: ctx.denoise_var(W, H, planes, out=out, device=True, iterations=ITER, prefilter=0),
    "var_planes_prefilter1": lambda: ctx.denoise_var(W, H, planes, m["mean"], moments=m, out=out, device=True,
                                                     iterations=ITER, prefilter=1),
    "var_planes_prefilter0": lambda: ctx.denoise_var(W, H, planes, m["mean"], moments=m, out=out, device=True,
                                                     iterations=ITER, prefilter=0),
    "var_planes_prefilter1_out_variance": lambda: ctx.denoise_var(W, H, planes, m["mean"], moments=m, out=out,
                                                                  out_variance=outv, device=True, iterations=ITER),
}
ms = {k: [] for k in calls}
for _round in range(2 + TIMED):                                 # alternated: every call once per round
    for k, f in calls.items():
        t0 = time.perf_counter()
        f()
        ms[k].append((time.perf_counter() - t0) * 1e3)
med = {k: statistics.median(v[2:]) for k, v in ms.items()}
finite = lambda f: int((~np.isfinite(f).all(-1)).sum())
calls["denoise"]()
fixed = out.to_array((H, W, 3), np.float32)
ctx.denoise(W, H, planes, fb, out=out, device=True, iterations=ITER)
fixed_fb = out.to_array((H, W, 3), np.float32)
calls["var_context_prefilter1"]()
guided = out.to_array((H, W, 3), np.float32)
print(json.dumps({"lib": os.path.basename(os.environ.get("KHP_LIB", "in-tree")), "iterations": ITER, "spp": SPP,
                  "median_ms": {k: round(v, 3) for k, v in med.items()},
                  "ratio_to_denoise": {k: round(v / med["denoise"], 3) for k, v in med.items()},
                  "min_ms": {k: round(min(v[2:]), 3) for k, v in ms.items()},
                  "max_ms": {k: round(max(v[2:]), 3) for k, v in ms.items()},
                  "scratch_MB": {"denoise": round(W * H * 80 / 1e6, 1), "denoise_var": round(W * H * 80 / 1e6, 1)},
                  "nonfinite_pixels": {"framebuffer": finite(raw), "mean": finite(mean), "denoise_of_framebuffer": finite(fixed_fb),
                                       "denoise_of_mean": finite(fixed), "denoise_var": finite(guided)}}), flush=True)
ctx.close()
