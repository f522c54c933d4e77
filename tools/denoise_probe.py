"""khp_denoise timing (dev tool, GPU box): at the metric row (config 3, 1920 x 1080) render one
8-spp pass, take the six planes of khp_render_aov into device buffers and time denoise on device
buffers -- default parameters (5 iterations), 2 warm-up calls, 7 timed -- next to one
khp_render_aov call and the pass itself.  One JSON line.  Under `rocprofv3 --kernel-trace
--stats -- python tools/denoise_probe.py` the per-kernel times are k_dn_prepare and k_dn_atrous.
usage: [KHP_LIB=variants/libkirk_x.so] python tools/denoise_probe.py [timed=7] [iterations=5] [demodulate=0]"""
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
DEMOD = bool(int(sys.argv[3])) if len(sys.argv) > 3 else False
W, H, D, SPP = 1920, 1080, 5, 8
ctx = HipContext(0)
scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()
ctx.render(W, H, SPP, D, readback=False)                       # warm-up pass
t0 = time.perf_counter()
ctx.render(W, H, SPP, D, first_sample=SPP, readback=False)
pass_ms = (time.perf_counter() - t0) * 1e3
ctx.render_aov(W, H, SPP)                                       # warm-up (scratch)
t0 = time.perf_counter()
aov = ctx.render_aov(W, H, SPP)
aov_ms = (time.perf_counter() - t0) * 1e3
planes = {ch: DeviceBuffer.from_array(ctx, aov[ch]) for ch in native.AOV_CHANNELS}
raw = ctx.read_framebuffer(W, H)
colour = DeviceBuffer.from_array(ctx, raw)
out = DeviceBuffer(ctx, W * H * 12)
ms = []
for k in range(2 + TIMED):
    t0 = time.perf_counter()
    ctx.denoise(W, H, planes, colour, out=out, device=True, iterations=ITER, demodulate=DEMOD)
    ms.append((time.perf_counter() - t0) * 1e3)
frame = out.to_array((H, W, 3), np.float32)
med = statistics.median(ms[2:])
# unique bytes of one iteration: three 16-B records and the centre's read, one written (64 + 16 B per pixel)
print(json.dumps({"lib": os.path.basename(os.environ.get("KHP_LIB", "in-tree")), "iterations": ITER,
                  "demodulate": DEMOD, "denoise_median_ms": round(med, 3), "denoise_ms": [round(x, 3) for x in ms],
                  "render_aov_ms": round(aov_ms, 3), "pass_8spp_ms": round(pass_ms, 3),
                  "unique_MB_per_iteration": round(W * H * 80 / 1e6, 1),
                  "nonfinite_pixels_raw": int((~np.isfinite(raw).all(-1)).sum()),
                  "nonfinite_pixels_denoised": int((~np.isfinite(frame).all(-1)).sum())}), flush=True)
ctx.close()
