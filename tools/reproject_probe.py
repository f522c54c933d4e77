"""khp_reproject timing (dev tool, GPU box): at the metric row (config 3, 1920 x 1080) with the moments
on render 16 spp at the scene's camera, turn the camera by about one pixel, render one more pass there,
take both cameras' khp_render_aov planes, the moments' mean and the variance of that mean into device
buffers and time, alternated in one session, khp_denoise (the yardstick: the same frame, the same run)
and khp_reproject with its defaults, with every test off, with every test on, and with the colour as
its only output -- 2 warm-up rounds, 7 timed, a host clock around calls that return when the outputs
are written.  One JSON line.  Under `rocprofv3 --kernel-trace --stats -- python tools/reproject_probe.py`
the kernel is k_reproject, the yardstick's k_dn_prepare / k_dn_atrous.
usage: python tools/reproject_probe.py [timed=7]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, native, scenes  # noqa: E402
from ba_pathtracing_fur_amd.pathtracer import REPROJECT_OUTPUTS, DeviceBuffer  # noqa: E402

TIMED = int(sys.argv[1]) if len(sys.argv) > 1 else 7
W, H, D, SPP = 1920, 1080, 5, 16
F32 = np.float32
ctx = HipContext(0)
sd = scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()
ctx.set_moments(True)
ctx.render(W, H, SPP // 2, D, readback=False)
ctx.render(W, H, SPP // 2, D, first_sample=SPP // 2, readback=False)
camA = sd.cam
v = lambda a: np.array(list(a), np.float64)
look = -np.cross(v(camA.axis_x), v(camA.axis_y))
ps = float(camA.pixel_size)
camB = scenes.camera(v(camA.position), look + 1.0 * ps * v(camA.axis_x) + 0.4 * ps * v(camA.axis_y), (0.0, 1.0, 0.0), W, H)
up = lambda a: DeviceBuffer.from_array(ctx, a)
aovA = {ch: up(a) for ch, a in ctx.render_aov(W, H, SPP).items()}
m = ctx.read_moments(W, H, planes=("mean", "m2", "count"))
nf = m["count"].astype(F32)
with np.errstate(all="ignore"):
    var = np.where(m["count"] >= 2, ((m["m2"][..., 0] + m["m2"][..., 1]) + m["m2"][..., 2]) / (nf * (nf - F32(1.0))),
                   F32(np.nan)).astype(F32)
hist = {"camera": camA, "colour": up(m["mean"]), "variance": up(var), "length": up(np.full((H, W), SPP, F32)), "aov": aovA}
ctx.set_camera(camB)
one = ctx.render(W, H, 1, D)
host_aovB = ctx.render_aov(W, H, 1)
cur = {"camera": camB, "colour": up(one), "aov": {ch: up(a) for ch, a in host_aovB.items()}}
out = {k: DeviceBuffer(ctx, W * H * 4 * int(np.prod(tail + (1,)))) for k, tail in REPROJECT_OUTPUTS.items()}
dn_out = DeviceBuffer(ctx, W * H * 12)
off = dict(depth_tol=0.0, normal_tol=0.0, tangent_tol=0.0, coverage_tol=0.0)
calls = {
    "denoise": lambda: ctx.denoise(W, H, aovA, hist["colour"], out=dn_out, device=True),
    "reproject_defaults": lambda: ctx.reproject(W, H, cur, hist, out=out, device=True),
    "reproject_tests_off": lambda: ctx.reproject(W, H, cur, hist, out=out, device=True, **off),
    "reproject_every_test": lambda: ctx.reproject(W, H, cur, hist, out=out, device=True, normal_tol=0.25, match_object=True),
    "reproject_colour_only": lambda: ctx.reproject(W, H, cur, hist, out={"colour": out["colour"], "length": None,
                                                                         "variance": None, "motion": None}, device=True),
    "reproject_no_history": lambda: ctx.reproject(W, H, cur, None, out=out, device=True),
}
ms = {k: [] for k in calls}
for _round in range(2 + TIMED):                                 # alternated: every call once per round
    for k, f in calls.items():
        t0 = time.perf_counter()
        f()
        ms[k].append((time.perf_counter() - t0) * 1e3)
med = {k: statistics.median(t[2:]) for k, t in ms.items()}
calls["reproject_defaults"]()
length = out["length"].to_array((H, W), F32)
motion = out["motion"].to_array((H, W, 2), F32)
surf = host_aovB["coverage"] > 0
# the planes the default call touches, bytes per pixel: the current frame read once, the history's unique
# footprint (each history pixel is a tap of about four current pixels), the outputs written
bytes_pp = {"current": 12 + 4 + 4 + 12, "history": 12 + 4 + 4 + 4 + 4 + 12, "outputs": 12 + 4 + 4 + 8}
print(json.dumps({"timed": TIMED, "spp_history": SPP,
                  "median_ms": {k: round(t, 3) for k, t in med.items()},
                  "ratio_to_denoise": {k: round(t / med["denoise"], 3) for k, t in med.items()},
                  "min_ms": {k: round(min(t[2:]), 3) for k, t in ms.items()},
                  "max_ms": {k: round(max(t[2:]), 3) for k, t in ms.items()},
                  "bytes_per_pixel_defaults": bytes_pp, "MB_defaults": round(sum(bytes_pp.values()) * W * H / 1e6, 1),
                  "surface_pixels": int(surf.sum()), "with_history": int((length[surf] > 1).sum()),
                  "median_motion_pixels": round(float(np.nanmedian(np.hypot(motion[..., 0], motion[..., 1]))), 3)}), flush=True)
ctx.close()
