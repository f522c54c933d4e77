"""Sample-moments measurements (dev tool, GPU box) at the metric row (config 3, 1920 x 1080,
1M strands, depth 5).  One JSON line per part:
  cost      the bench's timed loop -- 5 warm-up and 20 timed asynchronous 8-spp passes, fused by the
            library -- with khp_set_moments off and on, alternated, REPS times each;
  read      khp_read_moments of all five planes into device buffers and into host arrays, 2 warm-up
            calls and 7 timed each, medians;
  rejected  after a 16-spp frame from sample 0: pixels with bad > 0, non-finite pixels of mean and
            of the framebuffer.
Under `rocprofv3 --kernel-trace --stats -- python tools/moments_probe.py cost` the per-kernel times
are k_accumulate_all and k_accumulate_all_m.
usage: [KHP_LIB=variants/libkirk_x.so] python tools/moments_probe.py [cost|read|rejected|all] [reps=3]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, native, scenes  # noqa: E402

PART = sys.argv[1] if len(sys.argv) > 1 else "all"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W, H, D, SPP = 1920, 1080, 5, 8
WARMUP, STEPS = 5, 20
LIB = os.path.basename(os.environ.get("KHP_LIB", "in-tree"))

ctx = HipContext(0)
scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()


def timed_passes():
    """ms per pass of STEPS asynchronous SPP-sample passes after WARMUP of them (the bench's loop)."""
    for k in range(WARMUP):
        ctx.render(W, H, SPP, D, first_sample=k * SPP, async_=True)
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(WARMUP, WARMUP + STEPS):
        ctx.render(W, H, SPP, D, first_sample=k * SPP, async_=True)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / STEPS


if PART in ("cost", "all"):
    timed_passes()                                              # untimed: allocations, clocks
    ms = {False: [], True: []}
    for _ in range(REPS):
        for on in (False, True):
            ctx.set_moments(on)
            ms[on].append(round(timed_passes(), 4))
    ctx.set_moments(False)
    off, on = ms[False], ms[True]
    print(json.dumps({"part": "cost", "lib": LIB, "passes": STEPS, "spp": SPP, "ms_per_pass_off": off, "ms_per_pass_on": on,
                      "median_off": statistics.median(off), "median_on": statistics.median(on),
                      "spread_off": round(max(off) - min(off), 4),
                      "on_minus_off": round(statistics.median(on) - statistics.median(off), 4)}), flush=True)

if PART in ("read", "rejected", "all"):
    from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer  # noqa: E402
    ctx.set_moments(True)
    ctx.render(W, H, 16, D, readback=False)                     # §13's 16-spp frame
    if PART in ("read", "all"):
        bufs = {ch: DeviceBuffer(ctx, int(np.prod((H, W) + tail)) * 4) for ch, (tail, _) in native.MOMENTS_PLANES.items()}
        host = {ch: np.zeros((H, W) + tail, dt) for ch, (tail, dt) in native.MOMENTS_PLANES.items()}
        t = {"device": [], "host": []}
        for k in range(2 + 7):
            t0 = time.perf_counter()
            ctx.read_moments(W, H, device=True, out=bufs)
            t["device"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ctx.read_moments(W, H, out=host)
            t["host"].append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"part": "read", "lib": LIB, "planes": list(native.MOMENTS_PLANES),
                          "device_median_ms": round(statistics.median(t["device"][2:]), 3),
                          "host_median_ms": round(statistics.median(t["host"][2:]), 3),
                          "device_ms": [round(x, 3) for x in t["device"]], "host_ms": [round(x, 3) for x in t["host"]],
                          "MB_read": round(W * H * 32 / 1e6, 1), "MB_written": round(W * H * 36 / 1e6, 1)}), flush=True)
    if PART in ("rejected", "all"):
        m = ctx.read_moments(W, H)
        fb = ctx.read_framebuffer(W, H)
        lost = ~np.isfinite(fb).all(-1)
        print(json.dumps({"part": "rejected", "lib": LIB, "spp": 16, "pixels": W * H,
                          "pixels_with_bad": int((m["bad"] > 0).sum()), "rejected_samples": int(m["bad"].sum()),
                          "nonfinite_pixels_mean": int((~np.isfinite(m["mean"]).all(-1)).sum()),
                          "nonfinite_pixels_m2": int((~np.isfinite(m["m2"]).all(-1)).sum()),
                          "nonfinite_pixels_framebuffer": int(lost.sum()),
                          "framebuffer_lost_exactly_where_bad": bool(np.array_equal(lost, m["bad"] > 0)),
                          "mean_is_framebuffer_elsewhere": bool(np.array_equal(m["mean"][~lost].view(np.uint32),
                                                                               fb[~lost].view(np.uint32))),
                          "median_rel_error": float(np.median(m["rel_error"][np.isfinite(m["rel_error"])]))}), flush=True)
ctx.close()
