"""Adaptive-pass measurements (dev tool, GPU box) at the metric row (config 3, 1920 x 1080, 1M
strands, depth 5).  One JSON line per part:
  select  after a uniform 16-spp frame: the selection alone -- k_adapt_flag, k_adapt_scan,
          k_adapt_scatter and the count's copy between two HIP events (khp_debug_adaptive_list's
          select_ms) -- 2 warm-up passes and 9 timed, at the series' threshold and with every pixel
          stopped by max_samples (active == 0: the pass is the selection and nothing else, its wall
          time is given too);
  fold    one khp_render and one adaptive pass from sample 0, 17 spp each (above ACC_MAX_SAMPLES, so
          khp_render folds with k_accumulate_m): under `rocprofv3 --kernel-trace --stats -- python
          tools/adaptive_probe.py fold` the per-kernel times are k_accumulate_m and k_accumulate_a
          over the same pixels and samples;
  series  adaptive passes of 8 spp from sample 0 (threshold THRESHOLD, min_samples 8) until fewer
          than 1% of the pixels are active or MAX_PASSES ran: per pass the active pixels, wall
          milliseconds and Msamples/s; then uniform khp_render passes of 8 spp to the same total wall
          time, and the share of pixels with rel_error <= THRESHOLD for both.
usage: [KHP_LIB=variants/libkirk_x.so] python tools/adaptive_probe.py [select|fold|series|all]"""
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, scenes  # noqa: E402

PART = sys.argv[1] if len(sys.argv) > 1 else "all"
W, H, D, SPP = 1920, 1080, 5, 8
THRESHOLD = 0.0118          # the uniform 16-spp frame's median rel_error
MAX_PASSES = 24
LIB = os.path.basename(os.environ.get("KHP_LIB", "in-tree"))

ctx = HipContext(0)
scenes.config3_device(ctx, W, H, n_strands=1_000_000)
ctx.build_accel()
ctx.set_moments(True)


def share_converged():
    err = ctx.read_moments(W, H, planes=("rel_error",))["rel_error"]
    with np.errstate(invalid="ignore"):
        return float((err <= np.float32(THRESHOLD)).mean())


if PART in ("select", "all"):
    ctx.render(W, H, 16, D, readback=False)
    out = {"part": "select", "lib": LIB, "pixels": W * H, "state_MB": round(W * H * 32 / 1e6, 1)}
    for name, prm in (("threshold", dict(threshold=THRESHOLD, min_samples=8, max_samples=0)),
                      ("none_active", dict(threshold=THRESHOLD, min_samples=0, max_samples=1))):
        ms, wall, active = [], [], None
        for k in range(2 + 9):
            # the state is not advanced between the timed passes of "none_active"; "threshold" traces its
            # active pixels, so its selections see a state that moves on by 1 spp a pass
            t0 = time.perf_counter()
            _f, res = ctx.render_adaptive(W, H, 1, D, first_sample=16 + k, readback=False, **prm)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(ctx.debug_adaptive_list(timing=True)[1])
            active = res["active"] if active is None else active
        out[name] = {"first_active": active, "select_ms_median": round(statistics.median(ms[2:]), 4),
                     "select_ms": [round(x, 4) for x in ms], "call_wall_ms_median": round(statistics.median(wall[2:]), 4)}
    print(json.dumps(out), flush=True)

if PART in ("fold", "all"):
    ctx.render(W, H, 17, D, readback=False)
    t0 = time.perf_counter()
    ctx.render(W, H, 17, D, readback=False)
    t_u = (time.perf_counter() - t0) * 1e3
    ctx.render_adaptive(W, H, 17, D, readback=False, threshold=THRESHOLD)
    t0 = time.perf_counter()
    _f, res = ctx.render_adaptive(W, H, 17, D, readback=False, threshold=THRESHOLD)
    t_a = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"part": "fold", "lib": LIB, "spp": 17, "active": res["active"], "uniform_call_ms": round(t_u, 3),
                      "adaptive_call_ms": round(t_a, 3)}), flush=True)

if PART in ("series", "all"):
    prm = dict(threshold=THRESHOLD, min_samples=8, max_samples=0)
    ctx.render_adaptive(W, H, SPP, D, readback=False, **prm)            # untimed: allocations, clocks
    rows, total = [], 0.0
    for k in range(MAX_PASSES):
        t0 = time.perf_counter()
        _f, res = ctx.render_adaptive(W, H, SPP, D, first_sample=k * SPP, readback=False, **prm)
        ms = (time.perf_counter() - t0) * 1e3
        total += ms
        rows.append({"pass": k, "active": res["active"], "ms": round(ms, 3),
                     "select_ms": round(ctx.debug_adaptive_list(timing=True)[1], 4),
                     "Msamples_per_s": round(res["active"] * SPP / ms / 1e3, 1) if res["active"] else 0.0})
        if res["active"] < 0.01 * W * H:
            break
    st = ctx.read_moments(W, H, planes=("count", "bad"))
    taken = (st["count"].astype(np.uint64) + st["bad"]).reshape(-1)
    adaptive = {"passes": len(rows), "total_ms": round(total, 3), "share_converged": round(share_converged(), 5),
                "samples_traced": int(taken.sum()), "samples_per_pixel_mean": round(float(taken.mean()), 3),
                "samples_per_pixel_max": int(taken.max())}
    ctx.render(W, H, SPP, D, readback=False)                            # untimed
    t_u, n_u = 0.0, 0
    while t_u < total:
        t0 = time.perf_counter()
        ctx.render(W, H, SPP, D, first_sample=n_u * SPP, readback=False)
        t_u += (time.perf_counter() - t0) * 1e3
        n_u += 1
    uniform = {"passes": n_u, "total_ms": round(t_u, 3), "share_converged": round(share_converged(), 5),
               "samples_traced": n_u * SPP * W * H, "ms_per_pass": round(t_u / n_u, 3),
               "Msamples_per_s": round(n_u * SPP * W * H / t_u / 1e3, 1)}
    print(json.dumps({"part": "series", "lib": LIB, "spp": SPP, "threshold": THRESHOLD, "min_samples": 8,
                      "pixels": W * H, "max_passes": MAX_PASSES, "rows": rows, "adaptive": adaptive,
                      "uniform": uniform}), flush=True)
ctx.close()
