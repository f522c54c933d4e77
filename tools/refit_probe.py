"""What a refit costs and what it buys (dev tool, GPU box).

The metric scene (config 3: the 1M-strand hairball, 9M cones, 1920 x 1080), bent by scenes.bend at 0.01,
0.05 and 0.3 of its radius, every array in device memory before a clock starts.  Per amplitude, ROUNDS
alternated rounds in one process, a host clock around calls that return when the work is complete:
1. khp_get_refit_info (makes the refit plan, once per khp_build_accel; timed on its own), then
   khp_update_geometry_device from the original to the moved arrays, then one 8-spp depth-5 pass on the
   refitted tree (one untimed pass first: the first pass after a change pays for dropped render-ahead work);
2. khp_set_scene_device + khp_build_accel of the same moved arrays, then the same pass on the rebuilt tree;
3. the original scene built again (untimed) for the next round.
Also sah_cost / sah_cost_built of the refitted tree.  One JSON line: minimum, median, maximum of each.
usage: python tools/refit_probe.py [rounds=3] [n_strands=1000000]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from ba_pathtracing_fur_amd import HipContext, scenes  # noqa: E402
from ba_pathtracing_fur_amd import native as N  # noqa: E402
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
STRANDS = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
W, H, D, SPP = 1920, 1080, 5, 8
FRACS = (0.01, 0.05, 0.3)

ctx = HipContext(0)
lib = ctx.lib
sd = scenes.config3(W, H, n_strands=STRANDS)
_, radius = scenes.bend_frame(sd)


def device_desc(s):
    """khp_scene of `s` with the per-object arrays in device memory; (desc, buffers to keep)."""
    d = s.desc()
    keep = []

    def dev(a, ty):
        b = DeviceBuffer.from_array(ctx, a)
        keep.append(b)
        return ctypes.cast(b.ptr, ctypes.POINTER(ty))

    d.tri_v, d.tri_n = dev(s.tri_v, ctypes.c_float), dev(s.tri_n, ctypes.c_float)
    d.tri_frame, d.tri_mat = dev(s.frames(), ctypes.c_float), dev(s.tri_mat, ctypes.c_uint32)
    d.cone_base_r0, d.cone_apex_r1 = dev(s.cone_base_r0, ctypes.c_float), dev(s.cone_apex_r1, ctypes.c_float)
    d.cone_mat = dev(s.cone_mat, ctypes.c_uint32)
    return d, keep


def build(d):
    N.check(lib, lib.khp_set_scene_device(ctx.ptr, ctypes.byref(d)), "khp_set_scene_device")
    N.check(lib, lib.khp_build_accel(ctx.ptr), "khp_build_accel")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def pass_ms():
    ctx.render(W, H, SPP, D, readback=False)
    return timed(lambda: ctx.render(W, H, SPP, D, readback=False))


def mmm(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


d0, keep0 = device_desc(sd)
out = {"rounds": ROUNDS, "n_strands": STRANDS, "n_objects": sd.n_objects, "amplitudes": {}}
for frac in FRACS:
    mv = scenes.bend(sd, np.float32(frac) * radius)
    d1, keep1 = device_desc(mv)
    info = N.RefitInfo()
    plan, refit, rebuild, kern, p_refit, p_rebuilt, ratio = [], [], [], [], [], [], []
    for _ in range(ROUNDS):
        build(d0)
        plan.append(timed(ctx.refit_info))   # the refit plan, made once per khp_build_accel
        refit.append(timed(lambda: N.check(lib, lib.khp_update_geometry_device(ctx.ptr, ctypes.byref(d1),
                                                                               ctypes.byref(info)),
                                           "khp_update_geometry_device")))
        kern.append(info.kernel_ms)
        ratio.append(info.sah_cost / info.sah_cost_built)
        p_refit.append(pass_ms())
        rebuild.append(timed(lambda: build(d1)))
        p_rebuilt.append(pass_ms())
    out["amplitudes"][str(frac)] = {"refit_plan_ms": mmm(plan), "update_geometry_device_ms": mmm(refit), "its_kernels_ms": mmm(kern),
                                    "set_scene_device_plus_build_accel_ms": mmm(rebuild),
                                    "sah_cost_over_built": round(ratio[-1], 4),
                                    "pass_on_refitted_tree_ms": mmm(p_refit), "pass_on_rebuilt_tree_ms": mmm(p_rebuilt)}
    for b in keep1:
        b.free()
print(json.dumps(out))
ctx.close()
