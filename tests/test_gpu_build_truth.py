"""The device BVH build and layout against the independent reference (tests/_bvhref.py)
on the adversarial scenes of tests/_buildcases.py.

tests/test_gpu_build.py holds the device builder to the host builder on benign
scenes.  Here, per case: the device tree equals the numpy reference bit for bit
and passes the structural check; the device's traversal records equal the host
path's; 256 rays traced through a device-built and a host-built context return
identical bits, and where the float64 brute force can judge the scene the
decisive rays meet it.  tests/test_build_truth.py pins the host builder and the
oracle to the same reference on the CPU.
"""
import numpy as np
import pytest

import _buildcases as C
import _bvhref as R
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd.pathtracer import HipContext
from test_build_truth import NONFINITE, check_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_ctx():
    """A second context that builds on the host (KHP_CTX_HOST_BUILD)."""
    ctx = HipContext(0, host_build=True)
    yield ctx
    ctx.close()


def _build(ctx, sd):
    ctx.set_scene(sd)
    ctx.build_accel()
    return ctx.read_bvh(), ctx.read_layout(), ctx.stats()


def _trace(ctx, rays):
    orig, d, tmax = rays
    t, obj, uv = ctx.trace_closest(orig, d)
    return t, obj, uv, ctx.trace_any(orig, d, tmax)


def _unsign_zeros(a):
    a = np.ascontiguousarray(a, np.float32)
    return np.where(a == 0, np.float32(0.0), a).view(np.uint32)


@pytest.mark.parametrize("name", list(C.CASES))
def test_device_build_equals_reference(hip_ctx, host_ctx, name):
    case = C.CASES[name]
    sd, ref, bounds = case.scene(), case.reference(), case.host()["bounds"]
    dev, dlay, st = _build(hip_ctx, sd)
    assert st["bvh_on_device"] == 1 and st["n_nodes"] == len(ref["count"]) and st["bvh_depth"] == ref["depth"]
    got = _trace(hip_ctx, case.rays())
    _, hlay, hst = _build(host_ctx, sd)
    assert hst["bvh_on_device"] == 0
    want = _trace(host_ctx, case.rays())
    if case.signed_zero:
        # a parallel min / max may keep another zero than the sequential one.
        # Equal after clearing the sign of zeros, and every unequal word is a zero on both sides.
        db, rb = dev["boxes"], ref["boxes"]
        assert np.array_equal(_unsign_zeros(db), _unsign_zeros(rb))
        diff = db.view(np.uint32) != rb.view(np.uint32)
        print(f"{name}: {int(diff.sum())} node-box words differ in the sign of a zero")
        assert np.all((db[diff] == 0) & (rb[diff] == 0))
        for k in ("first", "count", "ids"):
            assert np.array_equal(dev[k], ref[k]), k
        assert dev["depth"] == ref["depth"]
        R.check_structure(dev, bounds, zero_sign_free=True)
        dn, hn = dlay["nodes"].view(np.float32), hlay["nodes"].view(np.float32)
        ndiff = dlay["nodes"] != hlay["nodes"]
        assert np.all((dn[ndiff] == 0) & (hn[ndiff] == 0))
    else:
        diff = R.same_tree(ref, dev)
        assert diff is None, f"{name}: reference != device tree: {diff}"
        R.check_structure(dev, bounds)
        assert np.array_equal(dlay["nodes"], hlay["nodes"])
    assert np.array_equal(dlay["aux"], hlay["aux"])
    assert np.array_equal(dlay["prims"].view(np.uint32), hlay["prims"].view(np.uint32))
    # the same rays through both contexts: identical bits, signed-zero cases included
    for what, g, w in zip(("t", "object", "uv", "any-hit"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{name}: {what} differs between the two builds"
    if case.trace_truth:
        check_trace(name, "device build", got[0], got[1], got[3])


def test_depth_64_is_refused_and_the_context_stays_usable(hip_ctx, host_ctx):
    """One level past the traversal stack (STACK_MAX 64 holds depth 63, the depth_63 case):
    KHP_EUNSUPPORTED from khp_build_accel on both paths, and the next scene works."""
    sd = C.DEPTH_64.scene()
    assert C.DEPTH_64.reference()["depth"] == 64
    for ctx in (hip_ctx, host_ctx):
        ctx.set_scene(sd)
        with pytest.raises(N.KhpError) as e:
            ctx.build_accel()
        assert e.value.status == N.KHP_EUNSUPPORTED
        case = C.CASES["count_257"]
        tree, _, st = _build(ctx, case.scene())
        assert R.same_tree(case.reference(), tree) is None and st["bvh_depth"] == case.reference()["depth"]
        t, obj, _, any_hit = _trace(ctx, case.rays())
        check_trace("count_257", "after a refused build", t, obj, any_hit)


@pytest.mark.parametrize("path", ["set_scene", "set_scene_device", "host_build_context"])
@pytest.mark.parametrize("make,arr", [pytest.param(m, a, id=i) for i, m, a in NONFINITE])
def test_nonfinite_geometry_is_refused(hip_ctx, host_ctx, path, make, arr):
    """A NaN or an infinity in tri_v, cone_base_r0 or cone_apex_r1 (first, middle, last
    object): KHP_EINVAL naming the array; khp_build_accel then has no scene."""
    ctx = host_ctx if path == "host_build_context" else hip_ctx
    with pytest.raises(N.KhpError) as e:
        (ctx.set_scene_device if path == "set_scene_device" else ctx.set_scene)(make())
    assert e.value.status == N.KHP_EINVAL and arr in str(e.value)
    with pytest.raises(N.KhpError) as e:
        ctx.build_accel()
    assert e.value.status == N.KHP_ENOTREADY


@pytest.mark.parametrize("path", ["set_scene", "set_scene_device"])
def test_geometry_whose_centroid_overflows_is_refused(hip_ctx, path):
    """The device twin of test_build_truth.test_host_build_refuses_geometry_whose_centroid_overflows."""
    sd = C.tris(C.base(), np.random.default_rng(4).uniform(-1, 1, (20, 3)))
    sd.tri_v[7, :, 0] = 2e38
    with pytest.raises(N.KhpError) as e:
        (hip_ctx.set_scene_device if path == "set_scene_device" else hip_ctx.set_scene)(sd)
    assert e.value.status == N.KHP_EINVAL and "overflow" in str(e.value)
