"""khp_reproject without a device: the exports and the structs, the refusals (each before
the context is touched, every pointer a poison that would fault if read), khp_reproject_host against
the numpy restatement (tests/_reprojectref.py) bit for bit, the motion vectors against a float64
evaluation written here, known answers, the TemporalAccumulator, and the quality of a pushed frame on
oracle frames (GPU frames are bit-identical to the oracle's)."""
import ctypes
import dataclasses
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ba_pathtracing_fur_amd as P
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes
from ba_pathtracing_fur_amd.pathtracer import HipContext

import _aovref as A
import _reprojectref as R
import oracle_ffi

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("colour", "length", "variance", "motion")
TOLS = ("depth_tol", "normal_tol", "tangent_tol", "coverage_tol")
ALL_OFF = {t: 0.0 for t in TOLS}


def same(a, b):
    return a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


# ---- export and layout -------------------------------------------------------------------------------------
def test_symbols_are_exported_listed_and_declared():
    lib = N.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    for sym in ("khp_reproject", "khp_reproject_host", "khp_reproject_params_defaults"):
        assert sym in N.EXPORTED and hasattr(lib, sym)
        assert re.search(r"\bT %s\b" % sym, out), sym
    header = open(os.path.join(ROOT, "include", "kirk_hip.h")).read()
    flat = " ".join(header.split())
    assert ("khp_status khp_reproject(khp_ctx* ctx, const khp_reproject_params* p, const khp_reproject_frame* cur, "
            "const khp_reproject_frame* hist /* nullable */, const khp_reproject_out* out);") in flat
    assert ("khp_status khp_reproject_host(const khp_reproject_params* p, const khp_reproject_frame* cur, "
            "const khp_reproject_frame* hist /* nullable */, const khp_reproject_out* out);") in flat
    assert "void khp_reproject_params_defaults(khp_reproject_params* out);" in flat
    assert "#define KHP_REPROJECT_DEVICE (1u << 0)" in flat and "#define KHP_REPROJECT_MATCH_OBJECT (1u << 1)" in flat
    assert "starting values, not a measured optimum" in flat
    for name in ("khp_reproject_params", "khp_reproject_frame", "khp_reproject_out"):
        assert "} %s;" % name in flat
    # symbols added, nothing moved: the ABI number stays
    assert "#define KHP_ABI_VERSION 17" in header and N.ABI_VERSION == 17 and lib.khp_abi_version() == 17
    hpp = open(os.path.join(ROOT, "include", "kirk_hip.hpp")).read()
    assert "khp_reproject(c_, &p, &cur, hist, &out)" in hpp and "khp_reproject_params_defaults" in hpp
    assert callable(HipContext.reproject) and callable(P.reproject_host) and callable(P.TemporalAccumulator)
    for name in ("ReprojectParams", "ReprojectFrame", "ReprojectOut", "REPROJECT_DEVICE", "REPROJECT_MATCH_OBJECT"):
        assert name in P.__all__ and getattr(P, name) is getattr(N, name)
    assert "reproject_host" in P.__all__ and "TemporalAccumulator" in P.__all__
    assert (N.REPROJECT_DEVICE, N.REPROJECT_MATCH_OBJECT) == (1, 2)


def test_struct_layout_and_defaults():
    def layout(cls):
        return {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}

    assert ctypes.sizeof(N.ReprojectParams) == 48
    assert layout(N.ReprojectParams) == dict(width=0, height=4, flags=8, samples=12, max_history=16, depth_tol=20,
                                             normal_tol=24, tangent_tol=28, coverage_tol=32, reserved=36)
    assert ctypes.sizeof(N.Camera) == 52 and ctypes.sizeof(N.AovBuffers) == 48
    assert ctypes.sizeof(N.ReprojectFrame) == 128
    assert layout(N.ReprojectFrame) == dict(camera=0, reserved=52, colour=56, variance=64, length=72, aov=80)
    assert ctypes.sizeof(N.ReprojectOut) == 32
    assert layout(N.ReprojectOut) == dict(colour=0, length=8, variance=16, motion=24)
    p = N.ReprojectParams(7, 7, 7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, (ctypes.c_uint32 * 3)(7, 7, 7))
    N.load_library().khp_reproject_params_defaults(ctypes.byref(p))
    assert (p.width, p.height, p.flags, list(p.reserved)) == (0, 0, 0, [0, 0, 0])
    got = (p.samples, p.max_history, p.depth_tol, p.normal_tol, p.tangent_tol, p.coverage_tol)
    assert got == tuple(float(F32(v)) for v in (1.0, 32.0, 0.05, 0.0, 0.25, 0.5))
    assert {k: R.DEFAULTS[k] for k in ("samples", "max_history") + TOLS} == \
        dict(zip(("samples", "max_history") + TOLS, (1.0, 32.0, 0.05, 0.0, 0.25, 0.5)))
    N.load_library().khp_reproject_params_defaults(None)         # a null pointer is ignored


# ---- refusals ----------------------------------------------------------------------------------------------
POISON_PTR = 0x10                                               # never dereferenced: a read would fault
PLANES = ("normal", "tangent", "depth", "coverage", "object")


def _poison(ctype=ctypes.c_float, at=POISON_PTR):
    return ctypes.cast(at, ctypes.POINTER(ctype))


def _frame(history, **null):
    """A khp_reproject_frame whose every plane is a poison pointer, but for those named in `null`."""
    f = N.ReprojectFrame(camera=scenes.camera((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 8, 8))
    for k in ("colour", "variance") + (("length",) if history else ()):
        if not null.get(k):
            setattr(f, k, _poison())
    for ch in PLANES:
        if not null.get(ch):
            setattr(f.aov, ch, _poison(ctypes.c_int32 if ch == "object" else ctypes.c_float))
    return f


def _out(*names):
    o = N.ReprojectOut()
    for k in names:
        setattr(o, k, _poison(at=POISON_PTR + 0x20))             # another address than the frames' planes
    return o


def _refusals(call, err, host):
    """Every refusal of the header through `call(p, cur, hist, out)`; the arguments may be None."""
    good = lambda **kw: N.ReprojectParams.defaults(width=8, height=8, **kw)
    cur, hist, out = _frame(False), _frame(True), _out(*OUTPUTS)
    ref = lambda s: ctypes.byref(s) if s is not None else None

    def bad(word, p=None, c=cur, h=hist, o=out):
        st = call(ref(p if p is not None else good()), ref(c), ref(h), ref(o))
        assert st == N.KHP_EINVAL and word in err(), f"{word!r} not refused as such: status {st}, {err()!r}"

    assert call(None, ref(cur), ref(hist), ref(out)) == N.KHP_EINVAL and "null" in err()
    bad("null", c=None)
    bad("null", o=None)
    for w, h in ((0, 8), (8, 0)):
        p = good()
        p.width, p.height = w, h
        bad("width", p)
    p = good()
    p.width, p.height = 1 << 16, (1 << 15) + 1
    bad("large", p)
    for flags in (1 << 2, 1 << 31, 7):
        bad("flags", good(flags=flags))
    for k in range(3):
        p = good()
        p.reserved[k] = 1
        bad("reserved", p)
    for which in (0, 1):
        frames = [_frame(False), _frame(True)]
        frames[which].reserved = 1
        bad("reserved", c=frames[0], h=frames[1])
    for v in (0.0, -1.0, math.nan, math.inf, -math.inf):
        bad("samples", good(samples=v))
    for field in ("max_history",) + TOLS:
        for v in (-1.0, -1e-30, math.nan, -math.inf):
            bad(field, good(**{field: v}))
    bad("every output is null", o=_out())
    bad("colour", c=_frame(False, colour=True))
    bad("colour", h=_frame(True, colour=True))
    for plane in ("depth", "coverage"):                          # the current frame's: they locate the pixel
        bad(plane, good(**ALL_OFF), c=_frame(False, **{plane: True}))
        bad(plane, good(**ALL_OFF), c=_frame(False, **{plane: True}), h=None)
    bad("length", h=_frame(True, length=True))
    # an enabled test whose plane is null in either frame
    for plane in ("depth", "normal", "tangent", "coverage"):
        p = good(**{**ALL_OFF, plane + "_tol": 0.5})
        if plane not in ("depth", "coverage"):
            bad(plane, p, c=_frame(False, **{plane: True}))
        bad(plane, p, h=_frame(True, **{plane: True}))
    for plane in ("depth", "normal", "tangent"):                # the history's coverage divides them
        bad("coverage", good(**{**ALL_OFF, plane + "_tol": 0.5}), h=_frame(True, coverage=True))
    p = good(flags=N.REPROJECT_MATCH_OBJECT, **ALL_OFF)
    bad("object", p, c=_frame(False, object=True))
    bad("object", p, h=_frame(True, object=True))
    # an output that is a plane of the history
    for name in OUTPUTS:
        for plane in ("colour", "variance", "length"):
            h, o = _frame(True), _out(*OUTPUTS)
            setattr(h, plane, ctypes.cast(0x20, ctypes.POINTER(ctypes.c_float)))
            setattr(o, name, ctypes.cast(0x20, ctypes.POINTER(ctypes.c_float)))
            bad("history", h=h, o=o)
    h, o = _frame(True), _out(*OUTPUTS)
    h.aov.depth = ctypes.cast(0x20, ctypes.POINTER(ctypes.c_float))
    o.colour = ctypes.cast(0x20, ctypes.POINTER(ctypes.c_float))
    bad("history", h=h, o=o)
    if host:
        bad("KHP_REPROJECT_DEVICE", good(flags=N.REPROJECT_DEVICE))


def test_host_entry_refusals_name_their_cause():
    lib = N.load_library()
    _refusals(lambda p, c, h, o: lib.khp_reproject_host(p, c, h, o), lambda: lib.khp_last_error().decode(), host=True)


def test_device_entry_refuses_arguments_before_the_context():
    """With a null context every refusal of an argument still names its own cause; a call whose arguments
    are all good reaches the context check, 'ctx is null', and has read none of the poisoned planes."""
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    _refusals(lambda p, c, h, o: lib.khp_reproject(None, p, c, h, o), err, host=False)
    cur, hist, out = _frame(False), _frame(True), _out(*OUTPUTS)
    for flags in (0, N.REPROJECT_DEVICE, N.REPROJECT_MATCH_OBJECT):
        p = N.ReprojectParams.defaults(width=8, height=8, flags=flags, normal_tol=0.2)
        for h in (ctypes.byref(hist), None):
            assert lib.khp_reproject(None, ctypes.byref(p), ctypes.byref(cur), h, ctypes.byref(out)) == N.KHP_EINVAL
            assert "ctx is null" in err()


def test_wrappers_check_arrays_before_the_native_call():
    ctx = HipContext.__new__(HipContext)                       # no device: the checks come before the call
    cam = scenes.camera((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 4, 4)
    cur = R.random_frame(4, 4, cam, 1, False, bad=False)
    with pytest.raises(ValueError, match="float32"):
        HipContext.reproject(ctx, 4, 4, dict(cur, colour=cur["colour"].astype(np.float64)))
    with pytest.raises(ValueError, match="shape"):
        HipContext.reproject(ctx, 4, 4, dict(cur, variance=cur["variance"][:3].copy()))
    with pytest.raises(ValueError, match="int32"):
        HipContext.reproject(ctx, 4, 4, dict(cur, aov=dict(cur["aov"], object=cur["aov"]["object"].astype(np.int64))))
    with pytest.raises(ValueError, match="Camera"):
        HipContext.reproject(ctx, 4, 4, dict(cur, camera=None))
    with pytest.raises(ValueError, match="DeviceBuffer"):
        HipContext.reproject(ctx, 4, 4, cur, device=True)
    with pytest.raises(ValueError, match="no field"):
        HipContext.reproject(ctx, 4, 4, cur, depth_tolerance=1.0)
    with pytest.raises(ValueError, match="no output"):
        P.reproject_host(4, 4, cur, out={"color": None})
    with pytest.raises(ValueError, match="no entry"):
        P.reproject_host(4, 4, dict(cur, colours=1))
    with pytest.raises(ValueError, match="push"):
        P.TemporalAccumulator(4, 4, samples=2.0)
    with pytest.raises(N.KhpError, match="every output"):
        P.reproject_host(4, 4, cur, out={k: None for k in OUTPUTS})
    ctx.ptr = None                                             # keep __del__ from closing what never opened


# ---- the host entry against the restatement ------------------------------------------------------------------
SIZES = [(13, 9), (67, 35), (130, 3), (1, 1)]
# every test alone, all of them, none; the cap on and off; another weight
COMBOS = [{}, dict(ALL_OFF), dict(ALL_OFF, match_object=True), dict(max_history=4.0), dict(max_history=0.0, samples=4.0),
          dict(depth_tol=0.1, normal_tol=0.3, tangent_tol=0.5, coverage_tol=0.6, match_object=True)] + \
         [dict(ALL_OFF, **{t: v}) for t, v in zip(TOLS, (0.05, 0.3, 0.5, 0.4))]


@functools.lru_cache(maxsize=None)
def cases(w, h):
    """[(name, cur, hist)]: every camera pair of _reprojectref.camera_pairs with seeded frames; read only."""
    res = []
    for k, (name, cc, hc) in enumerate(R.camera_pairs(scenes, w, h, 11 + w)):
        res.append((name, R.freeze(R.random_frame(w, h, cc, 100 + 7 * k + w, False)),
                    R.freeze(R.random_frame(w, h, hc, 200 + 7 * k + w, True))))
    return res


def test_the_cases_hold_what_they_should():
    """Over the sizes and camera pairs of the bit-exactness test: every situation the definition names."""
    seen = dict.fromkeys(("cur not finite", "hist not finite", "background", "fractional coverage", "unknown v_c",
                          "unknown v_q", "zero length", "behind", "degenerate", "left", "right", "top", "bottom", "have",
                          "repaired", "disoccluded", "dead", "rejected tap", "variance blended", "no normal"), False)
    for w, h in SIZES:
        for _name, cur, hist in cases(w, h):
            i = R.reproject(w, h, cur, hist)["info"]
            cv = cur["aov"]["coverage"]
            seen["cur not finite"] |= bool((~i["fin"]).any())
            seen["hist not finite"] |= not np.isfinite(hist["colour"]).all()
            seen["background"] |= bool((cv == 0).any())
            seen["fractional coverage"] |= bool(((cv > 0) & (cv < 1)).any())
            seen["unknown v_c"] |= bool((~i["vc_known"]).any())
            seen["unknown v_q"] |= bool((~R._known(hist["variance"])).any())
            seen["zero length"] |= bool((hist["length"] == 0).any())
            ok_det = np.isfinite(i["det"]) & (i["det"] != 0)
            seen["behind"] |= bool((ok_det & (i["t"] <= 0)).any())
            seen["degenerate"] |= bool((i["det"] == 0).any())
            c = i["cand"]
            seen["left"] |= bool((c & (i["x0"] == -1)).any())
            seen["right"] |= bool((c & (i["x0"] + 1 == w)).any())
            seen["top"] |= bool((c & (i["y0"] == -1)).any())
            seen["bottom"] |= bool((c & (i["y0"] + 1 == h)).any())
            seen["have"] |= bool((i["have"] & i["fin"]).any())
            seen["repaired"] |= bool((i["have"] & ~i["fin"]).any())
            seen["disoccluded"] |= bool((c & ~i["have"] & i["fin"]).any())
            seen["dead"] |= bool((~i["have"] & ~i["fin"]).any())
            seen["rejected tap"] |= bool((i["have"] & ~i["counted"].all(0)).any())
            seen["variance blended"] |= bool((i["have"] & i["fin"] & i["vc_known"] & i["vh_known"]).any())
            seen["no normal"] |= bool(((cv > 0) & ~cur["aov"]["normal"].any(-1)).any())
    assert all(seen.values()), [k for k, v in seen.items() if not v]


@pytest.mark.parametrize("w,h", SIZES)
def test_host_entry_equals_the_restatement(w, h):
    """All four outputs bit for bit (NaN by position) over the camera pairs and the test combinations, with
    and without the variance planes, and with no history frame."""
    for name, cur, hist in cases(w, h):
        for kw in COMBOS:
            ref, got = R.reproject(w, h, cur, hist, **kw), P.reproject_host(w, h, cur, hist, **kw)
            for k in OUTPUTS:
                assert same(ref[k], got[k]), (name, kw, k)
        for c, hs in ((dict(cur, variance=None), hist), (cur, dict(hist, variance=None)), (cur, None)):
            ref, got = R.reproject(w, h, c, hs, samples=2.0), P.reproject_host(w, h, c, hs, samples=2.0)
            for k in OUTPUTS:
                assert same(ref[k], got[k]), (name, k)
    none = P.reproject_host(w, h, cases(w, h)[0][1], None)
    cur = cases(w, h)[0][1]
    assert np.isnan(none["motion"]).all() and same(none["colour"], cur["colour"])
    fin = np.isfinite(cur["colour"]).all(-1)
    assert (none["length"] == np.where(fin, F32(1.0), F32(0.0))).all()
    known = fin & R._known(cur["variance"])
    assert same(none["variance"], np.where(known, cur["variance"], F32(np.inf)).astype(F32))


def test_outputs_alone_in_place_and_planes_never_read():
    w, h = 67, 35
    name, cur, hist = cases(w, h)[3]
    want = P.reproject_host(w, h, cur, hist)
    for k in OUTPUTS:                                           # each output alone, and each left out
        alone = P.reproject_host(w, h, cur, hist, out={o: None for o in OUTPUTS if o != k})
        assert list(alone) == [k] and same(alone[k], want[k])
        rest = P.reproject_host(w, h, cur, hist, out={k: None})
        assert k not in rest and all(same(rest[o], want[o]) for o in rest)
    buf, vbuf = cur["colour"].copy(), cur["variance"].copy()    # out.colour == cur.colour, out.variance == cur.variance
    res = P.reproject_host(w, h, dict(cur, colour=buf, variance=vbuf), hist, out={"colour": buf, "variance": vbuf})
    assert res["colour"] is buf and same(buf, want["colour"]) and same(vbuf, want["variance"])
    # a plane whose test is off may be missing -- and is not read: poison in it changes nothing
    only_depth = dict(ALL_OFF, depth_tol=0.05)
    ref = P.reproject_host(w, h, cur, hist, **only_depth)
    keep = lambda f: dict(f, aov={ch: f["aov"][ch] for ch in ("depth", "coverage")})
    got = P.reproject_host(w, h, keep(cur), keep(hist), **only_depth)
    assert all(same(ref[k], got[k]) for k in OUTPUTS)
    ref = P.reproject_host(w, h, cur, hist, **ALL_OFF)
    bare = dict(hist, aov={})
    got = P.reproject_host(w, h, keep(cur), bare, **ALL_OFF)
    assert all(same(ref[k], got[k]) for k in OUTPUTS)
    poison = lambda f: dict(f, aov={ch: (a if ch in ("depth", "coverage") else np.full_like(a, 99)) for ch, a in f["aov"].items()})
    got = P.reproject_host(w, h, poison(cur), dict(hist, aov={ch: np.full_like(a, 99) for ch, a in hist["aov"].items()}), **ALL_OFF)
    assert all(same(ref[k], got[k]) for k in OUTPUTS)


# ---- the motion vectors against float64 ----------------------------------------------------------------------
def _truth_motion(w, h, cur, hist_cam):
    """The same geometry in float64, written from the pinhole model and not from the definition's steps: the
    point X on the pixel-centre ray at the frame's depth, and the history pixel as the solution of
    pos' + t (X - pos') = bl' + a ax' + b ay' for (t, a, b) as one 3 x 3 linear system per pixel.
    Returns (motion, the share |det| / (|w| |n|))."""
    f64 = lambda cam: [np.asarray(a, np.float64) for a in R.cam_arrays(cam)]
    pos, bl, ax, ay, ps = f64(cur["camera"])
    hpos, hbl, hax, hay, hps = f64(hist_cam)
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    ray = bl + ax * (xs * ps)[..., None] + ay * (ys * ps)[..., None] - pos
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
    cv = cur["aov"]["coverage"].astype(np.float64)
    surf = cv > 0
    depth = np.where(surf, cur["aov"]["depth"].astype(np.float64) / np.where(surf, cv, 1.0), 0.0)
    wv = np.where(surf[..., None], pos + ray * depth[..., None] - hpos, ray)
    M = np.stack([wv, np.broadcast_to(-hax, wv.shape), np.broadcast_to(-hay, wv.shape)], -1)    # columns
    sol = np.linalg.solve(M, np.broadcast_to(hbl - hpos, wv.shape)[..., None])[..., 0]
    fx, fy = sol[..., 1] / hps, sol[..., 2] / hps
    n = np.cross(hax, hay)
    share = np.abs(wv @ n) / (np.linalg.norm(wv, axis=-1) * np.linalg.norm(n))
    return np.stack([fx - xs, fy - ys], -1), sol[..., 0], share


def test_motion_against_a_float64_evaluation():
    """Scene coordinates within [-2, 2], depths within [0.5, 4], W <= 130.  About 40 float32 operations, each
    within 2^-24 relative on magnitudes <= 4, give about 1e-5 of absolute error; divided by pixel_size >=
    0.036 / 130 that is at most about 0.035 pixel: the bound is 0.05 pixel, over the pixels where |det| is
    at least 1e-3 of |w| |n|.  The share of pixels that leaves out is printed and must stay below 2 %."""
    worst, left_out, total = 0.0, 0, 0
    for w, h in ((67, 35), (130, 87), (13, 9)):
        rng = np.random.default_rng(5 + w)
        base_p, base_l = np.array([0.1, -0.2, 1.9]), np.array([0.0, 0.02, -1.0])
        camA = scenes.camera(base_p, base_l, (0.0, 1.0, 0.0), w, h)
        ps = float(camA.pixel_size)
        assert ps >= 0.036 / 130
        for k in range(6):
            rot = rng.uniform(-4.0, 4.0, 3) * ps * (k % 3 != 0)
            shift = rng.uniform(-0.05, 0.05, 3) * (k % 3 != 1)
            camB = scenes.camera(base_p + shift, base_l + rot, (0.0, 1.0, 0.0), w, h)
            cur = R.random_frame(w, h, camA, 300 + k, False, bad=False)
            depth = rng.uniform(0.5, 2.5, (h, w))
            cov = cur["aov"]["coverage"]
            cur["aov"]["depth"] = (depth * cov).astype(F32)
            for cc, hc in ((camA, camB), (camB, camA)):
                frame = dict(cur, camera=cc)
                got = P.reproject_host(w, h, frame, dict(cur, camera=hc, length=np.ones((h, w), F32)),
                                       out={o: None for o in OUTPUTS if o != "motion"})["motion"]
                want, t, share = _truth_motion(w, h, frame, hc)
                use = share >= 1e-3
                left_out += int((~use).sum())
                total += use.size
                assert (t[use] > 0).all() and np.isfinite(got[use]).all()
                worst = max(worst, float(np.abs(got.astype(np.float64) - want)[use].max()))
    print(f"motion: worst |float32 - float64| {worst:.5f} pixel; {left_out} of {total} pixels left out "
          f"({100.0 * left_out / total:.3f} %)")
    assert left_out / total < 0.02
    assert worst <= 0.05


# ---- known answers that do not go through the restatement ---------------------------------------------------
def _wall(w, h, cam, depth_of, colour, length=None):
    """A frame that sees one wall: full coverage, depth along each pixel-centre ray from depth_of(rays)."""
    pos, bl, ax, ay, ps = (np.asarray(a, np.float64) for a in R.cam_arrays(cam))
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    ray = bl + ax * (xs * ps)[..., None] + ay * (ys * ps)[..., None] - pos
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
    one = np.ones((h, w), F32)
    f = {"camera": cam, "colour": np.ascontiguousarray(np.broadcast_to(colour, (h, w, 3)), F32),
         "aov": {"depth": depth_of(pos, ray).astype(F32), "coverage": one}}
    if length is not None:
        f["length"] = np.full((h, w), length, F32)
    return f


def test_identical_cameras_blend_a_constant_history():
    """The same camera twice and a wall at right angles to its axis: every interior pixel lands on itself,
    so with a constant history colour k and a history length N = 8 (a power of two: bw * N is exact, and
    al / ws is N) the result is k + alpha (c - k) with alpha = s / (N + s) to within 4 ulp, length N + s."""
    w, h, n_hist = 32, 20, 8.0
    cam = scenes.camera((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), w, h)
    plane = lambda pos, ray: (0.0 - pos[2]) / ray[..., 2]          # the wall z = 0
    k = np.array([0.75, 0.625, 0.875], F32)
    rng = np.random.default_rng(3)
    c = (0.5 + 0.5 * rng.random((h, w, 3))).astype(F32)
    for s in (1.0, 2.0):
        cur = _wall(w, h, cam, plane, c)
        hist = _wall(w, h, cam, plane, k, length=n_hist)
        got = P.reproject_host(w, h, cur, hist, samples=s, max_history=0.0, **dict(ALL_OFF, depth_tol=0.05))
        inner = (slice(1, h - 1), slice(1, w - 1))
        assert np.abs(got["motion"][inner]).max() < 1e-3
        assert (got["length"][inner] == F32(n_hist + s)).all()
        alpha = s / (n_hist + s)
        want = k.astype(np.float64) + alpha * (c.astype(np.float64) - k.astype(np.float64))
        ulp = np.spacing(np.abs(want).astype(F32)).astype(np.float64)
        err = np.abs(got["colour"].astype(np.float64) - want) / ulp
        print(f"s = {s}: worst error {err[inner].max():.2f} ulp")
        assert err[inner].max() <= 4.0
        assert np.isposinf(got["variance"]).all()                 # no variance plane: unknown


def test_a_hidden_history_pixel_is_rejected_by_the_depth_test():
    """The current frame sees a far wall; in the history a nearer surface covered where that wall point lands.
    The depth test rejects every tap: the pixel returns c and length s.  With the test off it blends."""
    w, h = 24, 16
    camA = scenes.camera((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), w, h)
    camB = scenes.camera((0.02, 0.0, 2.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), w, h)
    far = lambda pos, ray: (-1.0 - pos[2]) / ray[..., 2]           # z = -1, 3 away
    near = lambda pos, ray: (1.0 - pos[2]) / ray[..., 2]           # z = 1, 1 away
    rng = np.random.default_rng(4)
    c = rng.random((h, w, 3)).astype(F32)
    cur = _wall(w, h, camA, far, c)
    hidden = _wall(w, h, camB, near, F32(9.0), length=20.0)
    got = P.reproject_host(w, h, cur, hidden, samples=3.0, **dict(ALL_OFF, depth_tol=0.05))
    assert np.isfinite(got["motion"]).all()                       # the projection exists; the taps do not count
    assert same(got["colour"], c) and (got["length"] == F32(3.0)).all()
    got = P.reproject_host(w, h, cur, hidden, samples=3.0, **ALL_OFF)
    landed = got["length"] > 3.0
    assert landed.mean() > 0.8 and (got["colour"][landed] > 1.0).all()
    # the same wall in both frames passes the test
    seen = _wall(w, h, camB, far, F32(9.0), length=20.0)
    got = P.reproject_host(w, h, cur, seen, samples=3.0, **dict(ALL_OFF, depth_tol=0.05))
    assert (got["length"] > 3.0).mean() > 0.8


def test_the_accumulator_is_the_chain_of_calls():
    w, h = 13, 9
    frames = [hf for _n, _c, hf in cases(w, h)[:4]]                # four cameras
    acc = P.TemporalAccumulator(w, h, max_history=6.0)
    assert acc.history is None
    hist, kept = None, []
    for k, f in enumerate(frames):
        got = acc.push(f["camera"], f["aov"], f["colour"], f["variance"], samples=k + 1.0)
        want = P.reproject_host(w, h, f, hist, samples=k + 1.0, max_history=6.0)
        assert all(same(got[o], want[o]) for o in OUTPUTS), k
        hist = dict(f, colour=want["colour"], variance=want["variance"], length=want["length"])
        kept.append((got, {o: want[o].copy() for o in OUTPUTS}))
        if k:                                                   # the previous push's outputs are still as they were
            assert all(same(kept[k - 1][0][o], kept[k - 1][1][o]) for o in OUTPUTS)
    assert np.isnan(kept[0][1]["motion"]).all() and np.isfinite(kept[1][1]["motion"]).any()
    acc.reset()
    assert acc.history is None
    f = frames[0]
    assert np.isnan(acc.push(f["camera"], f["aov"], f["colour"], f["variance"])["motion"]).all()


# ---- quality --------------------------------------------------------------------------------------------------
QW, QH, QDEPTH, QPASSES, QSEED = 96, 64, 5, 16, 1


@functools.lru_cache(maxsize=None)
def quality_frames():
    """Oracle frames of the small hairball: QPASSES 1-spp passes at camera A (their mean and the variance of
    that mean), one further pass at camera B, A turned by about one pixel, and a many-sample frame at B."""
    sd = scenes.config2(QW, QH, n_strands=200)
    camA = sd.cam
    ps = float(camA.pixel_size)
    pos, bl, ax, ay, _ps = R.cam_arrays(camA)
    look = np.cross(ax.astype(np.float64), ay.astype(np.float64)) * -1.0                # the axis camA looks along
    camB = scenes.camera(pos, look + 1.0 * ps * ax + 0.4 * ps * ay, (0.0, 1.0, 0.0), QW, QH)
    oa, ob = oracle_ffi.Oracle(sd), oracle_ffi.Oracle(dataclasses.replace(sd, cam=camB))
    with np.errstate(all="ignore"):
        cols = np.stack([(F32(k + 1) * oa.render(QW, QH, 1, QDEPTH, seed=QSEED, first_sample=k)).astype(F32)
                         for k in range(QPASSES)])
        one = (F32(QPASSES + 1) * ob.render(QW, QH, 1, QDEPTH, seed=QSEED, first_sample=QPASSES)).astype(F32)
    st = P.moments_fold_host(cols)
    total, count = np.zeros((QH, QW, 3), np.float64), np.zeros((QH, QW, 3), np.int64)
    for seed in range(2000, 2064):                              # the per-pixel float64 mean over finite values
        f = ob.render(QW, QH, 8, QDEPTH, seed=seed)
        fin = np.isfinite(f)
        total += np.where(fin, f, 0.0)
        count += fin
    assert count.min() >= 32, count.min()
    planes = lambda g: {ch: np.ascontiguousarray(g[ch]) for ch in ("normal", "tangent", "depth", "coverage", "object")}
    aovA = planes(A.reference(oa, sd, QW, QH, QPASSES, QSEED))
    aovB = planes(A.reference(oa, sd, QW, QH, 1, QSEED, first_sample=QPASSES, cam=camB))
    nf = st["count"].astype(F32)
    with np.errstate(all="ignore"):                             # KHP_NOISE_PLANE's quantity: the variance of the mean, channels summed
        var = np.where(st["count"] >= 2, ((st["m2"][..., 0] + st["m2"][..., 1]) + st["m2"][..., 2]) / (nf * (nf - F32(1.0))),
                       F32(np.nan)).astype(F32)
    return dict(camA=camA, camB=camB, meanA=st["mean"], varA=var, one=one, aovA=aovA, aovB=aovB,
                ref=total / count)


def test_a_pushed_frame_is_nearer_the_reference_than_the_pass_alone():
    """Measured: the RMSE of the frame pushed after the camera move is below the single
    pass's own, and at least half of the surface pixels found their history."""
    q = quality_frames()
    acc = P.TemporalAccumulator(QW, QH)                         # the defaults
    first = acc.push(q["camA"], q["aovA"], q["meanA"], q["varA"], samples=float(QPASSES))
    assert same(first["colour"], q["meanA"])
    pushed = acc.push(q["camB"], q["aovB"], q["one"], samples=1.0)
    info = R.reproject(QW, QH, {"camera": q["camB"], "colour": q["one"], "aov": q["aovB"]},
                       {"camera": q["camA"], "colour": first["colour"], "length": first["length"],
                        "variance": first["variance"], "aov": q["aovA"]})["info"]
    surf = q["aovB"]["coverage"] > 0
    share = float(info["have"][surf].mean())
    fin = np.isfinite(q["one"]).all(-1) & np.isfinite(pushed["colour"]).all(-1)
    rmse = lambda f: float(np.sqrt(np.mean((f[fin].astype(np.float64) - q["ref"][fin]) ** 2)))
    alone, both = rmse(q["one"]), rmse(pushed["colour"])
    moved = np.nanmedian(np.hypot(pushed["motion"][..., 0], pushed["motion"][..., 1]))
    print(f"camera turned by {moved:.2f} pixel: RMSE of the pass alone {alone:.4f}, of the pushed frame {both:.4f} "
          f"(ratio {both / alone:.3f}); {100 * share:.1f} % of {int(surf.sum())} surface pixels have a history")
    assert (pushed["length"][info["have"] & fin] > 1.0).all()
    assert share >= 0.5
    assert both < alone
