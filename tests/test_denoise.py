"""khp_denoise without a device: the exports and the struct, the refusals (each before the
context is touched), khp_denoise_host against the numpy restatement (tests/_denoiseref.py) bit
for bit, known answers that do not go through the restatement, and the filter's quality on
oracle frames (GPU frames are bit-identical to the oracle's)."""
import ctypes
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
import _denoiseref as R
import oracle_ffi

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("normal", "albedo", "tangent", "depth", "coverage")
SIGMAS = ("sigma_color", "sigma_normal", "sigma_tangent", "sigma_depth", "sigma_coverage")
ALL_OFF = {s: 0.0 for s in SIGMAS}


# ---- export and layout -------------------------------------------------------------------------------------
def test_symbols_are_exported_listed_and_declared():
    lib = N.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    for sym in ("khp_denoise", "khp_denoise_host", "khp_denoise_params_defaults"):
        assert sym in N.EXPORTED and hasattr(lib, sym)
        assert re.search(r"\bT %s\b" % sym, out), sym
    header = open(os.path.join(ROOT, "include", "kirk_hip.h")).read()
    flat = " ".join(header.split())
    assert ("khp_status khp_denoise(khp_ctx* ctx, const khp_denoise_params* p, const float* colour, "
            "const khp_aov_buffers* guides, float* out);") in flat
    assert ("khp_status khp_denoise_host(const khp_denoise_params* p, const float* colour, "
            "const khp_aov_buffers* guides, float* out);") in flat
    assert "void khp_denoise_params_defaults(khp_denoise_params* out);" in flat
    assert "#define KHP_DENOISE_DEVICE (1u << 0)" in flat and "#define KHP_DENOISE_DEMODULATE (1u << 1)" in flat
    # symbols added, nothing moved: the ABI number stays
    assert "#define KHP_ABI_VERSION 17" in header and N.ABI_VERSION == 17 and lib.khp_abi_version() == 17
    assert "denoise" in open(os.path.join(ROOT, "include", "kirk_hip.hpp")).read()
    assert callable(HipContext.denoise) and callable(P.denoise_host)
    for name in ("DenoiseParams", "DENOISE_DEVICE", "DENOISE_DEMODULATE"):
        assert name in P.__all__ and getattr(P, name) is getattr(N, name)
    assert "denoise_host" in P.__all__
    assert (N.DENOISE_DEVICE, N.DENOISE_DEMODULATE) == (1, 2)


def test_struct_layout_and_defaults():
    assert ctypes.sizeof(N.DenoiseParams) == 48
    names = ["width", "height", "iterations", "flags", "sigma_color", "sigma_normal", "sigma_tangent", "sigma_depth",
             "sigma_coverage", "clamp", "reserved"]
    assert [f[0] for f in N.DenoiseParams._fields_] == names
    assert [getattr(N.DenoiseParams, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    p = N.DenoiseParams(width=7, height=7, iterations=7, flags=7, clamp=7.0)
    p.reserved[0] = p.reserved[1] = 7
    N.load_library().khp_denoise_params_defaults(ctypes.byref(p))
    assert (p.width, p.height, p.iterations, p.flags, tuple(p.reserved)) == (0, 0, 5, 0, (0, 0))
    got = [p.sigma_color, p.sigma_normal, p.sigma_tangent, p.sigma_depth, p.sigma_coverage, p.clamp]
    assert got == [float(F32(v)) for v in (4, 0.35, 0.35, 0.05, 0.25, 0)]
    assert R.DEFAULTS == dict(iterations=5, sigma_color=4.0, sigma_normal=0.35, sigma_tangent=0.35,
                              sigma_depth=0.05, sigma_coverage=0.25, clamp=0.0)
    N.load_library().khp_denoise_params_defaults(None)          # a null pointer is ignored


# ---- refusals ----------------------------------------------------------------------------------------------
def _call_args(n=64, **drop):
    keep = {ch: np.zeros((n,) + N.AOV_CHANNELS[ch][0], F32) for ch in PLANES if not drop.get(ch)}
    buf = N.AovBuffers()
    for ch, a in keep.items():
        setattr(buf, ch, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    colour, out = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    return buf, colour, out, keep


def _refusals(call, err, host):
    """Every KHP_EINVAL of the header, through `call(p, colour, guides, out)`; pointers may be None."""
    buf, colour, out, _keep = _call_args()
    cp, op, bp = colour.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(buf)
    good = lambda **kw: N.DenoiseParams.defaults(width=8, height=8, **kw)
    bad = lambda p, word: (call(ctypes.byref(p), cp, bp, op) == N.KHP_EINVAL and word in err()) or pytest.fail(
        f"{word!r} not refused as such: {err()!r}")
    assert call(None, cp, bp, op) == N.KHP_EINVAL and "null" in err()
    assert call(ctypes.byref(good()), cp, None, op) == N.KHP_EINVAL and "null" in err()
    assert call(ctypes.byref(good()), cp, bp, None) == N.KHP_EINVAL and "null" in err()
    for w, h in ((0, 8), (8, 0), (0, 0)):
        p = good()
        p.width, p.height = w, h
        bad(p, "width")
    p = good()
    p.width, p.height = 1 << 16, (1 << 15) + 1
    bad(p, "large")
    for it in (0, 9, 1 << 31):
        bad(good(iterations=it), "iterations")
    for flags in (1 << 2, 1 << 31, 3 | (1 << 7)):
        bad(good(flags=flags), "flags")
    if host:
        bad(good(flags=N.DENOISE_DEVICE), "KHP_DENOISE_DEVICE")
        assert call(ctypes.byref(good()), None, bp, op) == N.KHP_EINVAL and "colour" in err()
    for k in (0, 1):
        p = good()
        p.reserved[k] = 1
        bad(p, "reserved")
    for field in SIGMAS + ("clamp",):
        for v in (-1.0, -1e-30, math.nan, math.inf, -math.inf):
            bad(good(**{field: v}), field)
    for plane in ("normal", "tangent", "depth", "coverage"):
        nb, _c, _o, _k = _call_args(**{plane: True})
        p = good(**{**ALL_OFF, "sigma_" + plane: 0.5})
        assert call(ctypes.byref(p), cp, ctypes.byref(nb), op) == N.KHP_EINVAL and plane in err(), (plane, err())
    nb, _c, _o, _k = _call_args(albedo=True)
    assert call(ctypes.byref(good(flags=N.DENOISE_DEMODULATE)), cp, ctypes.byref(nb), op) == N.KHP_EINVAL
    assert "albedo" in err()
    nb, _c, _o, _k = _call_args(coverage=True)
    for kw in ({"sigma_normal": 0.5}, {"sigma_tangent": 0.5}, {"sigma_depth": 0.5}, {"flags": N.DENOISE_DEMODULATE}):
        p = good(**{**ALL_OFF, **kw})
        assert call(ctypes.byref(p), cp, ctypes.byref(nb), op) == N.KHP_EINVAL and "coverage" in err(), (kw, err())


def test_host_entry_refusals_name_their_cause():
    lib = N.load_library()
    _refusals(lambda p, c, g, o: lib.khp_denoise_host(p, c, g, o), lambda: lib.khp_last_error().decode(), host=True)


def test_device_entry_refuses_arguments_before_the_context():
    """With a null context every refusal of an argument still names its own cause; a call whose
    arguments are all good reaches the context check: 'ctx is null'."""
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    _refusals(lambda p, c, g, o: lib.khp_denoise(None, p, c, g, o), err, host=False)
    buf, colour, out, _keep = _call_args()
    cp, op = colour.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for flags in (0, N.DENOISE_DEVICE, N.DENOISE_DEMODULATE, N.DENOISE_DEVICE | N.DENOISE_DEMODULATE):
        p = N.DenoiseParams.defaults(width=8, height=8, flags=flags)
        for c in (cp, None):                                    # colour == NULL is the framebuffer: needs a context
            assert lib.khp_denoise(None, ctypes.byref(p), c, ctypes.byref(buf), op) == N.KHP_EINVAL
            assert "ctx is null" in err()


def test_wrappers_check_arrays_before_the_native_call():
    ctx = HipContext.__new__(HipContext)                       # no device: the checks come before the call
    c, g = R.random_case(4, 4, 1, bad=False)
    with pytest.raises(ValueError, match="no channel"):
        HipContext.denoise(ctx, 4, 4, {"colour": c}, c)
    with pytest.raises(ValueError, match="float32"):
        HipContext.denoise(ctx, 4, 4, {**g, "depth": g["depth"].astype(np.float64)}, c)
    with pytest.raises(ValueError, match="shape"):
        HipContext.denoise(ctx, 4, 4, {**g, "normal": g["depth"]}, c)
    with pytest.raises(ValueError, match="colour"):
        HipContext.denoise(ctx, 4, 4, g, c[:, :, :2].copy())
    with pytest.raises(ValueError, match="DeviceBuffer"):
        HipContext.denoise(ctx, 4, 4, g, c, device=True)
    with pytest.raises(ValueError, match="no field"):
        HipContext.denoise(ctx, 4, 4, g, c, sigma_colour=1.0)
    with pytest.raises(ValueError, match="out"):
        P.denoise_host(4, 4, g, c, out=np.zeros((4, 4), F32))
    ctx.ptr = None                                             # keep __del__ from closing what never opened


# ---- the restatement's k_expf is the product's ----------------------------------------------------------------
def test_restated_expf_is_kmath_expf():
    """ko_expf is kmath.h's k_expf in the oracle (parity with the product is bit-exact by design)."""
    L = oracle_ffi.load()
    rng = np.random.default_rng(5)
    xs = np.concatenate([-(rng.random(3000) * 120.0), -(rng.random(1000) * 2.0), -(10.0 ** rng.uniform(-8, 3, 1000)),
                         [0.0, -0.0, -87.3, -88.0, -103.27, -103.2789, -103.279, -104.0, 88.7, 88.73, 5.0, np.inf,
                          -np.inf, -1e-45]]).astype(F32)
    got = R.k_expf(xs)
    want = F32([L.ko_expf(float(x)) for x in xs])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(R.k_expf(F32([np.nan])))[0]


# ---- the host entry against the restatement ------------------------------------------------------------------
SIZES = [(13, 9), (1, 1), (5, 3), (67, 35)]


def _both(w, h, c, g, **kw):
    ref = R.denoise(c, g, **kw)
    got = P.denoise_host(w, h, g, c.copy(), **kw)
    return ref, got


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("demodulate", [False, True])
def test_host_entry_equals_the_restatement(w, h, demodulate):
    """Iterations 1..8 (at 13 x 9 every step from 4 on loses taps to the border, from 16 on only
    the centre tap remains), NaN, +inf, -inf and 1e38 pixels, a NaN patch and a coverage-0 pixel."""
    c, g = R.random_case(w, h, 100 + w)
    for it in range(1, 9):
        ref, got = _both(w, h, c, g, iterations=it, demodulate=demodulate)
        assert R.same(ref, got), (w, h, it, demodulate)


@pytest.mark.parametrize("w,h", SIZES)
def test_each_sigma_alone_all_and_none(w, h):
    c, g = R.random_case(w, h, 200 + w)
    tried = [{**ALL_OFF, s: v} for s, v in zip(SIGMAS, (1.5, 0.35, 0.35, 0.05, 0.25))]
    tried += [dict(zip(SIGMAS, (1.5, 0.5, 0.7, 0.3, 0.6))), dict(ALL_OFF)]
    outs = []
    for kw in tried:
        ref, got = _both(w, h, c, g, iterations=3, **kw)
        assert R.same(ref, got), kw
        outs.append(R.bits(got).tobytes())
    if w * h > 15:
        assert len(set(outs)) == len(outs)                      # every term does something of its own


@pytest.mark.parametrize("w,h", SIZES)
def test_clamp_in_place_and_null_planes(w, h):
    c, g = R.random_case(w, h, 300 + w)
    ref, got = _both(w, h, c, g, iterations=2, clamp=1.25)
    assert R.same(ref, got)
    fin = np.isfinite(got)
    assert (got[fin] <= 1.25 * (1 + 1e-5)).all()                # a mean of values clamped to 1.25, 1e38 and +inf included
    # in place
    ref = R.denoise(c, g, iterations=4, demodulate=True)
    buf = c.copy()
    assert P.denoise_host(w, h, g, buf, out=buf, iterations=4, demodulate=True) is buf
    assert R.same(ref, buf)
    # a plane whose term is off may be NULL -- and is not read: poison in it changes nothing
    only_colour = {**ALL_OFF, "sigma_color": 1.0}
    ref = R.denoise(c, {}, iterations=3, **only_colour)
    assert R.same(ref, P.denoise_host(w, h, {}, c, iterations=3, **only_colour))
    poison = {ch: np.full_like(a, np.nan) for ch, a in g.items()}
    assert R.same(ref, P.denoise_host(w, h, poison, c, iterations=3, **only_colour))
    kw = {**ALL_OFF, "sigma_depth": 0.2, "sigma_coverage": 0.4}
    some = {"depth": g["depth"], "coverage": g["coverage"], "normal": None}
    assert R.same(R.denoise(c, some, iterations=3, **kw), P.denoise_host(w, h, some, c, iterations=3, **kw))


def test_bad_pixels_are_repaired_and_never_spread():
    w, h = 13, 9
    c, g = R.random_case(w, h, 11, bad=False)
    clean = P.denoise_host(w, h, g, c, **ALL_OFF, iterations=1)
    for v in (np.nan, np.inf, -np.inf):
        d = c.copy()
        d[4, 6, 1] = v
        ref, got = _both(w, h, d, g, **ALL_OFF, iterations=1)
        assert R.same(ref, got) and np.isfinite(got).all()
        far = np.ones((h, w), bool)
        far[2:7, 4:9] = False                                   # outside the bad pixel's 5 x 5 reach nothing changed
        assert np.array_equal(got[far], clean[far])
    d = c.copy()
    d[4, 6] = 1e38                                              # finite: it takes part, and overflows its neighbours' sums
    ref, got = _both(w, h, d, g, iterations=5)
    assert R.same(ref, got)


def test_a_nan_pixel_among_nan_pixels_comes_back_unchanged():
    w, h = 13, 9
    c, g = R.random_case(w, h, 12)                              # rows and columns 1..7 are NaN
    ref, got = _both(w, h, c, g, iterations=1)
    assert R.same(ref, got)
    assert np.isnan(got[4, 4]).all() and np.isnan(c[4, 4]).all()   # every tap of (4, 4) at step 1 is NaN
    assert np.isfinite(got[1, 1]).all()                         # the patch's rim is repaired from outside
    every = np.full((h, w, 3), np.nan, F32)
    every.view(np.uint32)[...] = 0x7FC12345                     # a payload: the bits must come back, not a new NaN
    got = P.denoise_host(w, h, g, every, iterations=8)
    assert np.array_equal(got.view(np.uint32), every.view(np.uint32))


def test_a_coverage_zero_pixel_among_covered_ones():
    w, h = 13, 9
    c, g = R.random_case(w, h, 13, bad=False)
    assert g["coverage"][h // 2, w // 2] == 0 and not g["normal"][h // 2, w // 2].any()
    for demodulate in (False, True):
        ref, got = _both(w, h, c, g, iterations=3, demodulate=demodulate)
        assert R.same(ref, got) and np.isfinite(got).all()


# ---- known answers that do not go through the restatement ---------------------------------------------------
def test_impulse_gives_the_b3_kernel():
    """A unit impulse, one iteration, all sigmas 0.  The definition divides by the weight that fell
    inside the image, so at 5 x 5 only the centre pixel has the whole support (ws = 1) and gives
    h (x) h's 9/64; every other pixel gives its h (x) h entry over its inside weight (1/121 in the
    corners, not 1/256).  Both are checked by hand, and at 9 x 9, where the support of every pixel
    the impulse reaches lies inside, the output is exactly h (x) h."""
    c = np.zeros((5, 5, 3), F32)
    c[2, 2] = 1.0
    got = P.denoise_host(5, 5, {}, c, iterations=1, **ALL_OFF)
    h5 = np.array([1, 4, 6, 4, 1], np.float64) / 16.0
    want = np.outer(h5, h5)                                     # dyadic: every weight and every sum is exact
    # pixel p's tap at the centre has weight h[dy] h[dx] of ws = the sum of the taps inside the image
    for y in range(5):
        for x in range(5):
            inside = np.outer(h5[max(0, 2 - y):5 - max(0, y - 2)], h5[max(0, 2 - x):5 - max(0, x - 2)]).sum()
            assert np.array_equal(got[y, x], np.full(3, F32(want[y, x]) / F32(inside))), (y, x)   # both exact in float32
    assert np.array_equal(got[2, 2], np.full(3, F32(9.0 / 64.0)))
    # with the whole support inside the image the output is h (x) h itself
    big = np.zeros((9, 9, 3), F32)
    big[4, 4] = 1.0
    got = P.denoise_host(9, 9, {}, big, iterations=1, **ALL_OFF)
    assert np.array_equal(got[2:7, 2:7, 0], want.astype(F32)) and np.array_equal(got[..., 0], got[..., 2])
    assert not got[:2].any() and not got[7:].any() and not got[:, :2].any() and not got[:, 7:].any()


@pytest.mark.parametrize("demodulate", [False, True])
def test_a_constant_frame_comes_back_bit_for_bit(demodulate):
    w, h = 13, 9
    _c, g = R.random_case(w, h, 21)
    c = np.full((h, w, 3), 0.5, F32)
    if demodulate:                                              # c / m * m need not be c: pick m a power of two
        g["albedo"] = (np.full((h, w, 3), 2.0, F32) - (F32(1.0) - g["coverage"])[..., None]).astype(F32)
    got = P.denoise_host(w, h, g, c, iterations=5, demodulate=demodulate)
    assert np.array_equal(got.view(np.uint32), c.view(np.uint32))


def test_no_value_crosses_a_normal_edge():
    """k_expf(-4e4) = 0: with sigma_normal 0.01 a tap across the edge weighs nothing."""
    w, h = 12, 8
    n = np.zeros((h, w, 3), F32)
    n[:, :6, 2], n[:, 6:, 2] = 1.0, -1.0
    c = np.zeros((h, w, 3), F32)
    c[:, :6], c[:, 6:] = 0.5, 2.0
    g = {"normal": n, "coverage": np.ones((h, w), F32)}
    got = P.denoise_host(w, h, g, c, iterations=4, **{**ALL_OFF, "sigma_normal": 0.01})
    assert np.array_equal(got.view(np.uint32), c.view(np.uint32))
    blurred = P.denoise_host(w, h, g, c, iterations=4, **ALL_OFF)      # the edge is what keeps them apart
    assert 0.5 < blurred[4, 5, 0] < 2.0


# ---- quality --------------------------------------------------------------------------------------------------
QW, QH, QDEPTH = 48, 32, 5


@pytest.fixture(scope="module")
def quality_scene():
    sd = scenes.config2(QW, QH, n_strands=200)
    o = oracle_ffi.Oracle(sd)
    total, count = np.zeros((QH, QW, 3), np.float64), np.zeros((QH, QW, 3), np.int64)
    for seed in range(1000, 1064):                              # the per-pixel float64 mean over finite values
        f = o.render(QW, QH, 8, QDEPTH, seed=seed)
        fin = np.isfinite(f)
        total += np.where(fin, f, 0.0)
        count += fin
    assert count.min() >= 32, count.min()
    return sd, o, total / count


@pytest.mark.parametrize("spp", [1, 2, 4])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_denoised_frames_are_nearer_the_reference(quality_scene, spp, seed):
    """Measured: RMSE ratio 0.710 .. 0.873 over the nine cases, at most 8 pixels excluded."""
    sd, o, ref = quality_scene
    raw = o.render(QW, QH, spp, QDEPTH, seed=seed)
    g = A.reference(o, sd, QW, QH, spp, seed)
    guides = {ch: np.ascontiguousarray(g[ch], F32) for ch in PLANES}
    out = P.denoise_host(QW, QH, guides, raw, iterations=5, flags=0, sigma_color=4.0, sigma_normal=0.35,
                         sigma_tangent=0.35, sigma_depth=0.05, sigma_coverage=0.25)
    assert np.isfinite(out).all()
    keep = np.isfinite(raw).all(-1)
    excluded = int((~keep).sum())
    rmse = lambda f: float(np.sqrt(np.mean((f[keep].astype(np.float64) - ref[keep]) ** 2)))
    r_raw, r_out = rmse(raw), rmse(out)
    print(f"spp {spp} seed {seed}: raw {r_raw:.4f} denoised {r_out:.4f} ratio {r_out / r_raw:.3f} excluded {excluded}")
    assert excluded <= 16
    assert r_out < r_raw
