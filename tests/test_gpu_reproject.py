"""khp_reproject on the GPU: the kernel bit for bit against the numpy restatement
(tests/_reprojectref.py) and against khp_reproject_host, the plumbing (host and device pointers, in
place, poisoned outputs, outputs left out, the staging area regrowing), that the context is left
alone, and a TemporalAccumulator on device buffers across a real camera move."""
import ctypes
import functools

import numpy as np
import pytest

import ba_pathtracing_fur_amd as P
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import pathtracer as PT
from ba_pathtracing_fur_amd import scenes as S
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer, HipContext

import _reprojectref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
OUTPUTS = ("colour", "length", "variance", "motion")
SHAPES = {"colour": (3,), "length": (), "variance": (), "motion": (2,)}
TOLS = ("depth_tol", "normal_tol", "tangent_tol", "coverage_tol")
ALL_OFF = {t: 0.0 for t in TOLS}
POISON = np.uint32(0x7FC0DEAD).view(F32)        # a NaN no kernel produces
# more than one 64 x 4 block in each direction, ragged edges; and the smallest frame
SIZES = [(13, 9), (67, 35), (130, 3), (1, 1)]
COMBOS = [{}, dict(ALL_OFF), dict(max_history=4.0, samples=3.0),
          dict(depth_tol=0.1, normal_tol=0.3, tangent_tol=0.5, coverage_tol=0.6, match_object=True)] + \
         [dict(ALL_OFF, **{t: v}) for t, v in zip(TOLS, (0.05, 0.3, 0.5, 0.4))] + [dict(ALL_OFF, match_object=True)]


@functools.lru_cache(maxsize=None)
def cases(w, h):
    """[(name, cur, hist)]: every camera pair of _reprojectref.camera_pairs with seeded frames; read only."""
    res = []
    for k, (name, cc, hc) in enumerate(R.camera_pairs(S, w, h, 31 + w)):
        res.append((name, R.freeze(R.random_frame(w, h, cc, 500 + 7 * k + w, False)),
                    R.freeze(R.random_frame(w, h, hc, 600 + 7 * k + w, True))))
    return res


def differs(got, want):
    bad = R.bits(got) != R.bits(want)
    return f"{int(bad.sum())} values differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}" if bad.any() else ""


def to_device(ctx, frame):
    """The frame with every array as a DeviceBuffer, and the list of (buffer, host array) pairs."""
    pairs = []

    def up(a):
        b = DeviceBuffer.from_array(ctx, a)
        pairs.append((b, a))
        return b

    d = {"camera": frame["camera"], "colour": up(frame["colour"]), "aov": {ch: up(a) for ch, a in frame["aov"].items()}}
    for k in ("variance", "length"):
        if frame.get(k) is not None:
            d[k] = up(frame[k])
    return d, pairs


def read_back(res, w, h):
    return {k: b.to_array((h, w) + SHAPES[k], F32) for k, b in res.items()}


def device_call(ctx, w, h, cur, hist, out_init=None, in_place=False, **kw):
    """ctx.reproject on device buffers: the outputs read back, and whether every input is as it was."""
    dc, pc = to_device(ctx, cur)
    dh, ph = to_device(ctx, hist) if hist is not None else (None, [])
    out = None
    if out_init is not None:
        out = {k: DeviceBuffer.from_array(ctx, np.full((h, w) + SHAPES[k], out_init, F32)) for k in OUTPUTS}
    if in_place:
        out = {"colour": dc["colour"]}
    res = ctx.reproject(w, h, dc, dh, out=out, device=True, **kw)
    got = read_back(res, w, h)
    skip = {id(dc["colour"])} if in_place else set()
    untouched = all(b.to_array(a.shape, a.dtype).tobytes() == a.tobytes() for b, a in pc + ph if id(b) not in skip)
    for b, _a in pc + ph:
        b.free()
    for b in res.values():
        b.free()
    return got, untouched


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_restatement_and_the_host_entry(hip_ctx, w, h):
    """Host pointers and device pointers, every camera pair, the tests on and off."""
    for name, cur, hist in cases(w, h):
        for kw in COMBOS:
            ref, host = R.reproject(w, h, cur, hist, **kw), P.reproject_host(w, h, cur, hist, **kw)
            got = hip_ctx.reproject(w, h, cur, hist, **kw)
            for k in OUTPUTS:
                assert not differs(got[k], ref[k]), (name, kw, k, differs(got[k], ref[k]))
                assert not differs(got[k], host[k]), (name, kw, k)
        dev, untouched = device_call(hip_ctx, w, h, cur, hist)
        ref = R.reproject(w, h, cur, hist)
        assert untouched and all(not differs(dev[k], ref[k]) for k in OUTPUTS), name
    name, cur, hist = cases(w, h)[1]
    for c, hs in ((dict(cur, variance=None), hist), (cur, dict(hist, variance=None)), (cur, None)):
        ref, got = R.reproject(w, h, c, hs, samples=2.0), hip_ctx.reproject(w, h, c, hs, samples=2.0)
        dev, untouched = device_call(hip_ctx, w, h, c, hs, samples=2.0)
        for k in OUTPUTS:
            assert not differs(got[k], ref[k]) and not differs(dev[k], ref[k]) and untouched, k


def test_poisoned_outputs_in_place_and_outputs_left_out(hip_ctx):
    w, h = 67, 35
    name, cur, hist = cases(w, h)[5]
    want = R.reproject(w, h, cur, hist)
    poisoned = lambda a: (a.view(np.uint32) == np.uint32(0x7FC0DEAD)).any()
    # host pointers: poisoned outputs are fully overwritten, the inputs are untouched
    copy = lambda f: dict(f, colour=f["colour"].copy(), variance=f["variance"].copy(), aov={ch: a.copy() for ch, a in f["aov"].items()},
                          **({"length": f["length"].copy()} if "length" in f else {}))
    c0, h0 = copy(cur), copy(hist)
    out = {k: np.full((h, w) + SHAPES[k], POISON, F32) for k in OUTPUTS}
    got = hip_ctx.reproject(w, h, c0, h0, out=out)
    assert all(got[k] is out[k] and not differs(out[k], want[k]) and not poisoned(out[k]) for k in OUTPUTS)
    flat = lambda f: [f["colour"], f["variance"]] + ([f["length"]] if "length" in f else []) + [f["aov"][ch] for ch in sorted(f["aov"])]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flat(c0) + flat(h0), flat(cur) + flat(hist)))
    # device pointers: the same
    dev, untouched = device_call(hip_ctx, w, h, cur, hist, out_init=POISON)
    assert untouched and all(not differs(dev[k], want[k]) and not poisoned(dev[k]) for k in OUTPUTS)
    # out.colour == cur.colour, on the host and on the device
    buf = cur["colour"].copy()
    res = hip_ctx.reproject(w, h, dict(cur, colour=buf), hist, out={"colour": buf})
    assert res["colour"] is buf and not differs(buf, want["colour"])
    dev, untouched = device_call(hip_ctx, w, h, cur, hist, in_place=True)
    assert untouched and not differs(dev["colour"], want["colour"])
    # each output left out in turn does not change the others
    for k in OUTPUTS:
        rest = hip_ctx.reproject(w, h, cur, hist, out={k: None})
        assert k not in rest and all(not differs(rest[o], want[o]) for o in rest)
        alone = hip_ctx.reproject(w, h, cur, hist, out={o: None for o in OUTPUTS if o != k})
        assert list(alone) == [k] and not differs(alone[k], want[k])


def test_device_flag_refuses_host_pointers(hip_ctx):
    w, h = 13, 9
    name, cur, hist = cases(w, h)[2]
    dc, pc = to_device(hip_ctx, cur)
    dh, ph = to_device(hip_ctx, hist)
    err = lambda: hip_ctx.lib.khp_last_error().decode()
    host_plane = np.zeros((h, w, 3), F32)
    hp = host_plane.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def call(edit):
        p, cf, hf, o, res, keep = PT._reproject_args(hip_ctx, w, h, dc, dh, None, True, dict(normal_tol=0.3))
        edit(cf, hf, o)
        st = hip_ctx.lib.khp_reproject(hip_ctx.ptr, ctypes.byref(p), ctypes.byref(cf), ctypes.byref(hf), ctypes.byref(o))
        for b in res.values():
            b.free()
        return st

    assert call(lambda cf, hf, o: None) == N.KHP_OK, err()
    edits = [lambda cf, hf, o: setattr(cf, "colour", hp), lambda cf, hf, o: setattr(cf, "variance", hp),
             lambda cf, hf, o: setattr(cf.aov, "depth", hp), lambda cf, hf, o: setattr(cf.aov, "normal", hp),
             lambda cf, hf, o: setattr(hf, "colour", hp), lambda cf, hf, o: setattr(hf, "length", hp),
             lambda cf, hf, o: setattr(hf.aov, "coverage", hp), lambda cf, hf, o: setattr(hf.aov, "tangent", hp),
             lambda cf, hf, o: setattr(o, "colour", hp), lambda cf, hf, o: setattr(o, "motion", hp)]
    for e in edits:
        assert call(e) == N.KHP_EINVAL and "not device memory" in err(), err()
    # a plane whose test is off is not looked at: a host pointer there is no refusal
    p, cf, hf, o, res, keep = PT._reproject_args(hip_ctx, w, h, dc, dh, None, True, dict(ALL_OFF))
    cf.aov.normal = hp
    hf.aov.object = ctypes.cast(hp, ctypes.POINTER(ctypes.c_int32))
    assert hip_ctx.lib.khp_reproject(hip_ctx.ptr, ctypes.byref(p), ctypes.byref(cf), ctypes.byref(hf), ctypes.byref(o)) == N.KHP_OK
    for b in list(res.values()) + [b for b, _a in pc + ph]:
        b.free()


def test_sizes_in_a_row_regrow_the_staging_area():
    c = HipContext(0)                                           # a fresh context: its staging area starts empty
    try:
        for w, h in ((13, 9), (67, 35), (13, 9), (130, 3)):
            name, cur, hist = cases(w, h)[4]
            got, ref = c.reproject(w, h, cur, hist), R.reproject(w, h, cur, hist)
            assert all(not differs(got[k], ref[k]) for k in OUTPUTS), (w, h)
    finally:
        c.close()


# ---- the context is left alone ----------------------------------------------------------------------------------
CW, CH, DEPTH = 48, 32, 5


class Ctx:
    """A context with a built scene; closed on exit."""

    def __init__(self, sd):
        self.sd = sd

    def __enter__(self):
        self.c = HipContext(0)
        self.c.set_scene(self.sd)
        self.c.build_accel()
        return self.c

    def __exit__(self, *exc):
        self.c.close()


def raw_stats(c):
    s = N.Stats()
    N.check(c.lib, c.lib.khp_get_stats(c.ptr, ctypes.byref(s)), "khp_get_stats")
    return bytes(s)


def test_the_context_is_untouched():
    sd = S.config2(CW, CH, n_strands=200)
    name, cur, hist = cases(13, 9)[3]
    big = cases(67, 35)[3]

    def series(c, with_reproject):
        c.set_moments(True)
        frames = []
        for k in range(4):
            frames.append(c.render(CW, CH, 1, DEPTH, first_sample=k).copy())
            if with_reproject:
                fb, m, st = c.read_framebuffer(CW, CH), c.read_moments(CW, CH), raw_stats(c)
                c.reproject(13, 9, cur, hist)
                c.reproject(67, 35, big[1], big[2], match_object=True)
                c.reproject(13, 9, cur, None)
                assert raw_stats(c) == st                       # khp_stats, byte for byte
                assert c.read_framebuffer(CW, CH).tobytes() == fb.tobytes()
                after = c.read_moments(CW, CH)
                assert all(after[k2].tobytes() == m[k2].tobytes() for k2 in N.MOMENTS_PLANES)
        frames.append(c.read_framebuffer(CW, CH))
        m = c.read_moments(CW, CH)
        return frames + [m[k] for k in N.MOMENTS_PLANES], c.stats()["frames"]

    with Ctx(sd) as c:
        plain, n_plain = series(c, False)
    with Ctx(sd) as c:
        mixed, n_mixed = series(c, True)
    for k, (a, b) in enumerate(zip(plain, mixed)):
        assert a.tobytes() == b.tobytes(), f"frame or plane {k}"
    assert n_plain == n_mixed


# ---- end to end ---------------------------------------------------------------------------------------------------
def test_an_accumulator_on_device_buffers_across_a_camera_move():
    w, h, passes = 96, 64, 4
    sd = S.config2(w, h, n_strands=200)
    camA = sd.cam
    pos, _bl, ax, ay, ps = R.cam_arrays(camA)
    look = -np.cross(ax.astype(np.float64), ay.astype(np.float64))
    camB = S.camera(pos, look + 1.0 * float(ps) * ax + 0.4 * float(ps) * ay, (0.0, 1.0, 0.0), w, h)
    planes = ("normal", "tangent", "depth", "coverage", "object")
    with Ctx(sd) as c:
        c.set_moments(True)
        for k in range(passes):
            c.render(w, h, 1, DEPTH, first_sample=k)
        m = c.read_moments(w, h)
        nf = m["count"].astype(F32)
        with np.errstate(all="ignore"):
            varA = np.where(m["count"] >= 2, ((m["m2"][..., 0] + m["m2"][..., 1]) + m["m2"][..., 2]) / (nf * (nf - F32(1.0))),
                            F32(np.nan)).astype(F32)
        aovA = c.render_aov(w, h, passes)
        c.set_camera(camB)
        oneB = c.render(w, h, 1, DEPTH).copy()
        aovB = c.render_aov(w, h, 1)
        up = lambda a: DeviceBuffer.from_array(c, a)
        dA, dB = {ch: up(aovA[ch]) for ch in planes}, {ch: up(aovB[ch]) for ch in planes}
        acc = P.TemporalAccumulator(w, h, c)
        first = acc.push(camA, dA, up(m["mean"]), up(varA), samples=float(passes))
        assert not differs(read_back(first, w, h)["colour"], m["mean"])
        pushed = acc.push(camB, dB, up(oneB), samples=1.0)
        got = read_back(pushed, w, h)
        # the same chain through the host entry on the arrays read back
        hostA = {ch: aovA[ch] for ch in planes}
        h1 = P.reproject_host(w, h, {"camera": camA, "colour": m["mean"], "variance": varA, "aov": hostA}, None, samples=float(passes))
        h2 = P.reproject_host(w, h, {"camera": camB, "colour": oneB, "aov": {ch: aovB[ch] for ch in planes}},
                              {"camera": camA, "colour": h1["colour"], "length": h1["length"], "variance": h1["variance"], "aov": hostA})
        for k in OUTPUTS:
            assert not differs(got[k], h2[k]), (k, differs(got[k], h2[k]))
        surf = aovB["coverage"] > 0
        assert (got["length"][surf] > 1.0).mean() >= 0.5 and np.isfinite(got["motion"]).all()
        # the pushed frame and its variance go straight into the variance-guided filter
        guides = dict(dB, albedo=up(aovB["albedo"]))
        out = DeviceBuffer(c, 12 * w * h)
        c.denoise_var(w, h, guides, colour=pushed["colour"], variance=pushed["variance"], out=out, device=True)
        want = P.denoise_var_host(w, h, {ch: aovB[ch] for ch in planes[:4]}, got["colour"], variance=got["variance"])
        assert not differs(out.to_array((h, w, 3), F32), want)
