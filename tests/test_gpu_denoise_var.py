"""khp_denoise_var on the GPU: the kernels bit for bit against the numpy restatement
(tests/_denoisevarref.py) and against khp_denoise_var_host, the plumbing (host and device pointers,
in place, poisoned outputs, the scratch regrowing), the context's moments as the noise source, and
that rendering is left alone."""
import ctypes
import functools

import numpy as np
import pytest

import ba_pathtracing_fur_amd as P
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer, HipContext

import _denoisevarref as V

pytestmark = pytest.mark.gpu

F32 = np.float32
PLANES = ("normal", "albedo", "tangent", "depth", "coverage")
POISON = np.uint32(0x7FC0DEAD).view(F32)        # a NaN no kernel produces
# more than one 64 x 4 block in each direction, ragged edges; and the smallest frame
SIZES = [(13, 9), (67, 35), (130, 3), (1, 1)]
SOURCES = ("plane", "moments")


@functools.lru_cache(maxsize=None)
def case(w, h, source):
    """Seeded colours with bad pixels, the guide planes, and the noise as keyword arguments; read only."""
    c, g = V.random_case(w, h, 500 + w)
    nz = V.random_noise(w, h, 600 + w, source)
    for a in [c] + list(g.values()) + (list(nz.values()) if source == "moments" else [nz]):
        a.setflags(write=False)
    return c, g, ({"variance": nz} if source == "plane" else {"moments": nz})


@functools.lru_cache(maxsize=None)
def reference(w, h, source, iterations, prefilter):
    c, g, nz = case(w, h, source)
    ref = V.denoise_var(c, g, iterations=iterations, prefilter=prefilter, **nz)
    for a in ref:
        a.setflags(write=False)
    return ref


def differs(got, want):
    bad = V.bits(got) != V.bits(want)
    return f"{int(bad.sum())} values differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}" if bad.any() else ""


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("prefilter", [0, 1])
def test_device_equals_the_restatement_and_the_host_entry(hip_ctx, w, h, source, prefilter):
    c, g, nz = case(w, h, source)
    for it in (1, 3, 5, 8):
        got, got_v = hip_ctx.denoise_var(w, h, g, c, iterations=it, prefilter=prefilter, out_variance=True, **nz)
        ref, ref_v = reference(w, h, source, it, prefilter)
        assert not differs(got, ref), (it, differs(got, ref))
        assert not differs(got_v, ref_v), (it, differs(got_v, ref_v))
        host, host_v = P.denoise_var_host(w, h, g, c, iterations=it, prefilter=prefilter, out_variance=True, **nz)
        assert not differs(got, host) and not differs(got_v, host_v), it
        plain = hip_ctx.denoise_var(w, h, g, c, iterations=it, prefilter=prefilter, **nz)
        assert not differs(plain, got), it                       # the colour does not depend on out_variance
    if w * h > 1:
        assert not np.isfinite(c).all()


def test_terms_off_floor_zero_and_null_planes(hip_ctx):
    w, h = 67, 35
    c, g, nz = case(w, h, "plane")
    off = dict(sigma_color=0.0, sigma_normal=0.0, sigma_tangent=0.0, sigma_depth=0.0, sigma_coverage=0.0)
    for kw, planes in (({**off}, {}), ({**off, "sigma_color": 1.5, "clamp": 1.25, "floor": 0.0}, {}),
                       ({**off, "sigma_depth": 0.2}, {"depth": g["depth"], "coverage": g["coverage"]}),
                       ({**off, "sigma_color": 4.0, "sigma_tangent": 0.5, "sigma_coverage": 0.3, "prefilter": 0},
                        {"tangent": g["tangent"], "coverage": g["coverage"]}),
                       ({**off, "sigma_normal": 0.5}, {"normal": g["normal"], "coverage": g["coverage"]})):
        got, got_v = hip_ctx.denoise_var(w, h, planes, c, iterations=3, out_variance=True, **kw, **nz)
        ref, ref_v = V.denoise_var(c, planes, iterations=3, **kw, **nz)
        assert not differs(got, ref) and not differs(got_v, ref_v), kw
    # sigma_color == 0 is khp_denoise on the device too
    assert not differs(hip_ctx.denoise_var(w, h, g, c, sigma_color=0.0, **nz), hip_ctx.denoise(w, h, g, c, sigma_color=0.0))


def _device_call(ctx, w, h, c, g, nz, out_init, in_place=False, **kw):
    bufs = {ch: DeviceBuffer.from_array(ctx, g[ch]) for ch in PLANES}
    col = DeviceBuffer.from_array(ctx, c)
    if "variance" in nz:
        noise = {"variance": DeviceBuffer.from_array(ctx, nz["variance"])}
        planes = [(noise["variance"], nz["variance"])]
    else:
        m = {k: DeviceBuffer.from_array(ctx, nz["moments"][k]) for k in ("m2", "count")}
        noise = {"moments": m}
        planes = [(m[k], nz["moments"][k]) for k in ("m2", "count")]
    out = col if in_place else DeviceBuffer.from_array(ctx, out_init)
    outv = planes[0][0] if in_place and "variance" in nz else DeviceBuffer.from_array(ctx, np.full((h, w), POISON, F32))
    res = ctx.denoise_var(w, h, bufs, col, out=out, out_variance=outv, device=True, **noise, **kw)
    assert res[0] is out and res[1] is outv
    got, got_v = out.to_array((h, w, 3), F32), outv.to_array((h, w), F32)
    back = {ch: bufs[ch].to_array(g[ch].shape, F32) for ch in PLANES}
    col_back = col.to_array((h, w, 3), F32)
    noise_back = [b.to_array(a.shape, a.dtype) for b, a in planes]
    for b in list(bufs.values()) + [col, out, outv] + [b for b, _a in planes]:
        b.free()
    return got, got_v, back, col_back, noise_back


@pytest.mark.parametrize("source", SOURCES)
def test_device_pointers_in_place_and_poisoned_outputs(hip_ctx, source):
    w, h = 67, 35
    c, g, nz = case(w, h, source)
    want, want_v = reference(w, h, source, 5, 1)
    noise_arrays = [nz["variance"]] if source == "plane" else [nz["moments"]["m2"], nz["moments"]["count"]]
    poisoned = lambda a: (a.view(np.uint32) == np.uint32(0x7FC0DEAD)).any()
    # host pointers: poisoned outputs are fully overwritten, the inputs are untouched
    c0, g0 = c.copy(), {ch: a.copy() for ch, a in g.items()}
    nz0 = {"variance": nz["variance"].copy()} if source == "plane" else {"moments": {k: a.copy() for k, a in nz["moments"].items()}}
    out, out_v = hip_ctx.denoise_var(w, h, g0, c0, out=np.full((h, w, 3), POISON, F32),
                                     out_variance=np.full((h, w), POISON, F32), **nz0)
    assert not differs(out, want) and not differs(out_v, want_v) and not poisoned(out) and not poisoned(out_v)
    assert c0.tobytes() == c.tobytes() and all(g0[ch].tobytes() == g[ch].tobytes() for ch in g)
    kept = [nz0["variance"]] if source == "plane" else [nz0["moments"]["m2"], nz0["moments"]["count"]]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kept, noise_arrays))
    # in place on the host: out is colour (and out_variance is variance)
    buf = c.copy()
    if source == "plane":
        vbuf = nz["variance"].copy()
        res = hip_ctx.denoise_var(w, h, g, buf, variance=vbuf, out=buf, out_variance=vbuf)
        assert res[0] is buf and res[1] is vbuf and not differs(vbuf, want_v)
    else:
        assert hip_ctx.denoise_var(w, h, g, buf, out=buf, **nz) is buf
    assert not differs(buf, want)
    # device pointers: the same bits, the outputs overwritten, every input untouched
    got, got_v, back, col_back, noise_back = _device_call(hip_ctx, w, h, c, g, nz, np.full((h, w, 3), POISON, F32))
    assert not differs(got, want) and not differs(got_v, want_v) and not poisoned(got) and not poisoned(got_v)
    assert col_back.tobytes() == c.tobytes() and all(back[ch].tobytes() == g[ch].tobytes() for ch in PLANES)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(noise_back, noise_arrays))
    # in place on the device
    got, got_v, back, _col, _nb = _device_call(hip_ctx, w, h, c, g, nz, None, in_place=True)
    assert not differs(got, want) and not differs(got_v, want_v)
    assert all(back[ch].tobytes() == g[ch].tobytes() for ch in PLANES)


def test_device_flag_refuses_host_pointers(hip_ctx):
    w, h = 13, 9
    c, _g, nz = case(w, h, "plane")
    var = nz["variance"]
    buf = N.AovBuffers()
    p = N.DenoiseParams.defaults(width=w, height=h, flags=N.DENOISE_DEVICE, sigma_normal=0.0, sigma_tangent=0.0,
                                 sigma_depth=0.0, sigma_coverage=0.0)
    err = lambda: hip_ctx.lib.khp_last_error().decode()
    fptr = lambda a: ctypes.cast(a if isinstance(a, int) else a.ctypes.data, ctypes.POINTER(ctypes.c_float))
    d_c, d_v = DeviceBuffer.from_array(hip_ctx, c), DeviceBuffer.from_array(hip_ctx, var)
    d_out, d_outv = DeviceBuffer(hip_ctx, c.nbytes), DeviceBuffer(hip_ctx, var.nbytes)
    h_out, h_outv = np.zeros((h, w, 3), F32), np.zeros((h, w), F32)

    def call(colour, variance, out, outv):
        z = N.DenoiseNoise.defaults(variance=fptr(variance), out_variance=fptr(outv) if outv is not None else None)
        ptr = lambda a: ctypes.c_void_p(a if isinstance(a, int) else a.ctypes.data)
        return hip_ctx.lib.khp_denoise_var(hip_ctx.ptr, ctypes.byref(p), ptr(colour), ctypes.byref(buf), ctypes.byref(z), ptr(out))

    assert call(d_c.ptr, d_v.ptr, d_out.ptr, d_outv.ptr) == N.KHP_OK, err()
    for args in ((c, d_v.ptr, d_out.ptr, None), (d_c.ptr, var, d_out.ptr, None), (d_c.ptr, d_v.ptr, h_out, None),
                 (d_c.ptr, d_v.ptr, d_out.ptr, h_outv)):
        assert call(*args) == N.KHP_EINVAL and "not device memory" in err(), err()
    h_m2 = np.zeros((h, w, 3), F32)
    z = N.DenoiseNoise.defaults(source=N.NOISE_MOMENTS, m2=fptr(h_m2),
                                count=ctypes.cast(d_v.ptr, ctypes.POINTER(ctypes.c_uint32)))
    st = hip_ctx.lib.khp_denoise_var(hip_ctx.ptr, ctypes.byref(p), ctypes.c_void_p(d_c.ptr), ctypes.byref(buf),
                                     ctypes.byref(z), ctypes.c_void_p(d_out.ptr))
    assert st == N.KHP_EINVAL and "not device memory" in err()
    for b in (d_c, d_v, d_out, d_outv):
        b.free()


def test_sizes_in_a_row_regrow_the_scratch():
    c = HipContext(0)                                           # a fresh context: its scratch starts empty
    try:
        for w, h in ((13, 9), (67, 35), (13, 9), (130, 3)):
            for source in SOURCES:
                col, g, nz = case(w, h, source)
                got, got_v = c.denoise_var(w, h, g, col, iterations=3, out_variance=True, **nz)
                ref, ref_v = reference(w, h, source, 3, 1)
                assert not differs(got, ref) and not differs(got_v, ref_v), (w, h, source)
    finally:
        c.close()


# ---- the context's moments as the noise ---------------------------------------------------------------------
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


def test_context_source_reads_the_moments_in_place():
    sd = S.config2(CW, CH, n_strands=200)
    with Ctx(sd) as c:
        zeros = {ch: np.zeros((CH, CW) + N.AOV_CHANNELS[ch][0], F32) for ch in PLANES}
        with pytest.raises(N.KhpError) as e:                    # moments off
            c.denoise_var(CW, CH, zeros)
        assert e.value.status == N.KHP_ENOTREADY and "moments" in str(e.value)
        c.set_moments(True)
        with pytest.raises(N.KhpError) as e:                    # on, but nothing rendered
            c.denoise_var(CW, CH, zeros)
        assert e.value.status == N.KHP_ENOTREADY
        c.render(CW, CH, 4, DEPTH)
        c.render(CW, CH, 4, DEPTH, first_sample=4)
        aov = c.render_aov(CW, CH, 8)
        guides = {ch: aov[ch] for ch in PLANES}
        fb = c.read_framebuffer(CW, CH)
        m = c.read_moments(CW, CH)
        frames = c.stats()["frames"]
        assert (m["count"] >= 2).any() and np.isfinite(m["mean"]).all()
        for prefilter in (0, 1):
            got, got_v = c.denoise_var(CW, CH, guides, out_variance=True, prefilter=prefilter)
            want, want_v = c.denoise_var(CW, CH, guides, colour=m["mean"], moments=m, out_variance=True, prefilter=prefilter)
            assert not differs(got, want) and not differs(got_v, want_v), prefilter
            ref, ref_v = V.denoise_var(m["mean"], guides, moments=m, prefilter=prefilter)
            assert not differs(got, ref) and not differs(got_v, ref_v), prefilter
        # a caller's colour with the context's noise; the framebuffer with a caller's noise
        assert not differs(c.denoise_var(CW, CH, guides, colour=fb), V.denoise_var(fb, guides, moments=m)[0])
        assert not differs(c.denoise_var(CW, CH, guides, moments=m), V.denoise_var(fb, guides, moments=m)[0])
        # the device flag with the context as the source
        bufs = {ch: DeviceBuffer.from_array(c, guides[ch]) for ch in PLANES}
        out = DeviceBuffer(c, CW * CH * 12)
        c.denoise_var(CW, CH, bufs, out=out, device=True)
        assert not differs(out.to_array((CH, CW, 3), F32), V.denoise_var(m["mean"], guides, moments=m)[0])
        # nothing of the context was written
        assert c.read_framebuffer(CW, CH).tobytes() == fb.tobytes()
        after = c.read_moments(CW, CH)
        assert all(after[k].tobytes() == m[k].tobytes() for k in N.MOMENTS_PLANES)
        assert c.stats()["frames"] == frames
        with pytest.raises(N.KhpError) as e:                    # another size than the framebuffer's
            c.denoise_var(CW, CH - 1, {ch: np.ascontiguousarray(a[:-1]) for ch, a in guides.items()})
        assert e.value.status == N.KHP_EINVAL and "framebuffer" in str(e.value)
        for b in list(bufs.values()) + [out]:
            b.free()


def test_a_progressive_series_is_untouched():
    sd = S.config2(CW, CH, n_strands=200)
    gc, gg = V.random_case(CW, CH, 77)
    var = V.random_noise(CW, CH, 78)

    def series(c, with_denoise):
        c.set_moments(True)
        frames = []
        for k in range(4):
            frames.append(c.render(CW, CH, 1, DEPTH, first_sample=k).copy())
            if with_denoise:
                c.denoise_var(CW, CH, gg)                       # the moments' mean by the moments' noise
                c.denoise_var(CW, CH, gg, variance=var)         # the framebuffer by a caller's noise
                c.denoise_var(CW, CH, gg, gc, variance=var, iterations=2, out_variance=True)
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
