"""The per-pixel sample moments on the GPU: off by default and invisible when
off, the state bit for bit against khp_moments_fold_host over per-sample colours the feature
itself extracts (and those against the oracle), the same bits from every schedule, the invariant
against the framebuffer, tiles, khp_read_moments' plumbing, and the state's lifecycle."""
import ctypes
import functools

import numpy as np
import pytest

import ba_pathtracing_fur_amd as P
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S
from ba_pathtracing_fur_amd import sharding
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer, HipContext

import _momentsref as R

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W, H, DEPTH = 37, 23, 5            # 851 pixels: ragged against the 256-thread and the 128-pixel blocks
STATE = ("mean", "m2", "count", "bad")
POISON_F = np.uint32(0x7FC0DEAD).view(F32)        # a NaN no kernel produces
POISON_U = U32(0xDEADBEEF)


def scene(w, h):
    return S.config2(w, h, n_strands=200)


def defaults():
    prm = N.CtxParams()
    N.load_library().khp_ctx_params_defaults(ctypes.byref(prm))
    return prm.as_dict()


class Ctx:
    """One context of this module's own (the suite's shared one keeps its scene and parameters)."""
    ctx = None
    size = None

    @classmethod
    def get(cls, w=W, h=H, **params):
        """The context with the w x h scene, default parameters but `params`, moments off."""
        if cls.ctx is None:
            cls.ctx = HipContext(0)
        c = cls.ctx
        c.set_moments(False)
        if cls.size != (w, h):
            c.set_scene(scene(w, h))
            c.build_accel()
            cls.size = (w, h)
        c.set_params(**{**defaults(), **params})
        return c


@pytest.fixture(scope="module", autouse=True)
def _close_module_context():
    yield
    if Ctx.ctx is not None:
        Ctx.ctx.close()
        Ctx.ctx, Ctx.size = None, None


def raw(a):
    """The bits as they are (R.bits makes every NaN one pattern; a poison value must stay itself)."""
    return np.ascontiguousarray(a).view(U32)


def differs(got, want, planes=STATE):
    for ch in planes:
        a, b = R.bits(got[ch]), R.bits(want[ch])
        if a.shape != b.shape or not np.array_equal(a, b):
            bad = a != b
            return f"{ch}: {int(bad.sum())} values differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}"
    return ""


@functools.lru_cache(maxsize=None)
def extracted(w, h, n, seed=0x4B49524B):
    """Samples 0 .. n - 1 of every pixel as the feature itself reports them: the state zeroed (off,
    then on), one 1-spp call of sample k, mean read back.  (colours (n, h, w, 3), rejected (n, h, w));
    a rejected sample's colour is NaN here, as any non-finite value folds alike.  Read only."""
    c = Ctx.get(w, h)
    cols = np.zeros((n, h, w, 3), F32)
    rej = np.zeros((n, h, w), bool)
    for k in range(n):
        c.set_moments(False)
        c.set_moments(True)
        c.render(w, h, 1, DEPTH, seed=seed, first_sample=k, readback=False)
        m = c.read_moments(w, h)
        assert ((m["count"] + m["bad"]) == 1).all() and (m["count"] <= 1).all(), k
        assert (m["m2"] == 0).all() and np.isposinf(m["rel_error"]).all(), k
        assert np.isfinite(m["mean"]).all() and (m["mean"][m["bad"] == 1] == 0).all(), k
        cols[k] = m["mean"]
        rej[k] = m["bad"] == 1
    cols[rej] = np.nan
    c.set_moments(False)
    cols.setflags(write=False)
    rej.setflags(write=False)
    return cols, rej


@functools.lru_cache(maxsize=None)
def expected(w, h, n, seed=0x4B49524B):
    st = P.moments_fold_host(extracted(w, h, n, seed)[0])
    for a in st.values():
        a.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def oracle(w, h):
    import oracle_ffi
    return oracle_ffi.Oracle(scene(w, h))


# ---- 6. off by default --------------------------------------------------------------------------
@pytest.mark.parametrize("path_kernel", [0, 1])
def test_off_by_default_and_invisible_in_the_frame(path_kernel):
    c = Ctx.get(path_kernel=path_kernel)
    assert c.moments() is False
    with pytest.raises(N.KhpError, match="KHP_ENOTREADY"):
        c.read_moments(W, H)
    off = c.render(W, H, 5, DEPTH)
    off8 = c.read_rgba8(W, H)
    assert c.set_moments(True) is False and c.moments() is True
    assert c.set_moments(True) is True                       # the value it has: a no-op
    on = c.render(W, H, 5, DEPTH)
    on8 = c.read_rgba8(W, H)
    assert on.tobytes() == off.tobytes() and np.array_equal(on8, off8)
    m = c.read_moments(W, H)
    assert ((m["count"] + m["bad"]) == 5).all()
    assert c.set_moments(False) is True and c.moments() is False


# ---- 7. per-sample colours from the feature itself, and every schedule -----------------------
def test_extracted_colours_are_the_oracles():
    cols, rej = extracted(W, H, 6)
    o = oracle(W, H)
    for k in (0, 1, 3):                                      # k + 1 a power of two: col_k = (k + 1) f_k exactly
        f = o.render(W, H, 1, DEPTH, first_sample=k)         # col_k / (k + 1) on a zeroed buffer
        with np.errstate(all="ignore"):
            want = (F32(k + 1) * f).astype(F32)
        ok = ~rej[k]
        assert np.array_equal(R.bits(cols[k])[ok], R.bits(want)[ok]), k
        assert not np.isfinite(want[rej[k]]).all(-1).any(), k


def _one_call(c, n):
    c.render(W, H, n, DEPTH, readback=False)


def _calls(c, *spps):
    k = 0
    for s in spps:
        c.render(W, H, s, DEPTH, first_sample=k, readback=False)
        k += s


def _async_passes(c, n):
    for k in range(n):
        c.render(W, H, 1, DEPTH, first_sample=k, async_=True)
    c.sync()


SCHEDULES = {
    "one call": ({}, lambda c: _one_call(c, 6)),
    "six 1-spp calls": ({}, lambda c: _calls(c, 1, 1, 1, 1, 1, 1)),
    "six 1-spp calls, no render-ahead": ({"render_ahead": 0}, lambda c: _calls(c, 1, 1, 1, 1, 1, 1)),
    "2 + 4": ({}, lambda c: _calls(c, 2, 4)),
    "six fused asynchronous passes": ({}, lambda c: _async_passes(c, 6)),
    "asynchronous passes, not fused": ({"fuse_frames": 1}, lambda c: _async_passes(c, 6)),
    "two batches in flight": ({"frames_in_flight": 2, "fuse_frames": 2}, lambda c: _async_passes(c, 6)),
    "path kernel": ({"path_kernel": 1, "render_ahead": 0}, lambda c: _calls(c, 1, 1, 1, 1, 1, 1)),
    "path kernel, render-ahead 3": ({"path_kernel": 1, "render_ahead": 3}, lambda c: _calls(c, 1, 1, 1, 1, 1, 1)),
    "path kernel, one call": ({"path_kernel": 1}, lambda c: _one_call(c, 6)),
    # 851 pixels x 6 samples against 4096 paths a chunk: one call is cut into samples 0-3 and 4-5,
    # six fused passes into pixel chunks of 4096 / 6 = 682 at most
    "sample chunks": ({"chunk_paths": 4096}, lambda c: _one_call(c, 6)),
    "pixel chunks": ({"chunk_paths": 4096}, lambda c: _async_passes(c, 6)),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_every_schedule_gives_the_host_folds_bits(name):
    want = expected(W, H, 6)
    params, run = SCHEDULES[name]
    c = Ctx.get(**params)
    c.set_moments(True)
    run(c)
    got = c.read_moments(W, H)
    assert not differs(got, want), differs(got, want)
    assert R.same(got["rel_error"], want["rel_error"]) and R.same(got["rel_error"], R.rel_error(got))
    assert (got["bad"] > 0).any() and (got["bad"] == extracted(W, H, 6)[1].sum(0)).all()
    c.set_moments(False)


def test_seventeen_samples_take_the_per_frame_kernel():
    """spp = 17 is above ACC_MAX_SAMPLES = 16: k_accumulate_m instead of k_accumulate_all_m."""
    want = expected(W, H, 17)
    c = Ctx.get()
    c.set_moments(True)
    c.render(W, H, 17, DEPTH, readback=False)
    got = c.read_moments(W, H)
    assert not differs(got, want), differs(got, want)
    assert ((got["count"] + got["bad"]) == 17).all()
    c.set_moments(False)


def test_one_pixel_frame():
    want = expected(1, 1, 33)
    c = Ctx.get(1, 1)
    c.set_moments(True)
    c.render(1, 1, 33, DEPTH, readback=False)
    got = c.read_moments(1, 1)
    assert not differs(got, want, STATE + ("rel_error",)), differs(got, want, STATE + ("rel_error",))
    assert got["count"][0, 0] + got["bad"][0, 0] == 33
    c.set_moments(False)


# ---- 8. the invariant ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mean_is_the_framebuffer_where_nothing_was_rejected(seed):
    c = Ctx.get()
    c.set_moments(True)
    c.render(W, H, 17, DEPTH, seed=seed, readback=False)
    fb = c.read_framebuffer(W, H)
    m = c.read_moments(W, H)
    c.set_moments(False)
    good = m["bad"] == 0
    assert (~good).any()                                     # the oracle's frames have 18, 21 and 9 such pixels
    assert np.array_equal(R.bits(m["mean"])[good], R.bits(fb)[good])
    assert np.array_equal(np.isfinite(fb).all(-1), good)     # the framebuffer is lost exactly where bad > 0
    assert np.isfinite(m["mean"]).all()
    assert ((m["count"] + m["bad"]) == 17).all()


# ---- 9. tiles -----------------------------------------------------------------------------------
def test_tile_ranks_fold_only_their_pixels():
    c = Ctx.get()
    c.set_moments(True)
    c.render(W, H, 6, DEPTH, readback=False)
    whole = c.read_moments(W, H)
    c.set_moments(False)
    assert not differs(whole, expected(W, H, 6))
    sd = scene(W, H)
    seen = np.zeros((H, W), int)
    for rank in range(3):
        r = HipContext(0)
        try:
            r.set_scene(sd)
            r.build_accel()
            r.set_moments(True)
            r.render(W, H, 6, DEPTH, tile_size=8, tile_rank=rank, tile_nranks=3, readback=False)
            got = r.read_moments(W, H)
        finally:
            r.close()
        own = sharding.owned_mask(W, H, rank, 3, tile=8)
        assert own.any() and not own.all()
        seen += own
        for ch in STATE:
            assert np.array_equal(R.bits(got[ch])[own], R.bits(whole[ch])[own]), (rank, ch)
            assert (R.bits(got[ch])[~own] == 0).all(), (rank, ch)
        assert np.isposinf(got["rel_error"][~own]).all()
    assert (seen == 1).all()


# ---- 10. read -----------------------------------------------------------------------------------
def _poisoned(w, h):
    return {ch: np.full((h, w) + tail, POISON_F if dt == F32 else POISON_U, dt) for ch, (tail, dt) in N.MOMENTS_PLANES.items()}


def _rendered(w, h, spp=6):
    c = Ctx.get(w, h)
    c.set_moments(True)
    c.render(w, h, spp, DEPTH, readback=False)
    return c


@pytest.mark.parametrize("w,h", [(W, H), (130, 3)])          # 130 x 3: more than one 256-lane block
def test_read_into_host_and_device_buffers(w, h):
    c = _rendered(w, h)
    host = c.read_moments(w, h, out=_poisoned(w, h))
    for ch, a in host.items():
        assert not (raw(a) == raw(_poisoned(w, h)[ch])).any(), ch          # fully overwritten
    assert ((host["count"] + host["bad"]) == 6).all()
    assert R.same(host["rel_error"], R.rel_error(host))
    assert np.isfinite(host["rel_error"]).any()
    bufs = {ch: DeviceBuffer.from_array(c, a) for ch, a in _poisoned(w, h).items()}
    dev = c.read_moments(w, h, device=True, out=bufs)
    for ch, (tail, dt) in N.MOMENTS_PLANES.items():
        assert dev[ch] is bufs[ch]
        assert R.same(bufs[ch].to_array((h, w) + tail, dt), host[ch]), ch
    # NULL planes are skipped: the others of the same buffers stay as they were
    for only in (("count",), ("rel_error", "m2"), ("mean",)):
        part = c.read_moments(w, h, planes=only)
        assert tuple(part) == only
        for ch in only:
            assert R.same(part[ch], host[ch]), only
        skip = {ch: DeviceBuffer.from_array(c, a) for ch, a in _poisoned(w, h).items()}
        c.read_moments(w, h, device=True, planes=only, out=skip)
        for ch, (tail, dt) in N.MOMENTS_PLANES.items():
            want = host[ch] if ch in only else _poisoned(w, h)[ch]
            assert np.array_equal(raw(skip[ch].to_array((h, w) + tail, dt)), raw(want)), (only, ch)
        for b in skip.values():
            b.free()
    for b in bufs.values():
        b.free()
    c.set_moments(False)


def test_read_refusals():
    c = _rendered(W, H)
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    host = np.zeros((H, W), U32)
    b = N.MomentsBuffers()
    assert lib.khp_read_moments(c.ptr, 0, ctypes.byref(b)) == N.KHP_EINVAL and "every plane" in err()
    assert lib.khp_read_moments(c.ptr, 0, None) == N.KHP_EINVAL and "null" in err()
    b.count = host.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert lib.khp_read_moments(c.ptr, 2, ctypes.byref(b)) == N.KHP_EINVAL and "flag" in err()
    assert lib.khp_read_moments(c.ptr, 0, ctypes.byref(b)) == N.KHP_OK
    # a host pointer with KHP_MOMENTS_DEVICE is refused, not handed to a kernel
    assert lib.khp_read_moments(c.ptr, N.MOMENTS_DEVICE, ctypes.byref(b)) == N.KHP_EINVAL and "not device memory" in err()
    for m in (N.Moments(2), N.Moments(1, (0, 1, 0)), N.Moments(0, (0, 0, 7))):
        assert lib.khp_set_moments(c.ptr, ctypes.byref(m)) == N.KHP_EINVAL, (m.enabled, list(m.reserved))
    assert lib.khp_set_moments(c.ptr, None) == N.KHP_EINVAL and "null" in err()
    assert lib.khp_get_moments(c.ptr, None) == N.KHP_EINVAL and "null" in err()
    assert c.moments() is True                               # the refused calls changed nothing
    c.set_moments(False)


def test_reading_changes_nothing_of_a_progressive_series():
    frames = {}
    for read in (False, True):
        c = Ctx.get()
        c.set_moments(True)
        out = []
        for k in range(5):
            out.append(c.render(W, H, 1, DEPTH, first_sample=k).copy())
            if read:
                c.read_moments(W, H)
                c.read_moments(W, H, planes=("rel_error",))
        out.append(c.read_framebuffer(W, H))
        out.append(c.read_rgba8(W, H))
        st = c.read_moments(W, H)
        frames[read] = (out, st)
        c.set_moments(False)
    for a, b in zip(frames[False][0], frames[True][0]):
        assert a.tobytes() == b.tobytes()
    assert not differs(frames[True][1], frames[False][1], STATE + ("rel_error",))
    want = P.moments_fold_host(extracted(W, H, 6)[0][:5])
    assert not differs(frames[True][1], want), differs(frames[True][1], want)


# ---- 11. lifecycle ------------------------------------------------------------------------------
def test_lifecycle():
    c = HipContext(0)
    try:
        c.set_scene(scene(W, H))
        c.build_accel()
        c.set_moments(True)                                  # before any framebuffer: made with the first render
        with pytest.raises(N.KhpError, match="KHP_ENOTREADY"):
            c.read_moments(W, H)
        c.render(W, H, 6, DEPTH, readback=False)
        assert not differs(c.read_moments(W, H), expected(W, H, 6))
        # a call with first_sample = 0 restarts it
        c.render(W, H, 6, DEPTH, readback=False)
        assert not differs(c.read_moments(W, H), expected(W, H, 6))
        # a size change re-makes a zeroed state, there and back
        c.set_scene(scene(W - 5, H + 2))
        c.build_accel()
        c.render(W - 5, H + 2, 1, DEPTH, first_sample=3, readback=False)
        m = c.read_moments(W - 5, H + 2)
        assert m["count"].shape == (H + 2, W - 5) and ((m["count"] + m["bad"]) == 1).all() and (m["m2"] == 0).all()
        c.set_scene(scene(W, H))
        c.build_accel()
        c.render(W, H, 2, DEPTH, first_sample=4, readback=False)
        m = c.read_moments(W, H)
        want = P.moments_fold_host(extracted(W, H, 6)[0][4:6], first_sample=4)
        assert not differs(m, want), differs(m, want)
        # disabling and then reading
        c.set_moments(False)
        with pytest.raises(N.KhpError, match="KHP_ENOTREADY"):
            c.read_moments(W, H)
        # enabling in mid-series counts only the samples folded since; the framebuffer is there, so
        # the state is made at once and reads as zeros
        c.render(W, H, 2, DEPTH, readback=False)
        c.set_moments(True)
        m = c.read_moments(W, H)
        assert all((R.bits(m[ch]) == 0).all() for ch in STATE) and np.isposinf(m["rel_error"]).all()
        c.render(W, H, 4, DEPTH, first_sample=2, readback=False)
        m = c.read_moments(W, H)
        want = P.moments_fold_host(extracted(W, H, 6)[0][2:6], first_sample=2)
        assert not differs(m, want), differs(m, want)
        fb = c.read_framebuffer(W, H)
        c.set_moments(False)
        c.render(W, H, 6, DEPTH, readback=False)             # the framebuffer went on as without it
        assert c.read_framebuffer(W, H).tobytes() == fb.tobytes()
        c.set_moments(True)
    finally:
        c.close()                                            # frees the state with the context
