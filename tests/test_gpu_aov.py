"""khp_render_aov on the GPU: every channel bit for bit against the numpy restatement
(tests/_aovref.py: restated camera rays, khp_debug_surface / khp_debug_light_isect per sample,
the ordered float32 sum), the call's schedule and plumbing (chunks, device buffers, channel
subsets, tile ranks, a moved camera, renderer settings), that rendering is left untouched, and
that the restated camera rays are the renderer's own."""
import ctypes

import numpy as np
import pytest

from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S
from ba_pathtracing_fur_amd.pathtracer import DeviceBuffer, HipContext

import _aovref as A

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 32, 24
SEEDS = (0x4B49524B, 20260117)
POISON_F = np.uint32(0x7FC0DEAD).view(F32)      # a NaN no kernel produces
POISON_I = np.int32(-12345)


class Ctx:
    """A context with a built scene; closed on exit."""

    def __init__(self, sd, **params):
        self.sd, self.params = sd, params

    def __enter__(self):
        self.c = HipContext(0)
        self.c.set_scene(self.sd)
        self.c.build_accel()
        if self.params:
            self.c.set_params(**self.params)
        return self.c

    def __exit__(self, *exc):
        self.c.close()


def poisoned(width=W, height=H, channels=A.CHANNELS):
    return {ch: np.full((height, width) + N.AOV_CHANNELS[ch][0], POISON_I if ch == "object" else POISON_F,
                        N.AOV_CHANNELS[ch][1]) for ch in channels}


def untouched(a):
    return (a.view(np.uint32) == (np.uint32(0x7FC0DEAD) if a.dtype == F32 else POISON_I.view(np.uint32))).all()


def check(got, want, what=""):
    for ch in A.CHANNELS:
        if ch in got:
            bad = A.bits(got[ch]) != A.bits(want[ch])
            assert not bad.any(), f"{what}: channel {ch} differs in {int(bad.sum())} values, first at " \
                                  f"{tuple(int(i) for i in np.argwhere(bad)[0])}"


# ---- scenes ---------------------------------------------------------------------------------------------
def hairball_scene():
    return S.config2(W, H, n_strands=20)


def fibre_triangle_scene():
    sd = S.SceneData(name="cornell_fibre_tubes")
    S.cornell_box(sd, W, H)
    pos, rad = S.hairball(12, (0.0, 0.5, 0.0), 0.25, root_radius=0.02)
    sd.add_fibers(pos, rad, sd.add_material(S.fiber_material()), as_triangles=True, resolution=3)
    return sd


FLOOR_RGB, FUR_RGB = (200, 120, 40), (255, 0, 0)


def constant_texture_scene():
    """One-colour textures: the TEX instances run, and the albedo is texel / 255 wherever the hit is.  The fur's
    colour is Texture::getColor's answer for a NaN coordinate too (Color::RED), so a degenerate cone texcoord
    changes nothing."""
    sd = S.SceneData(name="constant_textures")
    floor = sd.add_material(S.material(diffuse=(0.5, 0.5, 0.5)))
    fur = sd.add_material(S.fiber_material())
    plain = sd.add_material(S.material(diffuse=(0.1, 0.7, 0.3)))
    sd.set_material_texture(floor, "diffuse", sd.add_texture(np.full((4, 6, 3), FLOOR_RGB, np.uint8)))
    sd.set_material_texture(fur, "diffuse", sd.add_texture(np.full((8, 8, 3), FUR_RGB, np.uint8)))
    v, n = S.quad((-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4), (0, 1, 0))
    sd.add_triangles(v, n, floor, uv=F32([[[-1.5, -1.5], [-1.5, 2.5], [2.5, 2.5]], [[-1.5, -1.5], [2.5, 2.5], [2.5, -1.5]]]))
    v, n = S.quad((0.6, 0.0, -1.4), (1.8, 0.0, -1.4), (1.8, 1.4, -1.4), (0.6, 1.4, -1.4), (0, 0, 1))
    sd.add_triangles(v, n, plain)
    pos, rad = S.hairball(40, (-0.3, 0.45, 0.2), 0.3, root_radius=0.02)
    sd.add_fibers(pos, rad, fur)
    sd.lights.append(S.quad_light((0.0, 2.8, 0.0), (0.0, -1.0, 0.0), (1.2, 1.2), (4.0, 4.0, 4.0), att_const=1.0))
    sd.cam = S.camera((0.0, 1.3, 3.4), (0.0, -0.25, -1.0), (0.0, 1.0, 0.0), W, H)
    return sd


def one_cone_scene(look=(0.0, 0.0, -1.0)):
    """tests/test_gpu_hair_lobes.py's cone, with the point light's sphere between the camera and the cone."""
    sd = S.SceneData(name="one_cone_light_in_view")
    sd.add_cones(F32([[-1.0, 0.0, 0.0, 0.2]]), F32([[1.0, 0.02, 0.0, 0.2]]), sd.add_material(S.fiber_material()))
    sd.lights.append(S.point_light((0.12, 0.08, 0.8), (5.0, 5.0, 5.0), radius=0.1))
    sd.cam = S.camera((0.0, 0.05, 1.5), look, width=W, height=H)
    return sd


# ---- 1. bit for bit against the restatement ------------------------------------------------------------
@pytest.fixture(scope="module")
def hairball():
    sd = hairball_scene()
    with Ctx(sd) as c:
        yield c, sd


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("first", [0, 7])
def test_hairball_matches_the_restatement(hairball, seed, first):
    c, sd = hairball
    for spp in (1, 3, 4, 5):
        want = A.reference(c, sd, W, H, spp, seed, first)
        got = c.render_aov(W, H, spp, seed=seed, first_sample=first)
        check(got, want, f"spp {spp}")
        cov = got["coverage"]
        # the box's opening, 1.35 away, spans 0.5 / 0.94 x 0.5 / 0.70 = 0.38 of the view (half-tangents 0.69 x 0.52)
        assert cov.min() >= 0.0 and cov.max() == 1.0 and 0.3 < (cov > 0).mean() < 0.45
        assert (got["object"] >= 0).any() and got["object"].max() < sd.n_objects
    # fur pixels carry a tangent, box pixels none (zero frames on plain triangles)
    # (20 strands of radius 0.004 cover about 4 pixels' worth of the frame: ~19 of 768 pixels at 5 spp)
    tangent = np.abs(got["tangent"]).sum(-1) > 0
    assert tangent.any() and not tangent.all()
    fur = got["object"] >= len(sd.tri_v)
    assert tangent[fur].all()


def _scene_case(sd, spp=3, seed=SEEDS[1], first=2):
    with Ctx(sd) as c:
        want = A.reference(c, sd, W, H, spp, seed, first)
        got = c.render_aov(W, H, spp, seed=seed, first_sample=first)
        check(got, want, sd.name)
    return got, want


def test_transformed_cones_match():
    got, _ = _scene_case(S.transformed_hairball(W, H, n_strands=120))
    assert (got["coverage"] > 0).any()


def test_fibre_triangles_match():
    sd = fibre_triangle_scene()
    got, _ = _scene_case(sd)
    tube = (got["object"] >= 10) & (got["coverage"] == 1.0)        # objects 0..9: the box's triangles
    assert tube.any() and (np.abs(got["tangent"][tube]).sum(-1) > 0).all()   # the fibre's frame rides on its triangles


def test_constant_textures_match_and_give_the_known_albedo():
    sd = constant_texture_scene()
    got, _ = _scene_case(sd, spp=1)
    full = got["coverage"] == 1.0
    obj = got["object"]
    floor, fur = full & (obj >= 0) & (obj < 2), full & (obj >= 4)
    assert floor.any() and fur.any()
    assert np.array_equal(got["albedo"][floor], np.tile(F32(FLOOR_RGB) / F32(255.0), (int(floor.sum()), 1)))
    assert np.array_equal(got["albedo"][fur], np.tile(F32([1.0, 0.0, 0.0]), (int(fur.sum()), 1)))
    plain = full & ((obj == 2) | (obj == 3))                       # an untextured material in a textured scene
    assert plain.any() and np.array_equal(got["albedo"][plain], np.tile(F32([0.1, 0.7, 0.3]), (int(plain.sum()), 1)))


def test_albedo_of_real_textures_is_the_material_query():
    """Textures whose texel depends on the hit (test_texture_truth's hit scene: every channel count, the
    pow wrap, uv beyond [0, 1], fibres in world space and under a node transform): the albedo of a sample
    is khp_debug_material's resolved diffuse for the restated camera ray -- the query test_texture_truth
    pins to a float64 truth -- and a pixel's albedo the ordered float32 mean of its samples'."""
    from test_texture_truth import hit_scene
    sd = hit_scene(W, H)
    npix = W * H
    with Ctx(sd) as c:
        for spp, first in ((1, 0), (3, 2)):
            pixels = np.repeat(np.arange(npix, dtype=np.uint64), spp)
            samples = np.tile(np.arange(first, first + spp, dtype=np.uint64), npix)
            o, raw, _ = A.camera_rays(sd.cam, W, pixels, SEEDS[1], samples)
            q = c.debug_material(o, raw)
            rec = A.sample_records(c, sd, o, raw, albedo=q["diffuse"])
            assert np.array_equal(rec["object"], np.where(rec["coverage"] == 1, q["obj"], -1))
            want = {ch: a.reshape((H, W) + a.shape[1:]) for ch, a in A.reduce_records(rec, npix, spp).items()}
            got = c.render_aov(W, H, spp, seed=SEEDS[1], first_sample=first)
            check(got, want, f"spp {spp}")
            if spp == 1:        # wherever the one sample is a surface sample: the query's own answers, bit for bit
                full = got["coverage"].reshape(-1) == 1.0
                assert full.mean() > 0.5
                assert np.array_equal(A.bits(got["albedo"].reshape(-1, 3)[full]), A.bits(q["diffuse"][full]))
                assert np.array_equal(got["object"].reshape(-1)[full], q["obj"][full])
                assert np.array_equal(A.bits(got["depth"].reshape(-1)[full]), A.bits(q["t"][full]))
                # and the texel does depend on the hit: the floor alone shows many colours
                floor = full & (q["obj"] >= 0) & (q["obj"] < 2)
                assert len(np.unique(got["albedo"].reshape(-1, 3)[floor], axis=0)) > 8


def test_samples_that_end_on_a_light_are_not_surface_samples():
    sd = one_cone_scene()
    got, want = _scene_case(sd, spp=4)
    assert want["light_ended"] > 0                                  # the light's sphere hides part of the cone
    assert 0.0 < got["coverage"].mean() < 1.0
    part = (got["coverage"] > 0) & (got["coverage"] < 1)
    assert part.any()                                               # premultiplied: a host divides by coverage
    n = got["normal"][part] / got["coverage"][part][:, None]
    assert np.isfinite(n).all()


def test_a_camera_that_sees_nothing_gives_zeros():
    sd = one_cone_scene(look=(0.0, 0.0, 1.0))
    with Ctx(sd) as c:
        got = c.render_aov(W, H, 3, out=poisoned())
    for ch in A.FLOAT_CHANNELS:
        assert not got[ch].view(np.uint32).any(), ch                # +0, not -0, and no poison left
    assert (got["object"] == -1).all()


# ---- 2. schedule and plumbing ---------------------------------------------------------------------------
def test_many_chunks_equal_one():
    sd = S.config2(96, 64, n_strands=20)
    with Ctx(sd) as c:
        one = c.render_aov(96, 64, 3, seed=SEEDS[1])
        c.set_params(chunk_paths=4096)                              # 96 x 64 x 3 = 18,432 paths: 5 chunks of 1,365 pixels
        many = c.render_aov(96, 64, 3, seed=SEEDS[1])
        check(many, one, "chunk_paths 4096")
        want = A.reference(c, sd, 96, 64, 3, SEEDS[1])
        check(many, want, "96x64 against the restatement")


def _device_call(c, width, height, spp, seed, channels, init, first=0, **tile):
    """khp_render_aov with KHP_RENDER_OUT_DEVICE into device copies of `init`, read back with khp_device_copy."""
    bufs = {ch: DeviceBuffer.from_array(c, init[ch]) for ch in channels}
    ab = N.AovBuffers()
    for ch, b in bufs.items():
        setattr(ab, ch, ctypes.cast(b.ptr, ctypes.POINTER(ctypes.c_int32 if ch == "object" else ctypes.c_float)))
    p = N.RenderParams(width, height, spp, 0, seed, first, tile.get("tile_size", 64), tile.get("tile_rank", 0),
                       tile.get("tile_nranks", 1), N.RENDER_OUT_DEVICE)
    N.check(c.lib, c.lib.khp_render_aov(c.ptr, ctypes.byref(p), ctypes.byref(ab)), "khp_render_aov")
    out = {ch: b.to_array(init[ch].shape, init[ch].dtype) for ch, b in bufs.items()}
    for b in bufs.values():
        b.free()
    return out


def test_device_buffers_equal_host_buffers(hairball):
    c, _ = hairball
    host = c.render_aov(W, H, 3, seed=SEEDS[0])
    dev = _device_call(c, W, H, 3, SEEDS[0], A.CHANNELS, poisoned())
    check(dev, host, "device buffers")
    # a host pointer with the device flag is refused, not written by a kernel
    ab, keep = N.AovBuffers(), np.zeros((H, W), F32)
    ab.depth = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    p = N.RenderParams(W, H, 1, 0, 1, 0, 0, 0, 1, N.RENDER_OUT_DEVICE)
    assert c.lib.khp_render_aov(c.ptr, ctypes.byref(p), ctypes.byref(ab)) == N.KHP_EINVAL
    assert "device" in c.lib.khp_last_error().decode()


@pytest.mark.parametrize("subset", [("depth",), ("object",), ("albedo", "coverage"), ("tangent", "normal", "object")])
def test_channel_subsets(hairball, subset):
    c, _ = hairball
    full = c.render_aov(W, H, 4, seed=SEEDS[0], first_sample=1)
    bufs = poisoned()
    got = c.render_aov(W, H, 4, seed=SEEDS[0], first_sample=1, channels=subset, out=bufs)
    assert set(got) == set(subset) and all(got[ch] is bufs[ch] for ch in subset)
    check(got, full, f"subset {subset}")
    for ch in A.CHANNELS:                                           # buffers not asked for are never written
        assert ch in subset or untouched(bufs[ch]), ch
    dev = _device_call(c, W, H, 4, SEEDS[0], subset, poisoned(), first=1)    # the same with device pointers, the others NULL
    check({ch: dev[ch] for ch in subset}, full, f"device subset {subset}")


def test_tile_ranks_partition_the_frame(hairball):
    c, _ = hairball
    T, R = 8, 3
    full = c.render_aov(W, H, 3, seed=SEEDS[1])
    owned = {}
    for r in (1, 2):                                                # a sender's plan lists the pixels it renders
        counts, pix = N.gather_plan(W, H, T, R, r, 0)
        assert counts[r] == len(pix)
        owned[r] = np.zeros(W * H, bool)
        owned[r][pix] = True
    owned[0] = ~(owned[1] | owned[2])
    assert not (owned[1] & owned[2]).any() and all(o.any() for o in owned.values())
    for r in range(R):
        host = c.render_aov(W, H, 3, seed=SEEDS[1], tile_size=T, tile_rank=r, tile_nranks=R, out=poisoned())
        dev = _device_call(c, W, H, 3, SEEDS[1], A.CHANNELS, poisoned(), tile_size=T, tile_rank=r, tile_nranks=R)
        m = owned[r].reshape(H, W)
        for name, got in (("host", host), ("device", dev)):
            for ch in A.CHANNELS:
                assert np.array_equal(A.bits(got[ch][m]), A.bits(full[ch][m])), (name, r, ch)
                assert untouched(got[ch][~m]), (name, r, ch)


def test_a_moved_camera_is_honoured():
    sd = hairball_scene()
    moved = S.camera((0.3, 0.6, 1.7), (-0.15, -0.05, -1.0), (0.0, 1.0, 0.0), W, H)
    with Ctx(sd) as c:
        before = c.render_aov(W, H, 2)
        c.set_camera(moved)
        got = c.render_aov(W, H, 2)
        want = A.reference(c, sd, W, H, 2, 0x4B49524B, cam=moved)
        check(got, want, "after khp_set_camera")
    assert not A.same(before["depth"], got["depth"])
    sd2 = hairball_scene()
    sd2.cam = moved
    with Ctx(sd2) as c2:
        check(c2.render_aov(W, H, 2), got, "a scene rebuilt with the moved camera")


def test_renderer_settings_change_nothing(hairball):
    c, _ = hairball
    base = c.render_aov(W, H, 3, seed=SEEDS[1])
    try:
        c.set_hair_lobes(N.HAIR_LOBE_R | N.HAIR_LOBE_TT | N.HAIR_LOBE_TRT)
        check(c.render_aov(W, H, 3, seed=SEEDS[1]), base, "hair lobes")
        c.set_hair_lobes(N.HAIR_LOBE_R)
        c.set_bdpt(enabled=1, light_paths=4, vertices=2)
        check(c.render_aov(W, H, 3, seed=SEEDS[1]), base, "light-path variant")
        c.set_bdpt(enabled=0)
        for kw in ({"path_kernel": 1}, {"path_kernel": 2}, {"wide_from": 0}, {"wide_from": 1, "lds_nodes": 7}):
            old = c.set_params(**kw)
            check(c.render_aov(W, H, 3, seed=SEEDS[1]), base, str(kw))
            c.set_params(**{k: old[k] for k in kw})
    finally:
        c.set_hair_lobes(N.HAIR_LOBE_R)
        c.set_bdpt(enabled=0)


# ---- 3. rendering is untouched ----------------------------------------------------------------------------
RW, RH, DEPTH = 48, 32, 4


def _sync_series(c, spp, with_aov):
    frames, stats = [], []
    for k in range(4):
        if with_aov:
            c.render_aov(RW, RH, 2, seed=SEEDS[1], first_sample=k)
        frames.append(c.render(RW, RH, spp, DEPTH, first_sample=k * spp).copy())
        st = c.stats()
        print(f"call {k}: frames {st['frames']}, ahead_resumed {st['ahead_resumed']}, ahead_finished "
              f"{st['ahead_finished']}" + (" (with AOV calls)" if with_aov else ""))
        # How the work done ahead splits into paths already finished and paths resumed from a park record
        # is decided by which lanes were mid-path when the earlier launch ended: it moves with the clock
        # from run to run of the same series (three runs of this 1-spp series on one MI355X, no AOV call
        # anywhere: 4 / 18 / 0, 1 / 0 / 0 and 13 / 0 / 0 paths resumed by calls 1-3, of 1,536).  Their sum is
        # what the call found done ahead; it is 0 once that work is dropped.
        stats.append((st["frames"], st["ahead_resumed"] + st["ahead_finished"]))
    if with_aov:
        c.render_aov(RW, RH, 1)
    frames.append(c.read_framebuffer(RW, RH))
    return frames, stats


@pytest.mark.parametrize("spp, params", [(1, {"path_kernel": 2, "render_ahead": 3}),
                                         (8, {"path_kernel": 1, "render_ahead": 3})])
def test_synchronous_series_are_untouched(spp, params):
    sd = S.config2(RW, RH, n_strands=200)
    with Ctx(sd, **params) as c:
        plain, st_plain = _sync_series(c, spp, False)
    with Ctx(sd, **params) as c:
        mixed, st_mixed = _sync_series(c, spp, True)
    print(f"spp {spp}: (frames, ahead_resumed, ahead_finished) per call {st_plain}")
    for k, (a, b) in enumerate(zip(plain, mixed)):
        assert a.tobytes() == b.tobytes(), f"framebuffer after call {k}"
    assert st_plain == st_mixed


def test_fused_asynchronous_passes_are_untouched():
    sd = S.config2(RW, RH, n_strands=200)

    def series(c, with_aov):
        for k in range(5):
            c.render(RW, RH, 1, DEPTH, first_sample=k, async_=True)
            if with_aov and k in (1, 4):
                c.render_aov(RW, RH, 2, first_sample=k)
        c.sync()
        return c.read_framebuffer(RW, RH), c.stats()["frames"]

    with Ctx(sd) as c:
        fb_plain, n_plain = series(c, False)
    with Ctx(sd) as c:
        fb_mixed, n_mixed = series(c, True)
    assert fb_plain.tobytes() == fb_mixed.tobytes()
    assert n_plain == n_mixed == 5


# ---- 4. the restated camera rays are the renderer's -------------------------------------------------------
def rows(*cols):
    """A multiset of float32 records as sorted rows of bits."""
    m = np.concatenate([np.asarray(c, F32).reshape(len(c), -1) for c in cols], axis=1).view(np.uint32)
    return m[np.lexsort(m.T[::-1])]


def test_restated_camera_rays_are_the_beauty_frames_bounce_0():
    sd = hairball_scene()
    with Ctx(sd, dump_bounce=0) as c:
        c.render(W, H, 1, DEPTH, seed=SEEDS[1], first_sample=3)
        (qo, qd), _ = c.debug_queues()
    pixels = np.arange(W * H, dtype=np.uint64)
    o, raw, _ = A.camera_rays(sd.cam, W, pixels, SEEDS[1], np.full(W * H, 3, np.uint64))
    assert len(qo) == W * H
    assert np.array_equal(rows(qo, qd), rows(o, A.normalize32(raw)))


# ---- 5. refusals on a context -----------------------------------------------------------------------------
def test_context_without_scene_or_tree_is_not_ready():
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    out = np.zeros((H, W), F32)
    ab = N.AovBuffers()
    ab.depth = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    p = N.RenderParams(W, H, 1, 0, 1, 0, 0, 0, 1, 0)
    c = HipContext(0)
    try:
        assert lib.khp_render_aov(c.ptr, ctypes.byref(p), ctypes.byref(ab)) == N.KHP_ENOTREADY and "khp_set_scene" in err()
        c.set_scene(hairball_scene())
        assert lib.khp_render_aov(c.ptr, ctypes.byref(p), ctypes.byref(ab)) == N.KHP_ENOTREADY and "khp_build_accel" in err()
        c.build_accel()
        assert lib.khp_render_aov(c.ptr, ctypes.byref(p), ctypes.byref(ab)) == N.KHP_OK, err()
        with pytest.raises(N.KhpError) as e:
            c.render_aov(W, H, 0)
        assert e.value.status == N.KHP_EINVAL
    finally:
        c.close()
