"""The environment light on the device (include/kirk_hip.h "an importance-sampled HDR environment light",
DESIGN.md §23).  Frames with the light on have no CPU oracle; these tests stand in for one:

 6. The queries: the device's tables equal the host's word for word (a 4096 x 8 and a 5 x 2048 map take the
    row loop's carry and the marginal's block loop past one step), khp_debug_env_light equals the host
    entries bit for bit on 4096 items plus the lattice, a device map builds the same tables, a bad texel of
    a device map is refused.
 7. Untouched defaults: never set, and set then cleared, config 2 is the oracle's frame.
 8. Shadow rays: the bounce-0 shadow rays of a render equal a numpy replay as multisets of bit rows, without
    lights and with one point light and select = 0.5.
 9. Two estimators of one integral: nee = 1 and nee = 0 agree per pixel class and channel within 4 standard
    errors of the difference plus depth * 2 * 4 pi * 1e-4 of the mean; background pixels are equal bit for bit.
10. Why it exists: under a map with one bright texel the summed variance of the pixel means is lower with nee = 1.
11. A function of the samples: every schedule renders the wavefront's frame; the AOV planes ignore the light.
12. Refusals, each changing nothing; scene and camera changes leave the light on; a change in mid-series
    completes the frames in flight with the old light.
"""
import ctypes

import numpy as np
import pytest

import _aovref as A
import oracle_ffi
from _furref import draw_u01
from _util import compare_images
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S
from ba_pathtracing_fur_amd.pathtracer import (DeviceBuffer, HipContext, comm_init_local, env_light_eval_host,
                                               env_light_sample_host, env_light_tables_host, hair_eval_host)

pytestmark = pytest.mark.gpu

F32 = np.float32
W_, H_, SPP, DEPTH, STRANDS = 64, 48, 4, 5, 200
SEED = 0x4B49524B
ONE_M = 1.0 - 2.0 ** -24
FLT_MAX = np.finfo(F32).max
WAVEFRONT = dict(path_kernel=1, path_from=0, ray_sort_from=9, render_ahead=0)
FIBRE = dict(color=(0.545, 0.353, 0.169), beta_m=0.3, beta_n=0.3, alpha=2.0, ior=1.55)


def same(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return compare_images(a, b)["bitexact"]


def rows(*cols):
    """A multiset of float32 records as sorted rows of bits."""
    m = np.concatenate([np.asarray(c, F32).reshape(len(c), -1) for c in cols], axis=1).view(np.uint32)
    return m[np.lexsort(m.T[::-1])] if len(m) else m


def dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize32(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a * (F32(1.0) / np.sqrt(dot32(a, a)))[:, None]


class _Ctx:
    """A context of its own with the scene built on it."""

    def __init__(self, sd=None, **params):
        self.ctx = HipContext(0)
        if sd is not None:
            self.ctx.set_scene(sd)
            self.ctx.build_accel()
        if params:
            self.ctx.set_params(**params)

    def __enter__(self):
        return self.ctx

    def __exit__(self, *a):
        self.ctx.close()


_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def seeded_map(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, (h, w, 3)) ** 4 * 20.0).astype(F32)


def sun_map(w=64, h=32):
    return S.sky_map(w, h, sun_dir=(0.3, 0.8, 0.5), sun_radiance=(400.0, 360.0, 300.0), sun_half_angle=0.05)


def patch_map():
    """A 64 x 32 gradient sky with a 2 x 2 patch of radiance 50."""
    m = S.sky_map(64, 32, sun_radiance=(0.9, 0.95, 1.0), sun_half_angle=0.0)
    m[24:26, 10:12] = 50.0
    return m


def assert_tables_equal(got, ref):
    for k in ("weight", "row_cdf", "marginal"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k


# ---- 6. the queries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(32, 16), (64, 32), (4096, 8), (5, 2048), (257, 129)])
def test_device_tables_equal_the_hosts(w, h):
    rgb = seeded_map(w, h, 40 + w)
    rgb[h // 2, : w // 2] = 0.0                       # texels that do not emit, a run of them
    with _Ctx() as c:
        c.set_env_light(rgb)
        assert_tables_equal(c.debug_env_light_tables(), env_light_tables_host(rgb))
        # the same map in device memory builds the same tables
        buf = DeviceBuffer.from_array(c, rgb)
        c.clear_env_light()
        c.set_env_light(buf, device_shape=(h, w), scale=2.0)
        assert_tables_equal(c.debug_env_light_tables(), env_light_tables_host(rgb))
        assert c.env_light() == dict(width=w, height=h, nee=True, scale=2.0, rotation=0.0, select=0.5)
        buf.free()


def query_lattice(w, h, rotation):
    dirs = [(0, 1, 0), (0, -1, 0), (0, 3, 0), (-1, 0, 0.0), (-1, 0, -0.0), (1, 0, 0), (0, 0, 1), (0, 0, -1), (2, 2, 2),
            (0, 0, 0), (np.cos(rotation), 0, np.sin(rotation))]
    for j in sorted({0, 1, h // 2, h - 1, h}):
        for i in sorted({0, 1, w // 2, w - 1}):
            th, ph = j * np.pi / h, i * 2 * np.pi / w + rotation
            dirs.append((np.sin(th) * np.cos(ph), -np.cos(th), np.sin(th) * np.sin(ph)))
    us = [(0, 0), (ONE_M, ONE_M), (0, ONE_M), (ONE_M, 0), (0.5, 0.5), (0.5, 0), (0, 0.5), (2.0 ** -24, 2.0 ** -24)]
    n = max(len(dirs), len(us))
    return F32([dirs[k % len(dirs)] for k in range(n)]), F32([us[k % len(us)] for k in range(n)])


@pytest.mark.parametrize("case", ["sun", "seeded"])
def test_device_sampler_and_evaluation_equal_the_host_entries(case):
    rgb, prm = {"sun": (sun_map(), dict(scale=2.5, rotation=0.7)), "seeded": (seeded_map(257, 129, 5), dict(rotation=-2.0))}[case]
    rng = np.random.default_rng(17)
    ld, lu = query_lattice(rgb.shape[1], rgb.shape[0], prm["rotation"])
    v = rng.standard_normal((4096, 3))
    dirs = np.concatenate([(v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (4096, 1))).astype(F32), ld])
    us = np.concatenate([(rng.integers(0, 1 << 24, (4096, 2)) / float(1 << 24)).astype(F32), lu])
    with _Ctx() as c:
        c.set_env_light(rgb, **prm)
        dev = c.debug_env_light(us, dirs)
    hs, he = env_light_sample_host(rgb, us, **prm), env_light_eval_host(rgb, dirs, **prm)
    for k in ("dir", "pdf", "radiance"):
        assert np.array_equal(A.bits(dev[k]), A.bits(hs[k])), k
    assert np.array_equal(dev["valid"], hs["valid"]) and hs["valid"][:4096].all()
    assert np.array_equal(A.bits(dev["e_radiance"]), A.bits(he["radiance"]))
    assert np.array_equal(A.bits(dev["e_pdf"]), A.bits(he["pdf"])) and (he["pdf"] > 0).any()


def test_a_bad_texel_of_a_device_map_is_refused_and_the_light_stays():
    good = seeded_map(32, 16, 3)
    with _Ctx() as c:
        c.set_env_light(good, scale=3.0)
        before = c.debug_env_light_tables()
        for bad in (np.nan, -1.0, np.inf):
            m = good.copy()
            m[9, 20, 1] = bad
            m[12, 3, 0] = -2.0                        # a later one: the first is named
            buf = DeviceBuffer.from_array(c, m)
            with pytest.raises(N.KhpError) as e:
                c.set_env_light(buf, device_shape=(16, 32))
            assert e.value.status == N.KHP_EINVAL and "texel (20, 9)" in str(e.value)
            buf.free()
        buf = DeviceBuffer.from_array(c, np.zeros((16, 32, 3), F32))
        with pytest.raises(N.KhpError) as e:
            c.set_env_light(buf, device_shape=(16, 32))
        assert e.value.status == N.KHP_EINVAL and "black" in str(e.value)
        buf.free()
        assert c.env_light()["scale"] == 3.0
        assert_tables_equal(c.debug_env_light_tables(), before)


# ---- 7. untouched defaults --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def marschner_scene():
    return cached("marschner", lambda: S.config2(W_, H_, n_strands=STRANDS))


@pytest.mark.parametrize("path_kernel", [1, 2])
def test_without_the_light_config2_is_the_oracles(marschner_scene, path_kernel):
    ref = cached("oracle", lambda: oracle_ffi.Oracle(marschner_scene).render(W_, H_, 2, DEPTH, threads=8))
    with _Ctx(marschner_scene, path_kernel=path_kernel) as c:
        assert same(c.render(W_, H_, 2, DEPTH), ref)                 # never set
        c.set_env_light(sun_map())
        lit = c.render(W_, H_, 2, DEPTH)
        assert not same(lit, ref)                                    # (a Marschner frame holds non-finite pixels)
        c.clear_env_light()
        assert c.env_light()["width"] == 0
        assert same(c.render(W_, H_, 2, DEPTH), ref)                 # set, then cleared


# ---- 8. the shadow rays -----------------------------------------------------------------------------------
RW, RH = 24, 24
P_LIGHT_SEL, P_LIGHT_0, P_LIGHT_1 = 4, 5, 6
OFFSET = F32(1e-4)
CONE_BASE, CONE_APEX = F32([-1.0, 0.0, 0.0, 0.2]), F32([1.0, 0.02, 0.0, 0.15])


def one_cone_scene(light):
    sd = S.SceneData(name="one_cone")
    sd.add_cones(CONE_BASE[None], CONE_APEX[None], sd.add_material(S.hair_material(**FIBRE)))
    if light:
        sd.lights.append(S.point_light((0.5, 1.0, 1.0), (5.0, 5.0, 5.0), radius=0.1))
    sd.env_ambient = (0.0, 0.0, 0.0)
    sd.cam = S.camera((0.0, 0.05, 1.5), (0.0, 0.0, -1.0), width=RW, height=RH)
    return sd


def moved_origin(base, V, nrm, wo, w, loc, org):
    """The origin rule of DESIGN.md §22 in float32: a direction w that enters the fibre starts beyond its far wall."""
    front = dot32(wo, nrm) >= 0
    npr = np.where(front[:, None], nrm, -nrm)
    into = dot32(w, npr) < 0
    base_d = dot32(np.broadcast_to(base, V.shape), V)
    tt = dot32(loc, V) - base_d
    q1 = loc - V * tt[:, None]
    e = q1 - base
    rho = np.sqrt(dot32(e, e))
    npp = normalize32(npr - V * dot32(npr, V)[:, None])
    c = -dot32(w, npp)
    dv = dot32(w, V)
    k = F32(1.0) - dv * dv
    with np.errstate(invalid="ignore", divide="ignore"):
        tx = np.where(k > F32(1e-8), ((F32(2.0) * rho) * c) / k, F32(0.0)).astype(F32)
    far = loc + w * (tx * F32(1.001) + OFFSET)[:, None]
    return np.where(into[:, None], far, org).astype(F32)


def replay_shadow_rays(c, sd, rgb, select):
    """The shadow rays of bounce 0 rebuilt from khp_debug_surface, the host sampler and kind 11's origin rule:
    towards the map (t_max FLT_MAX) where the draw says so, towards the light otherwise."""
    m = sd.materials[0]
    px = np.arange(RW * RH, dtype=np.uint32)
    o, raw, key = A.camera_rays(sd.cam, RW, px, SEED, np.zeros_like(px))
    d = A.normalize32(raw)
    hit = c.debug_surface(o, raw)
    lam = hit["t"]
    surf = lam != FLT_MAX
    if sd.lights:
        li = c.debug_light_isect(np.zeros(len(px), np.int32), o, raw)
        surf &= ~((li["hit"] != 0) & (li["t"] < lam))
    o, d, key = o[surf], d[surf], key[surf]
    nrm, lam, uvw = hit["n"][surf], lam[surf], hit["uvw"][surf]
    n = len(o)
    V = uvw[:, 1]
    loc = d * lam[:, None] + o
    counter = -normalize32(d)
    u = np.stack([draw_u01(key, P_LIGHT_0), draw_u01(key, P_LIGHT_1)], axis=1)
    usel = draw_u01(key, P_LIGHT_SEL)
    to_map = (usel < F32(select)) if sd.lights else np.ones(n, bool)
    # towards the map
    s = env_light_sample_host(rgb, u)
    ed = s["dir"]
    side = dot32(nrm, -ed) < 0
    eo = (loc + np.where(side[:, None], nrm, -nrm) * OFFSET).astype(F32)
    eo = moved_origin(CONE_BASE[:3], V, nrm, counter, ed, loc, eo)
    fe = hair_eval_host(m, uvw, nrm, -d, ed)
    ad = np.abs(dot32(ed, nrm))
    wsel = F32(1.0) / F32(select) if sd.lights else F32(1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        lc = s["radiance"] * (((fe * ad[:, None]) / s["pdf"][:, None]) * wsel)
    env = to_map & (s["valid"] != 0) & (lc != 0).any(axis=1)
    out_o, out_d, out_t = [eo[env]], [ed[env]], [np.full(int(env.sum()), FLT_MAX, F32)]
    n_light = 0
    if sd.lights:
        L = sd.lights[0]
        ld = c.debug_light_dir(np.zeros(n, np.int32), loc, u)
        lightpos = ld["o"] + ld["d"]
        side = dot32(nrm, ld["o"] - lightpos) < 0
        so = ld["o"] + np.where(side[:, None], nrm, -nrm) * OFFSET
        sdir = normalize32(ld["d"])
        so = moved_origin(CONE_BASE[:3], V, nrm, counter, sdir, loc, so)
        e = lightpos - so
        tmax = np.sqrt(dot32(e, e))
        f_l = hair_eval_host(m, uvw, nrm, -d, sdir)
        adl = np.abs(dot32(sdir, nrm))
        lcl = F32(list(L.color))[None, :] * ((ld["att"][:, None] * f_l) * adl[:, None])
        lit = ~to_map & (lcl != 0).any(axis=1)
        n_light = int(lit.sum())
        out_o.append(so[lit]); out_d.append(sdir[lit]); out_t.append(tmax[lit])
    return np.concatenate(out_o), np.concatenate(out_d), np.concatenate(out_t), int(env.sum()), n_light, n


@pytest.mark.parametrize("light", [False, True])
def test_shadow_rays_are_the_replays(light):
    sd = one_cone_scene(light)
    rgb = sun_map()
    with _Ctx(sd, path_kernel=1) as c:
        c.set_env_light(rgb, select=0.5)
        wo, wd, wt, n_env, n_light, n_surf = replay_shadow_rays(c, sd, rgb, 0.5)
        c.set_params(dump_bounce=0)
        c.render(RW, RH, 1, 3, seed=SEED)
        _, (so, sdir, st) = c.debug_queues()
    print(f"light {light}: {n_surf} hits, {n_env} shadow rays to the map, {n_light} to the light, {len(so)} dumped")
    assert n_surf > RW * RH // 8 and n_env > 0 and (n_light > 0) == light
    if light:
        assert 0.25 < n_env / (n_env + n_light) < 0.75          # the draw splits them
    assert int((st == FLT_MAX).sum()) == n_env
    assert np.array_equal(rows(so, sdir, st), rows(wo, wd, wt))


# ---- 9. two estimators of one integral --------------------------------------------------------------------
EW, EH, ESPP, EDEPTH = 64, 48, 256, 4


def estimator_scene(light=False, ground_only=False):
    sd = S.SceneData(name="env_estimators")
    v, n = S.quad((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3), (0, 1, 0))
    sd.add_triangles(v, n, sd.add_material(S.material(diffuse=(0.6, 0.6, 0.6))))
    if not ground_only:
        gv, gn = S.icosphere(1, (0.55, 0.3, 0.3), 0.28)
        sd.add_triangles(gv, gn, sd.add_material(S.material("GlassBSDF", volume=(1.0, 0.95, 0.9), ior=1.52)))
        pos, rad = S.hairball(STRANDS, (-0.25, 0.45, 0.0), 0.25)
        sd.add_fibers(pos, rad, sd.add_material(S.hair_material(**FIBRE)))
    if light:
        sd.lights.append(S.point_light((1.0, 2.0, 1.5), (3.0, 3.0, 3.0), radius=0.1))
    sd.env_ambient = (0.0, 0.0, 0.0)
    sd.cam = S.camera((0.0, 0.9, 2.2), (0.0, -0.3, -1.0), width=EW, height=EH)
    return sd


def moments_render(c, spp, depth):
    c.set_moments(False)
    c.set_moments(True)
    c.render(EW, EH, spp, depth, seed=SEED, readback=False)
    st = c.read_moments(EW, EH)
    assert (st["bad"] == 0).all() and (st["count"] == spp).all()
    return st["mean"].astype(np.float64), st["m2"].astype(np.float64) / (spp * (spp - 1.0))


@pytest.mark.parametrize("light", [False, True])
def test_nee_and_escaping_rays_estimate_one_integral(light):
    sd = estimator_scene(light)
    rgb = patch_map()
    with _Ctx(sd) as c:
        aov = c.render_aov(EW, EH, ESPP, seed=SEED, channels=("object", "coverage"))
        c.set_env_light(rgb, nee=True)
        m1, v1 = moments_render(c, ESPP, EDEPTH)
        c.set_env_light(rgb, nee=False)
        m0, v0 = moments_render(c, ESPP, EDEPTH)
    obj, n_tris = aov["object"], len(sd.tri_v)
    background = aov["coverage"] == 0                              # no sample of the pixel hits anything
    mat = np.where(obj < n_tris, np.asarray(sd.tri_mat).astype(np.int64)[np.clip(obj, 0, n_tris - 1)], 2)
    mat = np.where(background | (obj < 0), -1, mat)
    assert background.sum() > 50
    assert np.array_equal(m1[background].astype(F32).view(np.uint32), m0[background].astype(F32).view(np.uint32))
    assert (m0[background] > 0).all()
    for name, k in (("ground", 0), ("glass", 1), ("fibre", 2), ("background", -1)):
        px = mat == k
        assert px.sum() > 30, (name, int(px.sum()))
        a, b = m1[px].mean(0), m0[px].mean(0)
        se = np.sqrt(v1[px].sum(0) + v0[px].sum(0)) / px.sum()
        allow = 4 * se + EDEPTH * 2 * 4 * np.pi * 1e-4 * np.maximum(a, b)
        print(f"light {light}, {name}: {int(px.sum())} pixels, nee 1 {a}, nee 0 {b}, 4 se {4 * se}, "
              f"variance ratio nee0/nee1 {v0[px].sum(0) / np.maximum(v1[px].sum(0), 1e-300)}")
        assert (a > 0).all()
        assert (np.abs(a - b) <= allow).all(), (name, a, b, allow)


# ---- 10. why it exists ------------------------------------------------------------------------------------
def test_a_small_bright_texel_converges_faster_with_nee():
    rgb = np.full((32, 64, 3), 0.2, F32)
    rgb[26, 13] = 5000.0
    with _Ctx(estimator_scene(ground_only=True)) as c:
        c.set_env_light(rgb, nee=True)
        m1, v1 = moments_render(c, 64, 3)
        c.set_env_light(rgb, nee=False)
        m0, v0 = moments_render(c, 64, 3)
    ratio = v0.sum() / v1.sum()
    print(f"one texel of 5000 in a map of 0.2, 64 spp: summed variance of the pixel means nee 0 / nee 1 = {ratio:.1f}; "
          f"frame means {m1.mean():.4f} (nee 1), {m0.mean():.4f} (nee 0)")
    assert v1.sum() < v0.sum()


# ---- 11. a function of the samples ------------------------------------------------------------------------
LIGHT = dict(scale=1.5, rotation=0.4, select=0.5)


@pytest.fixture(scope="module")
def scene():
    return cached("scene", lambda: estimator_scene(light=True))


def lit_ctx(sd, **params):
    x = _Ctx(sd, **params)
    x.ctx.set_env_light(sun_map(), **LIGHT)
    return x


@pytest.fixture
def lit_frame(scene):
    def make():
        with lit_ctx(scene, **WAVEFRONT) as c:
            return c.render(W_, H_, SPP, DEPTH)
    return cached("lit_frame", make)


def test_the_lit_frame_is_finite_and_not_the_unlit_one(scene, lit_frame):
    assert np.isfinite(lit_frame).all() and (lit_frame > 0).any()
    with _Ctx(scene, **WAVEFRONT) as c:
        assert not same(c.render(W_, H_, SPP, DEPTH), lit_frame)


@pytest.mark.parametrize("schedule", ["path_kernel", "path_kernel_wide0", "path_from", "ray_sort_from", "shade_order"])
def test_schedules_render_one_frame(scene, lit_frame, schedule):
    prm = {"path_kernel": dict(path_kernel=2), "path_kernel_wide0": dict(path_kernel=2, wide_from=0),
           "path_from": dict(path_kernel=1, path_from=2), "ray_sort_from": dict(path_kernel=1, ray_sort_from=1),
           "shade_order": dict(path_kernel=1, shade_order=1)}[schedule]
    with lit_ctx(scene, **prm) as c:
        assert same(c.render(W_, H_, SPP, DEPTH), lit_frame)


def test_fused_asynchronous_passes(scene, lit_frame):
    with lit_ctx(scene) as c:
        for k in range(SPP):
            c.render(W_, H_, 1, DEPTH, first_sample=k, async_=True)
        c.sync()
        assert same(c.read_framebuffer(W_, H_), lit_frame)


def test_render_ahead_0_equals_3(scene, lit_frame):
    frames = []
    for ahead in (0, 3):
        with lit_ctx(scene, path_kernel=2, render_ahead=ahead) as c:
            for k in range(SPP):
                c.render(W_, H_, 1, DEPTH, first_sample=k, readback=False)
            frames.append(c.read_framebuffer(W_, H_))
    assert same(frames[0], frames[1]) and same(frames[0], lit_frame)


def test_two_ranks_gathered_equal_one_context(scene, lit_frame):
    ctxs = [HipContext(0) for _ in range(2)]
    try:
        for c in ctxs:
            c.set_scene(scene)
            c.build_accel()
            c.set_env_light(sun_map(), **LIGHT)
        comm_init_local(ctxs)
        for r in reversed(range(2)):
            ctxs[r].render(W_, H_, SPP, DEPTH, tile_size=16, tile_rank=r, tile_nranks=2, readback=False)
            ctxs[r].gather_framebuffer(W_, H_, SPP, DEPTH, 16, 2, r, 0)
        ctxs[1].sync()
        ctxs[0].sync()
        assert same(ctxs[0].read_framebuffer(W_, H_), lit_frame)
    finally:
        for c in ctxs:
            c.close()


def test_adaptive_series_with_every_pixel_active(scene, lit_frame):
    with lit_ctx(scene) as c:
        c.set_moments(True)
        for k in range(SPP):
            _, res = c.render_adaptive(W_, H_, 1, DEPTH, first_sample=k, threshold=0.0, min_samples=SPP + 1,
                                       max_samples=0, readback=False)
            assert res == {"owned": W_ * H_, "active": W_ * H_}
        fb, st = c.read_framebuffer(W_, H_), c.read_moments(W_, H_)
    assert (st["bad"] == 0).all()
    assert np.array_equal(A.bits(st["mean"]), A.bits(lit_frame)) and np.array_equal(A.bits(fb), A.bits(st["mean"]))


def test_a_lens_and_a_textured_scene():
    frames = []
    sd = S.textured(W_, H_, n_strands=STRANDS)
    for prm in (WAVEFRONT, dict(path_kernel=2), dict(path_kernel=1, path_from=2)):
        with lit_ctx(sd, **prm) as c:
            c.set_lens(radius=0.0692, focus_distance=1.0, focus=N.LENS_FOCUS_PLANE)
            frames.append(c.render(W_, H_, SPP, DEPTH))
    assert same(frames[0], frames[1]) and same(frames[0], frames[2])   # (Marschner fur: not finite everywhere, §2)
    assert (np.nan_to_num(frames[0], nan=0.0, posinf=0.0, neginf=0.0) > 0).any()


def test_the_aov_planes_ignore_the_light(scene):
    with _Ctx(scene) as c:
        before = c.render_aov(W_, H_, 2, seed=SEED)
        c.set_env_light(sun_map(), **LIGHT)
        after = c.render_aov(W_, H_, 2, seed=SEED)
    for k in before:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k


# ---- 12. refusals -----------------------------------------------------------------------------------------
def stats_bytes(c):
    s = N.Stats()
    N.check(c.lib, c.lib.khp_get_stats(c.ptr, ctypes.byref(s)), "khp_get_stats")
    return bytes(s)


def test_refusals_change_nothing(scene, marschner_scene):
    good = sun_map()

    def state(c):
        return (c.read_framebuffer(W_, H_).tobytes(), stats_bytes(c), c.set_bdpt()["enabled"], c.hair_lobes,
                tuple(sorted(c.env_light().items())))

    with lit_ctx(scene, **WAVEFRONT) as c:
        before = c.render(W_, H_, 1, DEPTH)
        st = state(c)
        for bad, where in ((np.nan, (5, 2)), (-1.0, (0, 0)), (np.inf, (63, 31))):
            m = good.copy()
            m[where[1], where[0], 2] = bad
            with pytest.raises(N.KhpError) as e:
                c.set_env_light(m)
            assert e.value.status == N.KHP_EINVAL and "texel (%d, %d)" % where in str(e.value)
            assert state(c) == st
        for m, kw, word in ((np.zeros((4, 4, 3), F32), {}, "black"), (good, dict(select=0.0), "select"),
                            (good, dict(select=1.25), "select"), (good, dict(scale=0.0), "scale"),
                            (good, dict(scale=np.inf), "scale"), (good, dict(rotation=np.nan), "rotation"),
                            (np.ones((2049, 1, 3), F32), {}, "height"), (np.ones((1, 4097, 3), F32), {}, "width")):
            with pytest.raises(N.KhpError) as e:
                c.set_env_light(m, **kw)
            assert e.value.status == N.KHP_EINVAL and word in str(e.value), (kw, str(e.value))
            assert state(c) == st
        prm = N.EnvLight(64, 32, 0, 1, 1.0, 0.0, 0.5, 1, good.ctypes.data)
        assert c.lib.khp_set_env_light(c.ptr, ctypes.byref(prm)) == N.KHP_EINVAL and state(c) == st   # reserved
        assert same(c.render(W_, H_, 1, DEPTH), before)
    # the light, then the light-path variant or other lobes (a scene without kind 11, which refuses them itself)
    with lit_ctx(marschner_scene, **WAVEFRONT) as c:
        before = c.render(W_, H_, 1, DEPTH)
        st = state(c)
        with pytest.raises(N.KhpError) as e:
            c.set_bdpt(enabled=1, light_paths=4, vertices=2)
        assert e.value.status == N.KHP_EUNSUPPORTED and "khp_set_env_light" in str(e.value)
        for lobes in (N.HAIR_LOBE_R | N.HAIR_LOBE_TT, N.HAIR_LOBE_TRT):
            with pytest.raises(N.KhpError) as e:
                c.set_hair_lobes(lobes)
            assert e.value.status == N.KHP_EUNSUPPORTED and "khp_set_env_light" in str(e.value)
        assert state(c) == st
        assert same(c.render(W_, H_, 1, DEPTH), before)
    # the light-path variant or other lobes, then the light
    for setup in ("bdpt", "lobes"):
        with _Ctx(marschner_scene, **WAVEFRONT) as c:
            if setup == "bdpt":
                c.set_bdpt(enabled=1, light_paths=4, vertices=2)
            else:
                c.set_hair_lobes(N.HAIR_LOBE_R | N.HAIR_LOBE_TT)
            before = c.render(W_, H_, 1, 3)
            st = state(c)
            with pytest.raises(N.KhpError) as e:
                c.set_env_light(good)
            assert e.value.status == N.KHP_EUNSUPPORTED and state(c) == st
            assert same(c.render(W_, H_, 1, 3), before)


def test_scene_and_camera_changes_leave_the_light_on(scene, lit_frame):
    with lit_ctx(estimator_scene(light=False), **WAVEFRONT) as c:
        c.render(W_, H_, 1, DEPTH)
        c.set_scene(scene)
        c.build_accel()
        c.set_camera(scene.cam)
        assert c.env_light()["width"] == 64
        assert same(c.render(W_, H_, SPP, DEPTH), lit_frame)


def test_a_change_in_mid_series_completes_the_frames_in_flight_with_the_old_light(scene):
    a, b = sun_map(), patch_map()
    frames = []
    for asynchronous in (True, False):
        with _Ctx(scene) as c:
            c.set_env_light(a, **LIGHT)
            for k in range(2):
                c.render(W_, H_, 1, DEPTH, first_sample=k, async_=asynchronous, readback=False)
            c.set_env_light(b)
            for k in range(2, 4):
                c.render(W_, H_, 1, DEPTH, first_sample=k, async_=asynchronous, readback=False)
            c.sync()
            frames.append(c.read_framebuffer(W_, H_))
    assert same(frames[0], frames[1]) and np.isfinite(frames[0]).all()
