"""numpy restatement of khp_render_aov (include/kirk_hip.h) for the tests.

Three parts, each what the definition says and nothing of the kernels:
  * the camera rays: path_key (kmath.h:330), draws dim_of(0, P_CAM_X / P_CAM_Y), and
    camera_path's float32 arithmetic, as tests/test_gpu_hair_lobes.py::replay restates it;
  * per-sample features from the batch queries khp_debug_surface and khp_debug_light_isect,
    which tests/test_shading_truth.py pins to a float64 truth;
  * the ordered float32 sum over a pixel's samples and the division by float32(spp).
"""
import numpy as np

from _furref import M32, draw_u01, lowbias32

F32 = np.float32
FLT_MAX = np.finfo(F32).max
P_CAM_X, P_CAM_Y = 0, 1
FLOAT_CHANNELS = ("normal", "albedo", "tangent", "depth", "coverage")
CHANNELS = FLOAT_CHANNELS + ("object",)
WIDTH = {"normal": 3, "albedo": 3, "tangent": 3, "depth": 1, "coverage": 1}


def path_key(seed, pixel, sample):
    """kmath.h path_key on arrays: lowbias32(lowbias32(lowbias32(seed ^ KIRK) ^ pixel) + sample * golden)."""
    pixel = np.asarray(pixel, np.uint64)
    sample = np.asarray(sample, np.uint64)
    k0 = lowbias32(np.uint64((seed ^ 0x4B49524B) & 0xFFFFFFFF))
    return lowbias32((lowbias32(k0 ^ pixel) + sample * np.uint64(0x9E3779B9)) & M32)


def camera_rays(cam, width, pixels, seed, samples):
    """camera_path for every (pixel, sample) pair (elementwise arrays): origin, the
    *unnormalised* direction (a query normalises what it is given, as KIRK::Ray does) and the key."""
    pixels = np.asarray(pixels, np.uint64)
    key = path_key(seed, pixels, samples)
    x, y = (pixels % np.uint64(width)).astype(F32), (pixels // np.uint64(width)).astype(F32)
    s1 = (x + draw_u01(key, P_CAM_X)) * F32(cam.pixel_size)
    s2 = (y + draw_u01(key, P_CAM_Y)) * F32(cam.pixel_size)
    v = lambda a: np.tile(F32(list(a)), (len(pixels), 1))
    raw = ((v(cam.bottom_left) + v(cam.axis_x) * s1[:, None]) + v(cam.axis_y) * s2[:, None]) - v(cam.position)
    return v(cam.position), raw.astype(F32), key


def normalize32(a):
    """kmath.h normalize: a * (1 / sqrt((x x + y y) + z z))."""
    d = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a * (F32(1.0) / np.sqrt(d))[:, None]).astype(F32)


def albedo_table(sd):
    """The resolved diffuse of every material.  A textured diffuse must be one colour all over
    (the tests' textures are): Material::getFromParam then gives texel / 255 wherever the hit is
    (Texture::getColor: rgb of 3- and 4-channel texels)."""
    tab = np.zeros((len(sd.materials), 3), F32)
    for i, m in enumerate(sd.materials):
        tab[i] = F32(list(m.diffuse))
        mt = sd.material_textures
        if mt is not None and i < len(mt) and mt[i][0] >= 0:
            texels = sd.textures[int(mt[i][0])][0]
            assert texels.shape[2] >= 3 and (texels == texels[0, 0]).all(), "constant rgb textures only"
            tab[i] = texels[0, 0, :3].astype(F32) / F32(255.0)
    return tab


def sample_records(ctx, sd, o, raw, albedo=None):
    """The definition's per-sample record for rays (o, raw): dict of float columns, `object`, and
    `light_ended` (a hit that a nearer light takes: not a surface sample).  albedo: the resolved
    diffuse of every ray's hit (n, 3), for textures that are not one colour (khp_debug_material's
    answer); without it albedo_table's."""
    n = len(o)
    hit = ctx.debug_surface(o, raw)
    t_lights = np.full(n, FLT_MAX, F32)
    for li in range(len(sd.lights)):
        r = ctx.debug_light_isect(np.full(n, li, np.int32), o, raw)
        t = np.where(r["hit"] != 0, r["t"], FLT_MAX).astype(F32)
        t_lights = np.where(t < t_lights, t, t_lights)            # gmin(t_lights, t)
    has = hit["obj"] >= 0
    with np.errstate(invalid="ignore"):
        surf = has & ~(t_lights < hit["t"])
    zero3 = np.zeros((n, 3), F32)
    alb = albedo_table(sd)[np.where(surf, hit["mat"], 0)] if albedo is None else np.asarray(albedo, F32)
    return {"normal": np.where(surf[:, None], hit["n"], zero3),
            "albedo": np.where(surf[:, None], alb, zero3),
            "tangent": np.where(surf[:, None], hit["uvw"][:, 1], zero3),
            "depth": np.where(surf, hit["t"], F32(0.0)).astype(F32),
            "coverage": surf.astype(F32),
            "object": np.where(surf, hit["obj"], -1).astype(np.int32),
            "light_ended": has & ~surf}


def reduce_samples(rec, spp):
    """rec: (pixels, spp[, 3]) float32 records in sample order -> s / float32(spp) with s = +0,
    s += record k for k = 0 .. spp - 1, every add rounded to float32."""
    rec = np.asarray(rec, F32)
    s = np.zeros(rec.shape[:1] + rec.shape[2:], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):
            s = (s + rec[:, k]).astype(F32)
        return (s / F32(spp)).astype(F32)


def reduce_records(records, n_pixels, spp):
    """All channels of per-sample records laid out pixel-major (pixel * spp + sample)."""
    out = {}
    for ch in FLOAT_CHANNELS:
        r = np.asarray(records[ch], F32)
        out[ch] = reduce_samples(r.reshape((n_pixels, spp) + r.shape[1:]), spp)
    out["object"] = np.asarray(records["object"], np.int32).reshape(n_pixels, spp)[:, 0].copy()
    return out


def reference(ctx, sd, width, height, spp, seed, first_sample=0, cam=None):
    """khp_render_aov of the whole frame, restated: dict of (H, W[, 3]) arrays + `light_ended` count."""
    npix = width * height
    pixels = np.repeat(np.arange(npix, dtype=np.uint64), spp)
    samples = np.tile(np.arange(first_sample, first_sample + spp, dtype=np.uint64), npix)
    o, raw, _ = camera_rays(cam if cam is not None else sd.cam, width, pixels, seed, samples)
    rec = sample_records(ctx, sd, o, raw)
    out = reduce_records(rec, npix, spp)
    res = {ch: a.reshape((height, width) + a.shape[1:]) for ch, a in out.items()}
    res["light_ended"] = int(rec["light_ended"].sum())
    return res


def bits(a):
    """An array's bits with every NaN made one pattern: an invalid operation's NaN differs
    between hosts in sign and payload and no definition above depends on it (tests/_util.py)."""
    a = np.ascontiguousarray(a)
    if a.dtype != F32:
        return a
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
