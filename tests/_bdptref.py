"""Float64 reference of the light-path (bidirectional) variant, DESIGN.md §10
(tests/test_bdpt_truth.py).

Plain numpy over N items, written from what KIRK's GLSL computes
(lbb_construction.compute, pt_shade.compute, inc_random.compute, inc_light.compute
read as a specification) and from the deviations DESIGN.md §10 states; none of
the oracle's or the product's functions.  The closest hit comes from
_geomref's brute force (no BVH), normals and BSDFs from _shaderef.

Every function takes `dtype`: float64 is the truth, the same code in float32
only calibrates the tolerance.  Every function returns the branch signature
`sig` of each item (_shaderef.Sig), so that _shaderef.decisive() can tell which
items survive +-2 float32 ulps on their inputs.

A light subpath is a chain, and a float64 chain leaves a float32 chain at the
first grazing hit.  Nothing here follows a chain: `step` takes the recorded
(float32) state of vertex j - 1 and the recorded direction towards vertex j as
exact inputs and computes vertex j alone.
"""
import numpy as np

import _geomref as G
import _shaderef as R

GL_PI = np.float32(3.14159265359)            # inc_random.compute:11: a GLSL float, not pi
GL_ONE_OVER_PI = np.float32(0.31830988618)   # inc_random.compute:12
LPATH_SEED = 0x4C504154                      # the light-path key
IMG_BOUNCE = 4095                            # the image-plane pass' draws: bounce slot 4095
P_CAM_X, P_CAM_Y, P_BSDF_0, P_BSDF_1, P_LIGHT_SEL, P_LIGHT_0, P_LIGHT_1, P_HAIR_ALPHA, P_HAIR_BETA = range(9)
ATT_MIN = 1e-4                               # lbb_construction.compute: the path-length cut
M32 = np.uint64(0xFFFFFFFF)
SIG_W = 24                                   # columns of a step's signature (the BSDFs' differ in number)


# ---- the counter RNG of DESIGN.md §2: integer arithmetic, restated exactly -----------------------
def lowbias32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def path_key(seed, pixel, sample):
    """lowbias32(lowbias32(lowbias32(seed ^ 'KIRK') ^ pixel) + sample * golden)."""
    pixel, sample = np.asarray(pixel, np.uint64), np.asarray(sample, np.uint64)
    k0 = lowbias32(np.uint64((int(seed) ^ 0x4B49524B) & 0xFFFFFFFF))
    return lowbias32((lowbias32(k0 ^ pixel) + sample * np.uint64(0x9E3779B9)) & M32)


def light_key(seed, sub, n_lights, light, k):
    """The key of subpath `sub` of light `light` at sample index k: path_key(seed ^ 'LPAT', s L + l, k)."""
    return path_key((int(seed) ^ LPATH_SEED) & 0xFFFFFFFF, np.asarray(sub, np.uint64) * np.uint64(n_lights) +
                    np.asarray(light, np.uint64), k)


def dim(bounce, purpose):
    return np.asarray(bounce, np.uint64) * np.uint64(16) + np.uint64(purpose)


def draw_u01(key, d):
    """The top 24 bits of lowbias32(key ^ (dim * 0x85EBCA6B + 0x632BE5AB)) as a float32 in [0, 1)."""
    mixed = (np.asarray(d, np.uint64) * np.uint64(0x85EBCA6B) + np.uint64(0x632BE5AB)) & M32
    return ((lowbias32(np.asarray(key, np.uint64) ^ mixed) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def vertex0_draws(key):
    """(N, 4): the position draws (dims 5, 6) and the direction draws (2, 3) of bounce 0."""
    return np.stack([draw_u01(key, dim(0, p)) for p in (P_LIGHT_0, P_LIGHT_1, P_BSDF_0, P_BSDF_1)], axis=1)


def vertex_draws(key, j):
    """(N, 4): the BSDF draws (dims 2, 3) and the hair draws (7, 8) of bounce j."""
    return np.stack([draw_u01(key, dim(j, p)) for p in (P_BSDF_0, P_BSDF_1, P_HAIR_ALPHA, P_HAIR_BETA)], axis=1)


# ---- the GLSL samplers (inc_random.compute:50-81) ------------------------------------------------
def cosine_hemisphere(u, v, dt):
    """cosineHemisphereSample: the disk (sqrt(u), 2 PI v) projected up."""
    r, th = np.sqrt(u), 2 * dt(GL_PI) * v
    x, y = r * np.cos(th), r * np.sin(th)
    return R.vec(x, y, np.sqrt(np.maximum(0, 1 - x * x - y * y)))


def uniform_sphere(u, v, dt):
    """uniformSphereSample: cos(theta) = 2 u - 1, phi = 2 PI v."""
    phi, ct = v * 2 * dt(GL_PI), 2 * u - 1
    st = np.sqrt(np.maximum(0, 1 - ct * ct))
    return R.vec(st * np.cos(phi), st * np.sin(phi), ct)


def sample_angle(u, v, max_angle, dt):
    """sampleAngle: uniform in the cone of half angle max_angle about +z."""
    phi, ct = v * 2 * dt(GL_PI), 1 - u * (1 - np.cos(max_angle))
    with np.errstate(invalid="ignore"):
        st = np.sqrt(1 - ct * ct)
    return R.vec(np.cos(phi) * st, np.sin(phi) * st, ct)


def to_world(v, n, sig, where=None):
    """The (s, t, n) frame of lbb_construction.compute:42-45 (localToWorld, BSDF/header.compute:23-26):
    s in the y-z plane when n.y^2 > n.x^2, in the x-z plane otherwise; t = n x s; both normalised."""
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    zero = np.zeros_like(nx)
    lean_y = sig.add(ny * ny > nx * nx, where)
    s = R.unit(np.where(lean_y[..., None], R.vec(zero, nz, -ny), R.vec(-nz, zero, nx)))
    t = R.unit(R.cross(n, s))
    return s * v[..., 0:1] + t * v[..., 1:2] + n * v[..., 2:3]


# ---- vertex 0: calcLightBounce{Point,Sun,Spot,Quad} (lbb_construction.compute:35-141) ---------------
def light_ray(L, u, dtype=np.float64):
    """The ray leaving light L (an _shaderef.light_setup) for the draws u (N, 4): position
    draws, then direction draws.  Returns o, d (normalised) and sig."""
    dt = dtype
    u = np.asarray(u, dt)
    a0, a1, b0, b1 = (u[:, i] for i in range(4))
    n_items = len(u)
    sig = R.Sig(n_items)
    one = np.ones((n_items, 1), dt)
    if L["kind"] == R.POINT:                                   # :35-58: a point of the sphere, hemisphere about its normal
        n = uniform_sphere(a0, a1, dt)
        o = L["pos"] + n * L["radius"]
        d = to_world(cosine_hemisphere(b0, b1, dt), n, sig)
    elif L["kind"] == R.SUN:                                   # :60-80: a far point, the light's direction
        pos = -L["dir"] + uniform_sphere(a0, a1, dt) * L["radius"]
        o = pos + R.unit(pos) * dt(1e16)
        d = L["dir"] * one
    elif L["kind"] == R.SPOT:                                  # :82-112: a disk point, the cone of `outer` degrees
        disc = cosine_hemisphere(a0, a1, dt)
        disc[:, 2] = 0
        axis = L["dir"] * one
        o = L["pos"] + to_world(disc * L["radius"], axis, sig)
        d = to_world(sample_angle(b0, b1, np.radians(L["outer"]), dt), axis, sig)
    else:                                                      # :114-141: a bilinear point, hemisphere about the direction
        v = L["vert"]
        x1 = v[0] + (v[1] - v[0]) * a0[:, None]
        x2 = v[3] + (v[2] - v[3]) * a0[:, None]
        o = x1 + (x2 - x1) * a1[:, None]
        d = to_world(cosine_hemisphere(b0, b1, dt), L["dir"] * one, sig)
    with np.errstate(invalid="ignore"):
        d = R.unit(d)
    s = np.zeros((n_items, 2), np.int8)
    a = sig.array()
    s[:, :a.shape[1]] = a
    return {"o": np.asarray(o, dt), "d": np.asarray(d, dt), "sig": s}


def carried_attenuation(L):
    """attenuation_linear / _quadratic as the light bounce carries them: point and quad lights only."""
    return (L["l"], L["q"]) if L["kind"] in (R.POINT, R.QUAD) else (0.0, 0.0)


def angular_attenuation(L, d, sig, dtype=np.float64):
    """angularAttenuation (inc_light.compute:207-237) for the direction d from the hit to the light
    point: the spot's linear ramp between inner and outer, the quad's cosine (negative from
    behind, kept as the GLSL has it), 1 otherwise."""
    dt = dtype
    if L["kind"] == R.SPOT:
        with np.errstate(invalid="ignore"):
            ang = np.degrees(np.arccos(R.dot(R.unit(-d), L["dir"])))
            x = (ang - L["inner"]) / (L["outer"] - L["inner"])
        sig.add(x <= 0)
        sig.add(x >= 1)
        return (1 - np.clip(x, 0, 1)).astype(dt)
    sig.add(np.zeros(len(d), bool))
    sig.add(np.zeros(len(d), bool))
    if L["kind"] == R.QUAD:
        return R.dot(R.unit(-d), L["dir"]).astype(dt)
    return np.ones(len(d), dt)


# ---- the scene as the steps and connections see it -------------------------------------------------
def cone_frames(sd, dtype=np.float64):
    """U, V, W of every world-space cone (Cylinder.cpp:17-25): V along the axis, U = V x (0, 1, 0)
    (x (0, 0, 1) for an axis within 1e-4 of +-y), W = U x V."""
    b = np.asarray(sd.cone_base_r0, dtype).reshape(-1, 4)[:, :3]
    a = np.asarray(sd.cone_apex_r1, dtype).reshape(-1, 4)[:, :3]
    v = R.unit(a - b)
    up = np.where((1 - np.abs(v[:, 1:2])) < 1e-4, np.array([0, 0, 1], dtype), np.array([0, 1, 0], dtype))
    u = R.unit(R.cross(v, up))
    w = R.unit(R.cross(u, v))
    return np.stack([u, v, w], axis=1)


class Geom:
    """A scenes.SceneData of world-space cones and plain triangles: brute-force hits, the surface
    at a hit and the BSDF of the object hit."""

    def __init__(self, sd):
        self.sd = sd
        self.nt = len(sd.tri_v)
        self.cs = G.cone_setup(sd) if len(sd.cone_base_r0) else None
        self.table = R.materials_table(sd)
        self.mat_of = np.concatenate([np.asarray(sd.tri_mat, np.int64), np.asarray(sd.cone_mat, np.int64)])
        self.frames = {dt: np.concatenate([np.zeros((self.nt, 3, 3), dt),
                                           cone_frames(sd, dt) if self.cs is not None else np.zeros((0, 3, 3), dt)])
                       for dt in (np.float64, np.float32)}
        self.lights = {dt: [R.light_setup(L, dt) for L in sd.lights] for dt in (np.float64, np.float32)}

    def hit(self, o, d):
        """Closest hit of float32 rays over every object, and whether it is decisive (_geomref's rule:
        the same object and t with radii x 0.9 and x 1.1).  obj -1: a miss."""
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        (tm, km), (t0, k0), (tp, kp) = G.brute_force_variants(self.sd, o, d)
        tol = G.tau(t0)
        with np.errstate(invalid="ignore"):
            same_t = (k0 < 0) | ((np.abs(tm - t0) <= tol) & (np.abs(tp - t0) <= tol))
        ok = (km == k0) & (kp == k0) & same_t
        return k0, ok

    def surface(self, obj, o, d, dt):
        """Hit distance and shading normal of ray (o, d) on object obj (>= 0)."""
        t, n = np.zeros(len(o), dt), np.zeros((len(o), 3), dt)
        tri = obj < self.nt
        if tri.any():
            n[tri], t[tri] = R.triangle_normal(self.sd.tri_v, self.sd.tri_n, obj[tri], o[tri], d[tri], dt, with_t=True)
        if (~tri).any():
            n[~tri], t[~tri] = R.cone_normal(self.cs, obj[~tri] - self.nt, o[~tri], d[~tri], dt)
        return t, n

    def material(self, obj):
        mat = self.mat_of[obj]
        return self.table["kind"][mat], {k: self.table[k][mat] for k in ("diffuse", "specular", "volume", "ior", "roughness")}

    def sample(self, obj, wi, n, sample, hair, dt):
        """BSDF::sample of each item's object; sig padded to SIG_W - 8 columns."""
        n_items = len(obj)
        kind, mat = self.material(obj)
        out = {"out": np.zeros((n_items, 3), dt), "pdf": np.zeros(n_items, dt), "f": np.zeros((n_items, 3), dt),
               "flags": np.zeros(n_items, np.int32), "sig": np.zeros((n_items, SIG_W - 8), np.int8)}
        for k in np.unique(kind):
            s = kind == k
            r = R.bsdf_sample(int(k), {key: v[s] for key, v in mat.items()}, self.frames[dt][obj[s]], wi[s], n[s],
                              sample[s], hair[s], np.zeros(int(s.sum()), np.int64), dt)
            for key in ("out", "pdf", "f", "flags"):
                out[key][s] = r[key]
            out["sig"][s, :r["sig"].shape[1]] = r["sig"]
        return out

    def evaluate(self, obj, wi, n, wo, dt):
        """BSDF::evaluateLight of each item's object: f (N, 3) and the same-side decision."""
        kind, mat = self.material(obj)
        f, sig = np.zeros((len(obj), 3), dt), np.zeros(len(obj), np.int8)
        for k in np.unique(kind):
            s = kind == k
            r = R.bsdf_eval(int(k), {"diffuse": mat["diffuse"][s]}, wi[s], n[s], wo[s], dt)
            f[s] = r["f"]
            if k in (R.LAMBERT, R.MARSCHNER, R.LAMBERT_TRANS):
                sig[s] = r["sig"][:, 0]
        return f, sig


# ---- one light-path step (traceLightRays + shadeLightRays, lbb_construction.compute:237-403) ---------
def step(geom, obj, o, d, ppos, phc, dist0, draws, al, aq, min_pdf, dtype=np.float64):
    """Vertex j from the state of vertex j - 1.  obj: the object the ray (o, d) hits (Geom.hit; -1: a
    miss, which ends the subpath), ppos / phc: position and hit colour of vertex j - 1, dist0: the
    path length up to the ray's origin, draws (N, 4): vertex_draws, al / aq: the attenuation the
    light carries.  Returns valid, pos, hc, the sampled direction out and sig."""
    dt = dtype
    o, d, ppos, phc, draws = (np.asarray(x, dt) for x in (o, d, ppos, phc, draws))
    dist0, al, aq = (np.asarray(x, dt) for x in (dist0, al, aq))
    n_items = len(o)
    res = {"valid": np.zeros(n_items, np.int32), "pos": np.zeros((n_items, 3), dt), "hc": np.zeros((n_items, 3), dt),
           "out": np.zeros((n_items, 3), dt), "sig": np.zeros((n_items, SIG_W), np.int8)}
    h = np.nonzero(np.asarray(obj) >= 0)[0]
    if not len(h):
        return res
    ob = np.asarray(obj)[h]
    sig = R.Sig(len(h))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dn = R.unit(d[h])                                      # the ray constructor normalises
        t, n = geom.surface(ob, o[h], dn, dt)
        pos = o[h] + dn * t[:, None]
        dist = dist0[h] + R.norm(pos - o[h])                   # :312: the length of the path so far
        att = 1 / ((1 + dist * al[h]) + dist * dist * aq[h])
        bs = geom.sample(ob, -dn, n, draws[h, 0:2], draws[h, 2:4], dt)   # in = -d; nothing at dot(in, n) == 0
        hc = phc[h] * bs["f"]
        # convertDensity (:280-299) with the previous vertex' position -- the light point for vertex 1,
        # where the GLSL reads an undefined triangle
        w = pos - ppos[h]
        ww = R.dot(w, w)
        flat = sig.add(ww == 0)
        pdf = np.where(flat, 0, bs["pdf"] * np.abs(R.dot(n, w / np.sqrt(ww)[:, None])))
        c = np.abs(R.dot(bs["out"], n)) * pdf
        sig.add(c <= 0)
        sig.add(c >= 1)
        hc = hc * np.clip(c, 0, 1)[:, None]
        emissive = sig.add((bs["flags"] & R.F_EMISSIVE) == R.F_EMISSIVE)
        black = sig.add(np.all(hc == 0, axis=1))
        thin = sig.add(pdf <= min_pdf)
        far = sig.add(att <= ATT_MIN)
    ok = ~(emissive | black | thin | far)
    res["valid"][h] = ok
    res["pos"][h] = np.where(ok[:, None], pos, 0)
    res["hc"][h] = np.where(ok[:, None], hc, 0)
    res["out"][h] = np.where(ok[:, None], bs["out"], 0)
    res["sig"][h, :7] = sig.array()
    res["sig"][h, 8:] = bs["sig"]
    return res


# ---- one hit connection (pt_shade.compute:150-199) ---------------------------------------------------
def connect(geom, obj, o, d, b, light, j, vert, bias, bounce_bias, dtype=np.float64):
    """The connection of the camera ray (o, d)'s hit on object obj (>= 0) at bounce b to the vertex
    record vert (N, 10; index j) of a subpath of light `light`: accepted, the connection ray o / d,
    tmax and the contribution cj = hc (colour |d . n| f(-ray, d)) / (j + 1 + b)."""
    dt = dtype
    o, d, vert = (np.asarray(x, dt) for x in (o, d, vert))
    b, light, j, obj = (np.asarray(x, np.int64) for x in (b, light, j, obj))
    n_items = len(o)
    sig = np.zeros((n_items, 4), np.int8)
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = R.unit(d)
        t, n = geom.surface(obj, o, dn, dt)
        loc = o + dn * t[:, None]
        pos, din, hc = vert[:, 1:4], vert[:, 4:7], vert[:, 7:10]
        lp = pos - din * dt(bounce_bias)                       # the vertex pulled back along its ray
        colour = np.zeros((n_items, 3), dt)
        for li in np.unique(light):
            s = light == li
            L = geom.lights[dt][li]
            sg = R.Sig(int(s.sum()))
            ang = angular_attenuation(L, (lp - loc)[s], sg, dt)
            first = (j[s] == 0)
            colour[s] = L["color"] * np.where(first, ang, 1)[:, None]
            sig[s, 0:2] = np.where(first[:, None], sg.array(), 0)
        so = loc + n * dt(bias)
        sd_ = R.unit(lp - loc)
        tmax = R.norm(lp - so)
        colour = colour * np.abs(R.dot(sd_, n))[:, None]
        f, same = geom.evaluate(obj, -dn, n, sd_, dt)
        sig[:, 2] = same
        cj = hc * (colour * f) / (j + 1 + b).astype(dt)[:, None]
    ok = vert[:, 0] != 0
    z = lambda a: np.where(ok.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(dt)
    return {"accepted": ok.astype(np.uint8), "o": z(so), "d": z(sd_), "tmax": z(tmax), "cj": z(cj), "sig": sig}


# ---- one image-plane connection (pt_shade.compute:17-97) ---------------------------------------------
def sensor_frame(cam, width, height, dt):
    """Sensor area |(H axis_y px) x (W axis_x px)| and the camera normal normalize(axis_y x axis_x)."""
    ax = np.array(list(cam.axis_x), dt) * dt(cam.pixel_size)
    ay = np.array(list(cam.axis_y), dt) * dt(cam.pixel_size)
    return R.norm(R.cross(ay * dt(height), ax * dt(width))), R.unit(R.cross(ay, ax))


def img_connect(cam, width, height, sensor, j, prev, cur, image_plane, bias, bounce_bias, dtype=np.float64):
    """The visibility ray from the sensor point to the target of record j and its term
    hc we / npdf / (j + 1), we = 1 / (a cos^4), npdf = t^2 / |cos|; we = 0 behind the sensor.
    image_plane 1, the GLSL as written (:38-44): the record's ray origin + bias * its direction,
    i.e. the light point for j <= 1 and vertex j - 1 nudged by bounce_bias + bias along the
    segment for j >= 2.  image_plane 2: vertex j itself, pulled back by bounce_bias."""
    dt = dtype
    sensor, prev, cur = (np.asarray(x, dt) for x in (sensor, prev, cur))
    j = np.asarray(j, np.int64)
    a, cn = sensor_frame(cam, width, height, dt)
    pos, din, hc = cur[:, 1:4], cur[:, 4:7], cur[:, 7:10]
    if image_plane == 1:
        before = np.where((j >= 1)[:, None], prev[:, 1:4], pos)
        org = np.where((j >= 2)[:, None], before + din * dt(bounce_bias), before)
        lp = org + din * dt(bias)
    else:
        lp = pos - din * dt(bounce_bias)
    sig = R.Sig(len(sensor))
    with np.errstate(invalid="ignore", divide="ignore"):
        dv = lp - sensor
        t = R.norm(dv)
        dirn = R.unit(dv)
        ct = R.dot(dirn, cn)
        behind = sig.add(ct <= 0)
        we = np.where(behind, 0, 1 / (a * ct * ct * ct * ct))
        npdf = t * t / np.abs(ct)
        cj = hc * we[:, None] / npdf[:, None] / (j + 1).astype(dt)[:, None]
    ok = cur[:, 0] != 0
    z = lambda x: np.where(ok.reshape((-1,) + (1,) * (x.ndim - 1)), x, 0).astype(dt)
    return {"accepted": ok.astype(np.uint8), "d": z(dirn), "t": z(t), "cj": z(cj), "sig": sig.array()}
