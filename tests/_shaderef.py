"""Float64 reference of KIRK's shading: BSDF sampling and evaluation, the surface
at a hit, light sampling and light intersection (tests/test_shading_truth.py).

Plain numpy over N items, written from KIRK's semantics (SURVEY.md and its
Appendix A, Bsdf.cpp / Light.cpp / Cylinder.cpp / Triangle.cpp read as a
specification) with libm-quality functions (numpy, scipy's J0); none of the
oracle's or the product's functions.  KIRK's quirks are the truth where they
are KIRK's:
  * Marschner's lobe shift and width are degrees used as radians (Bsdf.cpp:488-489,
    677, 698), d'Eon's are converted (:807-808);
  * Marschner hands the *angle* gamma_i to dialectricFresnel, which expects a
    cosine and clamps it to [-1, 1] (:713, 725; :143-171);
  * GlassBSDF / MilkGlassBSDF choose between refraction and reflection on
    sample.y (:338, 381);
  * the 3 f |cos theta_i| weighting lives in the shader, not here;
  * the TT / TRT paths of the two hair BSDFs are not part of this port (p = 0 is
    hard-coded, :669 / :969, and no BSDF ever sets the cylinder flags): an item
    that arrives with MATFLAG_CYLINDER_T/TR gets direction (0, 0, 1), f = 0 and
    everything else untouched, the port's documented answer (csrc/device.h).

Every function takes `dtype`.  float64 is the truth; the same code in float32
only calibrates the tolerance (how far float32 arithmetic alone strays).  Every
function also returns the *branch signature* of each item, `sig` (N, k): each
data-dependent decision taken.  `decisive()` re-runs a function on inputs
jittered by +-2 float32 ulps (16 seeded jitters, in float64): an item is
decisive when its signature never changes, and the spread of each output over
the jitters, J, is the output's conditioning with respect to its float32 inputs.
"""
import numpy as np

try:
    from scipy.special import j0 as _j0
except ImportError:                                   # the power series, to double precision for |x| < 30
    def _j0(x):
        x = np.asarray(x, np.float64)
        q = -(x * x) / 4.0
        term = np.ones_like(x)
        s = np.ones_like(x)
        for k in range(1, 120):
            term = term * q / (k * k)
            s = s + term
        return s

EPS32 = 2.0 ** -24
N_JITTER = 16
JITTER_ULPS = 2.0

F_TRANSPARENT, F_SPECULAR, F_EMISSIVE, F_CYL_T, F_CYL_TR = 1, 2, 4, 8, 16
(LAMBERT, SPEC_REFL, SPEC_TRANS, GLOSSY, GLASS, MILK_GLASS, LAMBERT_TRANS, EMISSION, TRANSPARENT, MARSCHNER,
 DEON) = range(11)
KIND_NAMES = ["lambert", "specular_reflection", "specular_transmission", "glossy", "glass", "milk_glass",
              "lambert_transmission", "emission", "transparent", "marschner", "deon"]
POINT, QUAD, SPOT, SUN = range(4)
LIGHT_NAMES = ["point", "quad", "spot", "sun"]
FLT_EPSILON = 2.0 ** -23


# ---- small vector algebra (keeps the dtype of its arguments) ---------------------------------
def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def vec(x, y, z):
    return np.stack(np.broadcast_arrays(x, y, z), axis=-1)


def cross(a, b):
    return vec(a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
               a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])


def norm(a):
    return np.sqrt(dot(a, a))


def unit(a):
    return a / norm(a)[..., None]


def rotate(v, axis, angle):
    """v turned by `angle` about `axis` (right-handed, Rodrigues)."""
    k = unit(axis)
    c, s = np.cos(angle)[..., None], np.sin(angle)[..., None]
    return v * c + cross(k, v) * s + k * (dot(k, v)[..., None] * (1 - c))


class Sig:
    """Collects the decisions of one call: add(cond, where) records cond for the
    items the decision applies to and 0 for the others."""

    def __init__(self, n):
        self.n = n
        self.cols = []

    def add(self, cond, where=None):
        c = np.broadcast_to(np.asarray(cond), (self.n,)).astype(np.int8)
        if where is not None:
            c = np.where(where, c, np.int8(0))
        self.cols.append(c)
        return cond

    def array(self):
        return np.stack(self.cols, axis=1) if self.cols else np.zeros((self.n, 0), np.int8)


# ---- BSDF helpers ------------------------------------------------------------------------------
def tangent_frame(v, n, sig, where=None):
    """Math::localToWorldNormal: v given in a frame (s, t, n) built around n; s lies in
    the y-z plane when n leans to y more than to x, in the x-z plane otherwise."""
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    zero = np.zeros_like(nx)
    lean_y = sig.add(ny * ny > nx * nx, where)
    s = unit(np.where(lean_y[..., None], vec(zero, nz, -ny), vec(-nz, zero, nx)))
    t = unit(cross(n, s))
    return s * v[..., 0:1] + t * v[..., 1:2] + n * v[..., 2:3]


def concentric_disc(u0, u1, sig, where=None):
    """Shirley's concentric map of the unit square to the unit disc (Bsdf.cpp:95-115)."""
    ox, oy = 2 * u0 - 1, 2 * u1 - 1
    centre = sig.add((ox == 0) & (oy == 0), where)
    wide = sig.add(np.abs(ox) > np.abs(oy), where)
    pi = np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(wide, ox, oy)
        th = np.where(wide, (pi / 4) * (oy / ox), pi / 2 - (pi / 4) * (ox / oy)).astype(u0.dtype)
    dx = np.where(centre, 0, r * np.cos(th))
    dy = np.where(centre, 0, r * np.sin(th))
    return dx, dy


def cosine_hemisphere(u0, u1, sig, where=None):
    dx, dy = concentric_disc(u0, u1, sig, where)
    return vec(dx, dy, np.sqrt(np.maximum(0, 1 - dx * dx - dy * dy)))


def cone_sample(u0, u1, max_angle):
    """sampleAngle (Bsdf.cpp:117-123): uniform in the cone of half angle max_angle about +z."""
    phi = (2 * np.pi) * u0
    ct = 1 - u1 * (1 - np.cos(max_angle))
    with np.errstate(invalid="ignore"):
        st = np.sqrt(1 - ct * ct)
    return vec(np.cos(phi) * st, np.sin(phi) * st, ct)


def fresnel(cos_theta, eta_i, eta_t, sig, where=None):
    """dialectricFresnel (Bsdf.cpp:143-171): unpolarised Fresnel reflectance; a cosine
    <= 0 swaps the media; 1 past the critical angle."""
    ci = np.clip(cos_theta, -1, 1)
    sig.add(cos_theta > 1, where)
    swap = sig.add(ci <= 0, where)
    eta_i, eta_t = np.where(swap, eta_t, eta_i), np.where(swap, eta_i, eta_t)
    ci = np.abs(ci)
    si = np.sqrt(np.maximum(0, 1 - ci * ci))
    with np.errstate(invalid="ignore", divide="ignore"):
        st = eta_i / eta_t * si
        total = sig.add(st >= 1, where)
        ct = np.sqrt(np.maximum(0, 1 - st * st))
        r_par = (eta_t * ci - eta_i * ct) / (eta_t * ci + eta_i * ct)
        r_perp = (eta_i * ci - eta_t * ct) / (eta_i * ci + eta_t * ct)
        return np.where(total, 1, (r_par * r_par + r_perp * r_perp) / 2)


def reflect(i, n):
    return i - n * (2 * dot(n, i))[..., None]


def refract(i, n, eta, sig, where=None):
    """glm::refract: the zero vector under total internal reflection."""
    d = dot(n, i)
    k = 1 - eta * eta * (1 - d * d)
    total = sig.add(~(k >= 0), where)
    with np.errstate(invalid="ignore"):
        r = i * eta[..., None] - n * (eta * d + np.sqrt(k))[..., None]
    return np.where(total[..., None], 0, r), total


def gauss_pdf(x, sd):
    return 1 / ((2 * np.pi) ** 0.5 * sd) * np.exp(-0.5 * (x / sd) ** 2)


def j0(x):
    """The hair lobes' Bessel step runs in double on every side (k_j0)."""
    return _j0(np.asarray(x, np.float64)).astype(np.asarray(x).dtype)


def materials_table(scene, dtype=np.float64):
    """The scene's materials as arrays indexed by material index."""
    m = scene.materials
    return {"kind": np.array([x.bsdf for x in m], np.int64),
            "diffuse": np.array([list(x.diffuse) for x in m], dtype), "specular": np.array([list(x.specular) for x in m], dtype),
            "volume": np.array([list(x.volume) for x in m], dtype), "ior": np.array([x.ior for x in m], dtype),
            "roughness": np.array([x.roughness for x in m], dtype)}


def _hair(kind, frame, ior, wi, n, hair, sig, dt):
    """The R lobe of MarschnerHairBSDF (Bsdf.cpp:465-489, 669-736) and DEonHairBSDF
    (:784-808, 969-1017).  Returns out, pdf, f (scalar), theta_i."""
    U, V, W = frame[:, 0], frame[:, 1], frame[:, 2]
    w = unit(wi)
    lift = 5 + 5 * hair[:, 0], 5 + 5 * hair[:, 1]            # [5, 10): KIRK draws both from one distribution
    if kind == DEON:
        alpha, beta = -np.radians(lift[0]), np.radians(lift[1])
    else:
        alpha, beta = -lift[0], lift[1]                      # degrees used as radians (KIRK's)
    facing = sig.add(dot(n, w) > 0)                          # faceforward(n, -w, n)
    nf = np.where(facing[..., None], n, -n)
    mirror = reflect(-w, nf)
    # vec4(d, 0) * glm::rotate(alpha, V): the row-vector product, i.e. the transpose R^T = a turn by -alpha
    out = rotate(mirror, V, -alpha)
    # the fibre's local space (x, y, z) = (V, U, W); theta measured from the y (= U) axis
    lin = vec(dot(wi, V), dot(wi, U), dot(wi, W))
    lout = vec(dot(out, V), dot(out, U), dot(out, W))
    theta_i = np.arctan2(np.hypot(lin[:, 0], lin[:, 2]), lin[:, 1])
    theta_r = np.arctan2(np.hypot(lout[:, 0], lout[:, 2]), lout[:, 1])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == MARSCHNER:
            theta_h, theta_d = (theta_r + theta_i) / 2, (theta_r - theta_i) / 2
            pdf = gauss_pdf(theta_h - alpha, beta)
            gamma = np.arccos(np.clip(dot(w, unit(n)), -1, 1))
            h = np.sin(gamma)
            dh_dphi = np.abs(-2 / np.sqrt(1 - h * h))        # Bsdf.cpp:715: infinite at grazing incidence
            x1 = np.sqrt(ior * ior - np.sin(gamma) ** 2)
            eta1 = x1 / np.cos(gamma)                        # Bravais indices
            eta2 = ior * ior * np.cos(gamma) / x1
            F = fresnel(gamma, eta1, eta2, sig)              # the angle where a cosine is expected (KIRK's)
            f = pdf * (0.5 * F * dh_dphi) / np.cos(theta_d) ** 2
        else:
            v = beta * beta
            csch = 1 / np.sinh(np.radians(1 / v))
            e = np.exp(np.sin(-theta_i) * np.sin(theta_r) / np.degrees(v))
            bes = j0(np.cos(-theta_i) * np.cos(theta_r) / np.degrees(v))
            pdf = csch / (2 * v) * e * bes
            phi_i = np.arctan2(lin[:, 0], lin[:, 1])
            phi_r = np.arctan2(lout[:, 0], lout[:, 1])
            d_r = 0.25 * np.abs(np.cos(phi_r - phi_i / 2))
            half = 0.5 * np.arccos(dot(w, unit(out)))
            F = fresnel(half, np.ones_like(ior), ior, sig)
            f = pdf * (0.5 * F * d_r)
    return out.astype(dt), pdf.astype(dt), f.astype(dt), theta_i.astype(dt)


def bsdf_sample(kind, mat, frame, wi, n, sample, hair, flags_in, dtype=np.float64):
    """BSDF::sample (Bsdf.cpp:179-184) of one BSDF kind on N items.

    mat: per-item material arrays (diffuse, specular, volume (N, 3), ior, roughness (N)),
    frame: (N, 3, 3) the object's U, V, W; wi: ray_in, n: normal, sample (N, 2), hair
    (N, 2) the two hair draws, flags_in (N).  Returns out, pdf, f, sample, flags, valid, sig.
    Outputs the BSDF leaves unwritten are the inputs (sample, flags) or 0 (pdf, out)."""
    dt = dtype
    wi, n, sample, hair, frame = (np.asarray(x, dt) for x in (wi, n, sample, hair, frame))
    diffuse, specular, volume = (np.asarray(mat[k], dt) for k in ("diffuse", "specular", "volume"))
    ior, rough = np.asarray(mat["ior"], dt), np.asarray(mat["roughness"], dt)
    flags_in = np.asarray(flags_in, np.int64)
    N = len(wi)
    sig = Sig(N)
    one, zero3 = np.ones(N, dt), np.zeros((N, 3), dt)
    cos_in = dot(wi, n)
    early = sig.add(cos_in == 0)                               # Bsdf.cpp:181: no sample at exactly grazing incidence
    entering = sig.add(cos_in > 0)
    nf = np.where(entering[..., None], n, -n)                  # faceforward(n, -in, n)
    u0, u1 = sample[:, 0], sample[:, 1]
    s_out = sample.copy()
    pi = np.pi
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind in (LAMBERT, LAMBERT_TRANS):
            h = cosine_hemisphere(u0, u1, sig)
            same_side = entering if kind == LAMBERT else ~entering
            out = tangent_frame(np.where(same_side[..., None], h, -h), n, sig)
            pdf = np.abs(dot(out, n)) / pi
            black = sig.add(pdf == 0)
            colour = diffuse if kind == LAMBERT else volume
            f = np.where(black[..., None], 0, colour / pi)
            flags = np.full(N, 0 if kind == LAMBERT else F_TRANSPARENT)
        elif kind == SPEC_REFL:
            out = reflect(-wi, nf)
            pdf = one
            f = specular / np.abs(dot(out, n))[..., None]
            flags = flags_in | F_SPECULAR
        elif kind == GLOSSY:
            lobe = cone_sample(u0, u1, rough * pi)             # (180 - (1 - roughness) 180) degrees
            mirror = reflect(-wi, nf)
            out = tangent_frame(lobe, mirror, sig)
            below = sig.add(dot(out, nf) < 0)
            out = np.where(below[..., None], tangent_frame(lobe * np.array([-1, -1, 1], dt), mirror, Sig(N)), out)
            pdf = one
            f = specular / np.abs(dot(out, n))[..., None]
            flags = flags_in | F_SPECULAR
        elif kind in (SPEC_TRANS, GLASS, MILK_GLASS):
            eta_i = np.where(entering, one, ior)
            eta_t = np.where(entering, ior, one)
            w = unit(wi)
            # SpecularTransmissionBSDF takes the cosine of the raw ray_in (:265), the other two normalise it
            F = fresnel(np.abs(dot(wi if kind == SPEC_TRANS else w, n)), eta_i, eta_t, sig)
            bent, total = refract(-w, nf, eta_i / eta_t, sig)
            through = ~total & ~np.isnan(bent[:, 0]) & ~np.all(bent == 0, axis=1)
            if kind != SPEC_TRANS:
                through = through & sig.add(u1 > F, ~total)     # the decision is on sample.y (KIRK's)
            carried = volume * ((1 - F) * (eta_i * eta_i) / (eta_t * eta_t))[..., None]
            if kind == SPEC_TRANS:
                out = bent
                pdf = one
                f = np.where(through[..., None], carried / np.abs(dot(out, n))[..., None], 0)
            else:
                if kind == GLASS:
                    out = np.where(through[..., None], bent, reflect(-w, nf))
                else:
                    lobe = cone_sample(u0, u1, rough * pi)
                    flipped = lobe * np.array([-1, -1, 1], dt)
                    o_t = tangent_frame(lobe, bent, sig, through)
                    wrong_t = sig.add(dot(o_t, nf) > 0, through)
                    o_t = np.where(wrong_t[..., None], tangent_frame(flipped, bent, Sig(N)), o_t)
                    mirror = reflect(-wi, nf)
                    o_r = tangent_frame(lobe, mirror, sig, ~through)
                    wrong_r = sig.add(dot(o_r, nf) < 0, ~through)
                    o_r = np.where(wrong_r[..., None], tangent_frame(flipped, mirror, Sig(N)), o_r)
                    out = np.where(through[..., None], o_t, o_r)
                pdf = np.where(through, 1 - F, F)
                f = np.where(through[..., None], carried, specular * F[..., None]) / np.abs(dot(out, n))[..., None]
            flags = flags_in | F_SPECULAR | np.where(through, F_TRANSPARENT, 0)
        elif kind == EMISSION:
            out, pdf, f, flags = zero3, one, np.ones((N, 3), dt), np.full(N, F_EMISSIVE)
        elif kind == TRANSPARENT:
            out = -wi
            pdf = one
            f = volume / np.abs(dot(out, n))[..., None]
            flags = np.full(N, F_TRANSPARENT | F_SPECULAR)
        elif kind in (MARSCHNER, DEON):
            out, pdf, fs, theta_i = _hair(kind, frame, ior, wi, n, hair, sig, dt)
            f = np.repeat(fs[:, None], 3, axis=1)
            flags = np.full(N, F_SPECULAR)
            if kind == MARSCHNER:                              # sample.x carries theta_i to the shader (:695)
                s_out = np.stack([theta_i, np.zeros(N, dt)], axis=1)
            inside = (flags_in & (F_CYL_T | F_CYL_TR)) != 0    # TT / TRT: not part of the port (see the module docstring)
            up = np.array([0, 0, 1], dt)
            out = np.where(inside[..., None], up, out)
            f = np.where(inside[..., None], 0, f)
            pdf = np.where(inside, 0, pdf)
            flags = np.where(inside, flags_in, flags)
            s_out = np.where(inside[..., None], sample, s_out)
        else:
            raise ValueError(kind)
    up = np.array([0, 0, 1], dt)
    res = {"out": np.where(early[..., None], up, out).astype(dt), "pdf": np.where(early, 0, pdf).astype(dt),
           "f": np.where(early[..., None], 0, f).astype(dt), "sample": np.where(early[..., None], sample, s_out).astype(dt),
           "flags": np.where(early, flags_in, flags).astype(np.int32), "valid": (~early).astype(np.int32)}
    s = sig.array()
    s[early, 2:] = 0                                           # nothing after the exit is a decision of the item
    res["sig"] = s
    return res


def bsdf_eval(kind, mat, wi, n, wo, dtype=np.float64):
    """BSDF::evaluateLight (Bsdf.cpp:197-202, 310-318, 771-776; every other kind returns 0)."""
    dt = dtype
    wi, n, wo = (np.asarray(x, dt) for x in (wi, n, wo))
    diffuse = np.asarray(mat["diffuse"], dt)
    sig = Sig(len(wi))
    same = sig.add(dot(wi, n) * dot(wo, n) > 0)
    if kind in (LAMBERT, MARSCHNER):
        f = np.where(same[..., None], diffuse / np.pi, 0)
    elif kind == LAMBERT_TRANS:
        f = np.where(same[..., None], 0, diffuse / np.pi)
    else:
        f = np.zeros_like(wi)
    return {"f": f.astype(dt), "sig": sig.array()}


# ---- lights ------------------------------------------------------------------------------------
def light_setup(L, dtype=np.float64):
    """The state KIRK's light constructors and Light::transform derive (Light.h,
    Light.cpp:216-220, 263-276), from the constructor arguments of one light."""
    dt = dtype
    a = lambda x: np.array(list(x), dt)
    s = {"kind": int(L.kind), "color": a(L.color), "pos": a(L.position), "radius": dt(L.radius),
         "c": dt(L.att_const), "l": dt(L.att_lin), "q": dt(L.att_quad)}
    with np.errstate(invalid="ignore", divide="ignore"):
        s["dir"] = unit(a(L.direction))
    if s["kind"] == SPOT:
        outer, inner = dt(L.outer_angle), dt(L.inner_angle)
        s["outer"] = outer
        s["inner"] = outer if (inner < 0 or inner > outer) else inner
    if s["kind"] == QUAD:
        e1, e2 = plane_base(s["dir"])
        hx, hy = e1 * (dt(L.size[0]) / 2), e2 * (dt(L.size[1]) / 2)
        s["vert"] = np.stack([s["pos"] - hx - hy, s["pos"] + hx - hy, s["pos"] + hx + hy, s["pos"] - hx + hy])
    return s


def plane_base(n):
    """Light::orthonormalBase (Light.cpp:112-118): two unit vectors spanning the plane of normal n."""
    if abs(n[0]) > abs(n[1]):
        s = np.array([-n[2], 0, n[0]], n.dtype) / np.sqrt(n[0] * n[0] + n[2] * n[2])
    else:
        s = np.array([0, n[2], -n[1]], n.dtype) / np.sqrt(n[1] * n[1] + n[2] * n[2])
    return s, np.cross(n, s).astype(n.dtype)


def sphere_point(u0, u1):
    phi = (2 * np.pi) * u0
    ct = 2 * u1 - 1
    st = np.sqrt(np.maximum(0, 1 - ct * ct))
    return vec(st * np.cos(phi), st * np.sin(phi), ct)


def _distance_attenuation(L, d):
    if L["c"] > 0 or (L["l"] > 0 and L["q"] > 0):          # Light.h:70-73
        return 1 / (L["c"] + L["l"] * d + L["q"] * d * d)
    return np.ones_like(d)


def _clamp01(x, sig):
    sig.add(x <= 0)
    sig.add(x >= 1)
    return np.clip(x, 0, 1)


def light_dir(L, p, u, dtype=np.float64):
    """calcLightdir with randomize = true (Light.cpp:127-145, 278-296, 327-343, 463-475):
    the shadow ray from p towards a sampled point of the light, and the attenuation."""
    dt = dtype
    p, u = np.asarray(p, dt), np.asarray(u, dt)
    sig = Sig(len(p))
    u0, u1 = u[:, 0], u[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if L["kind"] == POINT:
            to_centre = unit(L["pos"] - p)
            s = sphere_point(u0, u1)
            target = L["pos"] + s * L["radius"]
            facing = _clamp01(dot(s, -to_centre), sig)
            ld = target - p
            att = facing * _distance_attenuation(L, norm(ld))
        elif L["kind"] == QUAD:
            v = L["vert"]
            a = v[0] + (v[1] - v[0]) * u0[:, None]
            b = v[3] + (v[2] - v[3]) * u0[:, None]
            ld = a + (b - a) * u1[:, None] - p
            facing = _clamp01(dot(unit(-ld), L["dir"]), sig)
            att = facing * _distance_attenuation(L, norm(ld))
        elif L["kind"] == SPOT:
            r, th = np.sqrt(u0), (2 * np.pi) * u1
            e1, e2 = plane_base(L["dir"])
            on_disc = (e1 * (L["radius"] * r * np.cos(th))[:, None]) + (e2 * (L["radius"] * r * np.sin(th))[:, None])
            ld = (L["pos"] + on_disc) - p
            ang = np.degrees(np.arccos(dot(unit(-ld), L["dir"])))
            fall = 1 - _clamp01((ang - L["inner"]) / (L["outer"] - L["inner"]), sig)
            att = fall ** 4 * _distance_attenuation(L, norm(ld))
        else:
            far = unit(sphere_point(u0, u1) * L["radius"] - L["dir"]) * dt(1e16)
            ld = far - p
            att = np.ones(len(p), dt)
        d = unit(ld)
    return {"o": p.astype(dt), "d": d.astype(dt), "att": att.astype(dt), "sig": sig.array()}


def _triangle(o, d, a, b, c, sig, where):
    """Light::intersectTriangle (Light.cpp:13-64): Moeller-Trumbore, |det| >= FLT_EPSILON, t > FLT_EPSILON."""
    e1, e2 = b - a, c - a
    pv = cross(d, e2)
    det = dot(pv, e1)
    flat = sig.add(np.abs(det) < FLT_EPSILON, where)
    with np.errstate(invalid="ignore", divide="ignore"):
        tv = o - a
        uu = dot(tv, pv) / det
        q = cross(tv, e1)
        vv = dot(d, q) / det
        t = dot(e2, q) / det
    ok = ~flat
    ok = ok & ~sig.add((uu < 0) | (uu > 1), where & ok)
    ok = ok & ~sig.add((vv < 0) | (uu + vv > 1), where & ok)
    ok = ok & sig.add(t > FLT_EPSILON, where & ok)
    return ok, t


def light_isect(L, o, d, dtype=np.float64):
    """isIntersection (Light.cpp:169-189, 227-232, 367-428, 497-501) and
    sampleLightSource (:196-199, 234-239, 436-440, 508-511) for rays (o, unit(d))."""
    dt = dtype
    o, d = np.asarray(o, dt), unit(np.asarray(d, dt))
    N = len(o)
    sig = Sig(N)
    every = np.ones(N, bool)
    hit, t = np.zeros(N, bool), np.zeros(N, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        if L["kind"] == POINT:
            if L["radius"] * L["radius"] != 0:
                oc = o - L["pos"]
                leaving = sig.add(dot(d, oc) > 0)                       # Appendix A.3, Light.cpp:174-175
                a, b, c = dot(d, d), 2 * dot(d, oc), dot(oc, oc) - L["radius"] ** 2
                disc = b * b - 4 * a * c
                miss = sig.add(disc < 0, ~leaving)
                hit = ~leaving & ~miss
                t = -(b + np.sqrt(disc)) / (2 * a)                      # the near root, whatever its sign
        elif L["kind"] == QUAD:
            v = L["vert"]
            h1, t1 = _triangle(o, d, v[0], v[1], v[3], sig, every)
            h2, t2 = _triangle(o, d, v[2], v[3], v[1], sig, ~h1)
            hit, t = h1 | h2, np.where(h1, t1, t2)
        elif L["kind"] == SPOT:
            if L["radius"] != 0:
                e1, e2 = plane_base(L["dir"])
                nrm = np.cross(e1, e2)
                denom = dot(d, nrm)
                flat = sig.add(np.abs(denom) < FLT_EPSILON)
                t = dot(L["pos"] - o, nrm) / denom
                q = o + d * t[:, None] - L["pos"]
                outside = sig.add(dot(q, e1) ** 2 + dot(q, e2) ** 2 > L["radius"] ** 2, ~flat)
                hit = ~flat & ~outside
                hit = hit & sig.add(t > FLT_EPSILON, hit)
        cdiv = L["c"] if L["c"] > 0 else dt(1)
        if L["kind"] == POINT:
            emit = np.broadcast_to(L["color"] / np.pi / cdiv, (N, 3))
        elif L["kind"] in (QUAD, SPOT):
            front = ~sig.add(dot(unit(-d), L["dir"]) < 0)
            emit = np.where(front[:, None], L["color"] / np.pi / cdiv, 0)
        else:
            emit = np.broadcast_to(L["color"], (N, 3))
    return {"hit": hit.astype(np.uint8), "t": np.where(hit, t, 0).astype(dt), "emit": np.asarray(emit, dt),
            "sig": sig.array()}


# ---- the surface at a hit ------------------------------------------------------------------------
def cone_normal(cs, c, o, d, dtype=np.float64):
    """Outward unit normal of cone c (indices into _geomref.cone_setup's arrays cs) at
    the first hit of ray (o, d): the normalised gradient of the frustum's implicit
    function |p_perp|^2 - (r0 - s y)^2 at the hit point.  Also returns that hit's t."""
    import _geomref as G
    dt = dtype
    base, axis, h, r0, r1 = (np.asarray(x[c], dt) for x in cs)
    o, d = np.asarray(o, dt), np.asarray(d, dt)
    lo, hi, ok_lo, ok_hi = G.cone_roots(base, axis, h, r0, r1, o, d)
    t = np.where(ok_lo, lo, hi)
    p = o + d * t[:, None] - base
    y = dot(p, axis)
    s = (r0 - r1) / h
    grad = (p - axis * y[:, None]) + axis * (s * (r0 - s * y))[:, None]
    with np.errstate(invalid="ignore"):
        return unit(grad).astype(dt), t.astype(dt)


def triangle_normal(tri_v, tri_n, k, o, d, dtype=np.float64, with_t=False):
    """Shading normal of triangle k at the hit of ray (o, d): the barycentric blend of
    its unit vertex normals (Triangle.cpp:244-248), normalised.  with_t: also the hit
    distance against the same (KIRK's) edges."""
    dt = dtype
    v, vn = np.asarray(tri_v, dt)[k].copy(), np.asarray(tri_n, dt)[k].copy()
    o, d = np.asarray(o, dt), np.asarray(d, dt)
    # KIRK's own (Triangle.cpp:13-123): the constructor orders the vertices along the longest axis of
    # the triangle's box (six overlapping <= tests, the last one that holds wins) and replaces an
    # edge's component along that axis by 1e-4 where it is exactly 0.  Its barycentrics are taken
    # against those edges, so for a triangle with two vertices level on that axis (every second
    # triangle of a grid mesh, and of a fibre tube) they differ from the geometric ones by up to
    # 1e-4 / edge length.  The truth follows it.
    ext = v.max(axis=1) - v.min(axis=1)                      # + 2 RAY_EPS on every axis: no effect on the order
    la = np.where(ext[:, 2] > np.maximum(ext[:, 0], ext[:, 1]), 2, np.where(ext[:, 1] > ext[:, 0], 1, 0))
    rows = np.arange(len(v))
    ca, cb, cc = (v[rows, j, la] for j in range(3))
    perm = np.tile(np.arange(3), (len(v), 1))
    for cond, p in (((ca <= cb) & (cb <= cc), (0, 1, 2)), ((cb <= ca) & (ca <= cc), (1, 0, 2)),
                    ((ca <= cc) & (cc <= cb), (0, 2, 1)), ((cc <= ca) & (ca <= cb), (2, 0, 1)),
                    ((cb <= cc) & (cc <= ca), (1, 2, 0)), ((cc <= cb) & (cb <= ca), (2, 1, 0))):
        perm[cond] = p
    v = np.take_along_axis(v, perm[:, :, None], axis=1)
    vn = np.take_along_axis(vn, perm[:, :, None], axis=1)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    for e in (e1, e2):
        level = e[rows, la] == 0
        e[rows[level], la[level]] = 1e-4
    pv = cross(d, e2)
    with np.errstate(invalid="ignore", divide="ignore"):
        det = dot(pv, e1)
        tv = o - v[:, 0]
        b1 = dot(tv, pv) / det
        b2 = dot(d, cross(tv, e1)) / det
        blend = unit(vn[:, 0]) * (1 - b1 - b2)[:, None] + unit(vn[:, 1]) * b1[:, None] + unit(vn[:, 2]) * b2[:, None]
        if with_t:
            return unit(blend).astype(dt), (dot(e2, cross(tv, e1)) / det).astype(dt)
        return unit(blend).astype(dt)


# ---- decisive items, conditioning, comparison ----------------------------------------------------
def _jitter(x, rng):
    x32 = np.asarray(x, np.float32)
    ulp = np.spacing(np.abs(x32)).astype(np.float64)
    return x32.astype(np.float64) + rng.uniform(-JITTER_ULPS, JITTER_ULPS, x32.shape) * ulp


def decisive(fn, inputs, outputs, seed=1234):
    """fn(**inputs) in float64 on the inputs as given and on N_JITTER seeded jitters of
    them (every float input moved by up to +-JITTER_ULPS float32 ulps).  Returns the
    unjittered result, the decisive mask (signature unchanged by every jitter) and J:
    per output its spread (max - min over the 1 + N_JITTER evaluations)."""
    base = fn(**{k: np.asarray(v, np.float32).astype(np.float64) for k, v in inputs.items()})
    rng = np.random.default_rng(seed)
    ok = np.ones(len(base["sig"]), bool)
    lo = {k: np.asarray(base[k], np.float64).copy() for k in outputs}
    hi = {k: np.asarray(base[k], np.float64).copy() for k in outputs}
    for _ in range(N_JITTER):
        r = fn(**{k: _jitter(v, rng) for k, v in inputs.items()})
        ok &= np.all(r["sig"] == base["sig"], axis=1)
        for k in outputs:
            with np.errstate(invalid="ignore"):
                lo[k] = np.fmin(lo[k], r[k])
                hi[k] = np.fmax(hi[k], r[k])
    with np.errstate(invalid="ignore"):
        J = {k: hi[k] - lo[k] for k in outputs}
    return base, ok, J


def ratio(got, truth, J):
    """|got - truth| / (J + eps32 |truth|) per item; a vector output is measured by its
    largest component on both sides (a direction's small component carries the
    rounding of its large ones).  0 where got == truth."""
    got, truth, J = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.asarray(J, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - truth)
    if truth.ndim > 1:
        axes = tuple(range(1, truth.ndim))
        err, J, scale = err.max(axis=axes), J.max(axis=axes), np.abs(truth).max(axis=axes)
    else:
        scale = np.abs(truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = err / (J + EPS32 * scale)
    same = np.all(got == truth, axis=tuple(range(1, truth.ndim))) if truth.ndim > 1 else got == truth
    return np.where(same, 0.0, r)
