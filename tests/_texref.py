"""Reference for texture lookups, hit texcoords, textured material parameters and the
environment maps, in plain numpy and parametrised by dtype (float64: the truth;
float32: the same formulas at KIRK's own precision).

Written from KIRK's sources alone (paths relative to src/libraries/KIRK/Common):
  Texture::getColor        Texture.cpp:243-287
  Material::getFromParam   Material.cpp:15-23
  Cylinder::Cylinder       Cylinder.cpp:5-36      (the frame calcTcoord reads)
  Cylinder::calcTcoord     Cylinder.cpp:239-260
  Triangle::Triangle       Triangle.cpp:13-123    (the reordering of tca, tcb, tcc)
  Triangle::calcTcoord     Triangle.cpp:250-254
  Environment::getColor    Environment.cpp:91-133
not from the product's device.h and not from the oracle.

Every function returns its outputs, a branch signature `sig` (one row per item: every
data-dependent decision) and `stable`: False where a truncated or compared
intermediate lies so close to its threshold that float32 rounding -- or the band the
caller grants the coordinates -- could move it across.  An item is decisive when
`sig` is unchanged by the +-2 ulp jitters of its inputs and `stable` holds.

Where KIRK's behaviour is undefined the reference follows the clamp the product
documents and says so in `stable`: a texel index computed from a NaN product (an
infinite coordinate under a wrap mode other than CLAMP) is 0, and indices are clamped
into the image.
"""
import numpy as np

import _shaderef as R

EPS32 = 2.0 ** -24
ROUND_ULPS = 4          # float32 roundings between a coordinate and its texel product: x - floor(x), the pow
#                         rounded to float, the product with (w - 1); and one to spare
UV_BAND = 4 * 2.0 ** -23    # the cube / sphere map's uv in [0, 1]: a normalise, a quotient, (q + 1) / 2
FACE_ULPS = 4               # relative gap between the two largest |components| below which the face may flip
ENV_COLOR, ENV_CUBE, ENV_SPHERE = 0, 1, 2
PARAMS = ("diffuse", "specular", "volume", "emission", "roughness")


def texture(texels, wrap):
    t = np.asarray(texels, np.uint8)
    if t.ndim == 2:
        t = t[:, :, None]
    return {"data": t, "h": t.shape[0], "w": t.shape[1], "ch": t.shape[2], "wrap": int(wrap)}


def scene_textures(sd):
    return [texture(t, w) for t, w in sd.textures]


# ---- Texture::getColor ---------------------------------------------------------------------------
def _axis(x, size, mode, dt):
    """One coordinate: (texel index, side, rounding-stable).  side: -1 below 0, +1 above 1, 0 inside."""
    x = np.asarray(x, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        above, below = x > 1.0, x < 0.0
        frac = x - np.floor(x)                                   # glm::floor on a float: float arithmetic
        # glm::pow(float, unsigned char) is std::pow on doubles, assigned back to a float
        wrapped = np.power(frac.astype(np.float64), float(mode)).astype(dt)
        u = np.where(above | below, wrapped, x)
        p = u * dt(size - 1)
        # CLAMP's pow(frac, 0) is 1 whatever the fraction's rounding, and 1 (w - 1) is exact; any other
        # mode raises the fraction's own rounding (2^-24 absolute: -1e-8 - floorf(-1e-8) is 1.0f) to its power
        wide = ROUND_ULPS * 2 * EPS32 + np.where(frac > 0, mode * 2 * EPS32 / np.where(frac > 0, frac, 1), 0.0)
        rb = np.where(above | below, 0.0 if mode == 0 else wide, ROUND_ULPS * 2 * EPS32) * np.abs(p)
    idx = lambda q: np.clip(np.trunc(np.where(np.isnan(q), 0.0, q)), 0, size - 1).astype(np.int64)
    i = idx(p)
    with np.errstate(invalid="ignore"):
        stable = ~np.isnan(p) & (idx(p - rb) == i) & (idx(p + rb) == i)
    return i, above.astype(np.int64) - below.astype(np.int64), stable


def tex_color(tex, x, y, dtype=np.float64, bx=0.0, by=0.0):
    """Texture::getColor at (x, y) -> rgba (n, 4), sig (nan, side x, side y, texel x, texel y), stable.
    bx, by: absolute bands on the coordinates (the tolerance of the texcoord that feeds the lookup):
    `stable` also needs sides and texels unchanged at x -+ bx, y -+ by."""
    dt = dtype
    x, y = np.asarray(x, dt), np.asarray(y, dt)
    nan = np.isnan(x) | np.isnan(y)
    ix, sx, okx = _axis(x, tex["w"], tex["wrap"], dt)
    iy, sy, oky = _axis(y, tex["h"], tex["wrap"], dt)
    stable = okx & oky
    for c, b, size, i0, s0 in ((x, bx, tex["w"], ix, sx), (y, by, tex["h"], iy, sy)):
        b = np.broadcast_to(np.asarray(b, dt), c.shape)
        if np.any(b > 0):
            for cv in (c - b, c + b):
                i1, s1, ok1 = _axis(cv, size, tex["wrap"], dt)
                stable &= ok1 & (i1 == i0) & (s1 == s0)
    p = tex["data"][iy, ix].astype(dt) / dt(255.0)                # (n, ch)
    one = np.ones(len(x), dt)
    ch = tex["ch"]
    if ch == 1:
        rgba = np.stack([p[:, 0]] * 4, axis=1)                    # rrrr
    elif ch == 2:
        rgba = np.stack([p[:, 0], p[:, 0], p[:, 0], p[:, 1]], axis=1)     # rrr + the second channel
    elif ch == 3:
        rgba = np.stack([p[:, 0], p[:, 1], p[:, 2], one], axis=1)
    else:
        rgba = p[:, :4]
    rgba = np.where(nan[:, None], np.asarray([1, 0, 0, 1], dt), rgba)    # Color::RED
    z = np.zeros(len(x), np.int64)
    sig = np.stack([nan.astype(np.int64), np.where(nan, z, sx), np.where(nan, z, sy), np.where(nan, z, ix),
                    np.where(nan, z, iy)], axis=1)
    return {"rgba": rgba.astype(dt), "sig": sig, "stable": stable | nan}


def lookup(textures, tex, xy, dtype=np.float64, band=None):
    """tex_color over items of several textures: tex[i] indexes `textures`."""
    tex = np.asarray(tex)
    xy = np.asarray(xy, dtype)
    n = len(tex)
    out = {"rgba": np.zeros((n, 4), dtype), "sig": np.zeros((n, 5), np.int64), "stable": np.zeros(n, bool)}
    for t in np.unique(tex):
        s = tex == t
        b = (0.0, 0.0) if band is None else (band[s, 0], band[s, 1])
        r = tex_color(textures[t], xy[s, 0], xy[s, 1], dtype, *b)
        for k in out:
            out[k][s] = r[k]
    return out


# ---- Environment::getColor -----------------------------------------------------------------------
def _sign(x):
    return (0.0 < x).astype(x.dtype) - (x < 0.0).astype(x.dtype)      # glm::sign: 0 for 0 and for NaN


def env_color(env, d, dtype=np.float64):
    """env: {"type", "color", "tex": [textures]} -> rgb (n, 3), sig (face or -1, then tex_color's), stable."""
    dt = dtype
    d = np.asarray(d, dt)
    n = len(d)
    if env["type"] == ENV_COLOR:
        return {"rgb": np.broadcast_to(np.asarray(env["color"], dt)[:3], (n, 3)).copy(),
                "sig": np.zeros((n, 6), np.int64), "stable": np.ones(n, bool)}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        len2 = R.dot(d, d)
        dn = d * (dt(1.0) / np.sqrt(len2))[:, None]                    # glm::normalize: v * inversesqrt(dot(v, v))
        x, y, z = dn[:, 0], dn[:, 1], dn[:, 2]
        # a squared length below float32's normal range loses its bits there: not for the truth to judge
        stable = ~(len2 < 2.0 ** -100) & ~(len2 > 2.0 ** 120)
        if env["type"] == ENV_CUBE:
            ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
            mx = np.maximum(np.maximum(ax, ay), az)
            fx = mx == ax
            fy = ~fx & (mx == ay)
            fz = ~fx & ~fy
            side = np.where(fx, np.trunc(0 + 1.5 - 1.5 * _sign(x)),
                            np.where(fy, np.trunc(1 + 1.5 - 1.5 * _sign(y)), np.trunc(2 + 1.5 + 1.5 * _sign(z))))
            side = side.astype(np.int64)
            two = dt(2.0)
            u = np.where(fx, (z / x + 1) / two, np.where(fy, (x / ay + 1) / two, -(x / z + 1) / two))
            v = np.where(fx, (y / ax + 1) / two, np.where(fy, (z / y + 1) / two, (y / az + 1) / two))
            second = np.sort(np.stack([ax, ay, az], axis=1), axis=1)[:, 1]
            stable &= ~(second >= mx * (1 - FACE_ULPS * 2 * EPS32))
            face_tex = [env["tex"][k] for k in range(6)]
        else:
            if dt == np.float32:   # 2.0 * sqrt(x x + y y + (z + 1.0) (z + 1.0)): float products, the z term in double
                zz = z.astype(np.float64) + 1.0
                m = (2.0 * np.sqrt((x * x + y * y).astype(np.float64) + zz * zz)).astype(dt)
                u = ((x / m).astype(np.float64) + 0.5).astype(dt)
                v = ((y / m).astype(np.float64) + 0.5).astype(dt)
            else:
                m = 2.0 * np.sqrt(x * x + y * y + (z + 1.0) * (z + 1.0))
                u, v = x / m + 0.5, y / m + 0.5
            side = np.zeros(n, np.int64)
            face_tex = [env["tex"][0]]
    rgb = np.zeros((n, 3), dt)
    sig = np.zeros((n, 6), np.int64)
    sig[:, 0] = side
    for k in np.unique(side):
        s = side == k
        r = tex_color(face_tex[k], u[s], v[s], dt, UV_BAND, UV_BAND)
        rgb[s] = r["rgba"][:, :3]
        sig[s, 1:] = r["sig"]
        stable[s] &= r["stable"]
    return {"rgb": rgb, "sig": sig, "stable": stable}


# ---- the objects as their constructors leave them ---------------------------------------------------
def cone_setup(sd, dtype=np.float64):
    """Cylinder::Cylinder (Cylinder.cpp:5-36) for every cone: the transformed base point, the frame
    U V W (derived from the PRE-transform axis, then carried by the transposed inverse of the model
    matrix), the slope and the height -- both from the pre-transform points."""
    dt = dtype
    base = np.asarray(sd.cone_base_r0, dt)
    apex = np.asarray(sd.cone_apex_r1, dt)
    n = len(base)
    M = np.tile(np.eye(4, dtype=dt), (n, 1, 1))
    if len(sd.cone_models):
        models = np.asarray(sd.cone_models, dt).reshape(-1, 4, 4).transpose(0, 2, 1)     # stored column-major
        M = models[np.asarray(sd.cone_model, np.int64)]
    Mti = np.linalg.inv(M[:, :3, :3].astype(np.float64)).transpose(0, 2, 1).astype(dt)
    b, a = base[:, :3], apex[:, :3]
    v = a - b
    height = R.norm(v)
    v = v / height[:, None]
    up = np.where((1 - np.abs(v[:, 1:2])) < 1e-4, np.asarray([0, 0, 1], dt), np.asarray([0, 1, 0], dt))
    u = R.unit(R.cross(v, up))
    w = R.unit(R.cross(u, v))
    carry = lambda q: R.unit(np.einsum("nij,nj->ni", Mti, q))
    return {"base": np.einsum("nij,nj->ni", M[:, :3, :3], b) + M[:, :3, 3], "r0": base[:, 3], "u": carry(u),
            "v": carry(v), "w": carry(w), "slope": (base[:, 3] - apex[:, 3]) / height, "height": height}


def triangle_texcoords(sd, la, dtype=np.float64):
    """tca, tcb, tcc of every triangle after the constructor's reordering (Triangle.cpp:37-112): the
    vertices are ordered along the longest axis la of the triangle's box by six overlapping <= tests, the
    last one that holds wins, and the texcoords follow their vertices.  la: m_lA per triangle, from the
    pinned records (Oracle.tri_records; it is chosen from the float32 box, +- the ray epsilon)."""
    v = np.asarray(sd.tri_v, np.float64)
    uv = np.asarray(sd.uvs(), dtype)
    la = np.asarray(la, np.int64)
    rows = np.arange(len(v))
    a, b, c = (v[rows, j, la] for j in range(3))
    perm = np.tile(np.arange(3), (len(v), 1))
    for cond, p in (((a <= b) & (b <= c), (0, 1, 2)), ((b <= a) & (a <= c), (1, 0, 2)), ((a <= c) & (c <= b), (0, 2, 1)),
                    ((c <= a) & (a <= b), (2, 0, 1)), ((b <= c) & (c <= a), (1, 2, 0)), ((c <= b) & (b <= a), (2, 1, 0))):
        perm[cond] = p
    return np.take_along_axis(uv, perm[:, :, None], axis=1)


# ---- calcTcoord ----------------------------------------------------------------------------------
def texcoord(cs, ttc, n_tris, obj, o, d, t, bary, dtype=np.float64):
    """The texcoord of the hit (object obj[i], distance t[i], barycentrics bary[i]) of ray (o, d):
    -> tc (n, 2), sig (cone, qu < 0, clamp of tmp: -1 / 0 / +1, nan), stable.
    cs: cone_setup's arrays; ttc: triangle_texcoords'."""
    dt = dtype
    obj = np.asarray(obj, np.int64)
    o, d, t, bary = np.asarray(o, dt), np.asarray(d, dt), np.asarray(t, dt), np.asarray(bary, dt)
    n = len(obj)
    tc = np.zeros((n, 2), dt)
    sig = np.zeros((n, 4), np.int64)
    stable = np.ones(n, bool)
    cone = obj >= n_tris
    tri = (obj >= 0) & ~cone
    if tri.any():
        k = obj[tri]
        bu, bv = bary[tri, 0], bary[tri, 1]
        bx = (1 - bu) - bv                                           # m_barycentric_coord = (1 - u - v, u, v)
        tc[tri] = bx[:, None] * ttc[k, 0] + bu[:, None] * ttc[k, 1] + bv[:, None] * ttc[k, 2]
    if cone.any():
        c = obj[cone] - n_tris
        with np.errstate(invalid="ignore", divide="ignore"):
            dn = d[cone] * (dt(1.0) / np.sqrt(R.dot(d[cone], d[cone])))[:, None]    # KIRK::Ray normalises
            loc = o[cone] + dn * t[cone][:, None]
            Q = loc - cs["base"][c].astype(dt)
            qu, qv, qw = (R.dot(Q, cs[a][c].astype(dt)) for a in ("u", "v", "w"))
            r = cs["r0"][c].astype(dt) - cs["slope"][c].astype(dt) * qv
            tmp = qw / r
            lo, hi = tmp < -1.0, tmp > 1.0
            tmpc = np.where(lo, dt(-1.0), np.where(hi, dt(1.0), tmp))        # if / else if: NaN stays NaN
            ac = np.arccos(tmpc)
            neg = qu < 0
            phi = np.where(neg, dt(2.0) * dt(np.pi) - ac, ac)
            tc[cone, 0] = phi / dt(2.0) / dt(np.pi)
            tc[cone, 1] = qv / cs["height"][c].astype(dt)
            # float32 roundings of loc and Q: a few ulps of the magnitudes that were added
            scale = np.abs(o[cone]).max(axis=1) + np.abs(t[cone]) + np.abs(cs["base"][c]).max(axis=1)
            bq = ROUND_ULPS * 2 * EPS32 * scale
            btmp = bq / np.abs(r) * (1 + np.abs(tmp)) + ROUND_ULPS * 2 * EPS32 * np.abs(tmp)
            nan = np.isnan(tmp) | np.isnan(qu)
            st = (np.abs(qu) > bq) & (np.abs(np.abs(tmp) - 1) > btmp)
        sig[cone, 0] = 1
        sig[cone, 1] = neg
        sig[cone, 2] = hi.astype(np.int64) - lo.astype(np.int64)
        sig[cone, 3] = nan
        stable[cone] = st & ~nan
    return {"tc": tc, "sig": sig, "stable": stable}


# ---- Material::getFromParam ----------------------------------------------------------------------
def material_at(sd, textures, mat, tc, dtype=np.float64, band=None):
    """The five parameters of material mat[i] at texcoord tc[i]: textured colours take the texel's
    rgb, a textured roughness the length of its rgba (glm::length of a vec4); the others the
    material's values.  sig: tex_color's per parameter (zeros where not textured)."""
    dt = dtype
    mat = np.asarray(mat, np.int64)
    tc = np.asarray(tc, dt)
    n = len(mat)
    out = {k: np.zeros((n, 3), dt) for k in PARAMS[:4]}
    out["roughness"] = np.zeros(n, dt)
    sig = np.zeros((n, 25), np.int64)
    stable = np.ones(n, bool)
    mtex = np.full((len(sd.materials), 5), -1, np.int64)
    if sd.material_textures is not None:
        mtex[:len(sd.material_textures)] = sd.material_textures
    for m in np.unique(mat[mat >= 0]):
        s = mat == m
        M = sd.materials[m]
        for j, k in enumerate(PARAMS):
            if mtex[m, j] < 0:
                out[k][s] = np.asarray(getattr(M, k), dt) if j < 4 else dt(M.roughness)
                continue
            b = (0.0, 0.0) if band is None else (band[s, 0], band[s, 1])
            r = tex_color(textures[mtex[m, j]], tc[s, 0], tc[s, 1], dt, *b)
            c = r["rgba"]
            out[k][s] = c[:, :3] if j < 4 else np.sqrt(np.sum(c * c, axis=1))
            sig[s, 5 * j:5 * j + 5] = r["sig"]
            stable[s] &= r["stable"]
    out["sig"], out["stable"] = sig, stable
    return out


# ---- decisive items --------------------------------------------------------------------------------
def decisive(fn, inputs, outputs, seed=1234):
    """_shaderef.decisive with `stable`: fn in float64 on the inputs and on N_JITTER +-2 ulp jitters of
    them -> the unjittered result, the mask (sig unchanged by every jitter, stable on the inputs as
    given) and J, the spread of each output in `outputs` over the evaluations."""
    base, ok, J = R.decisive(fn, inputs, outputs, seed)
    return base, ok & base["stable"], J
