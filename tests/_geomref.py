"""Float64 brute-force ray/scene intersection: the geometric truth for the
closest-hit and any-hit queries (tests/test_geometry_truth.py).

Pure numpy, no BVH, none of the oracle's or the product's code or formulas:
every ray is tested against every triangle and every cone frustum of a
scenes.SceneData (world-space cones only; scenes with model transforms are
not covered).  Object ids are KIRK's: triangles first, then cones.

A ray is trusted only where the answer does not hang on float32 rounding: the
geometry is also evaluated a little thinner and a little fatter (grow -1 / +1),
and a ray is *decisive* when all three variants agree.  The margins:
  * radii x (1 + 0.1 grow): KIRK's float32 quadratic loses about eps32 t^2 / r^2
    relative to the radius (c = Px^2 + Pz^2 - r^2 cancels), 0.06 at t = 1 for
    the thinnest tip r = 0.001 of these scenes;
  * axial window widened by 0.02 h grow at each end, barycentric tests by
    1e-3 grow: KIRK's triangle ctor replaces a zero edge component along the
    longest axis by 1e-4 (a crack of about 1e-4 along axis-aligned edges), and
    the cone's window test is a float32 dot product v.Q;
  * t within TAU_REL max(1, t), the tolerance of
    test_oracle_kat.test_tilted_cone_matches_analytic.
"""
import numpy as np

RAY_EPS = 1e-4      # KIRK's cRayEpsilon: the smallest accepted cone root
TAU_REL = 1e-3      # |t - t64| <= TAU_REL * max(1, t64)
R_MARGIN = 0.1      # radii x (1 + R_MARGIN * grow)
Y_MARGIN = 0.02     # axial window widened by Y_MARGIN * h * grow at each end
UV_MARGIN = 1e-3    # barycentric tests widened by UV_MARGIN * grow
_CHUNK = 256        # rays per block: 256 x 20k objects x 8 B = 40 MB per temporary


def tau(t):
    t = np.asarray(t, np.float64)
    return TAU_REL * np.maximum(1.0, np.where(np.isfinite(t), t, 1.0))


# ---- cones ---------------------------------------------------------------------------------
def cone_setup(scene):
    b = np.asarray(scene.cone_base_r0, np.float64).reshape(-1, 4)
    a = np.asarray(scene.cone_apex_r1, np.float64).reshape(-1, 4)
    if len(np.asarray(scene.cone_model).reshape(-1)):
        raise ValueError("_geomref covers world-space cones only")
    ax = a[:, :3] - b[:, :3]
    h = np.linalg.norm(ax, axis=1)
    return b[:, :3], ax / h[:, None], h, b[:, 3], a[:, 3]


def cone_roots(base, axis, h, r0, r1, orig, d, grow=0):
    """Both roots of ray x cone, elementwise over broadcastable (..., 3) / (...) arrays.

    The frustum's radius is r(y) = r0 - s y, s = (r0 - r1) / h, y the axial
    coordinate.  With w = orig - base split into wy (axial) and w_perp, d alike:
    |w_perp + t d_perp| = r(wy + t dy)  <=>  A t^2 + 2 B t + C = 0.
    Returns (t_lo, t_hi, ok_lo, ok_hi): the roots in ascending order and whether
    each is a hit (t >= RAY_EPS and y inside the axial window)."""
    g = 1.0 + R_MARGIN * grow
    r0, r1 = r0 * g, r1 * g
    s = (r0 - r1) / h
    w = orig - base
    wy = np.sum(w * axis, axis=-1)
    dy = np.sum(d * axis, axis=-1)
    wp = w - wy[..., None] * axis
    dp = d - dy[..., None] * axis
    rr = r0 - s * wy
    A = np.sum(dp * dp, axis=-1) - s * s * dy * dy
    B = np.sum(wp * dp, axis=-1) + s * dy * rr
    C = np.sum(wp * wp, axis=-1) - rr * rr
    return _solve(A, B, C, wy, dy, h, grow)


def _solve(A, B, C, wy, dy, h, grow):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sq = np.sqrt(B * B - A * C)          # NaN where the ray misses the infinite cone
        ta, tb = (-B - sq) / A, (-B + sq) / A
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)   # A < 0: a ray steeper than the cone's side
        m = Y_MARGIN * grow * h
        ok = []
        for t in (lo, hi):
            y = wy + t * dy
            ok.append((t >= RAY_EPS) & (y >= -m) & (y <= h + m))   # NaN compares false
    return lo, hi, ok[0], ok[1]


def _cones_block(cs, o, d, grows):
    """Closest cone hit of each ray of a block, for each grow: [(t, index)], inf /
    -1 on a miss.  cone_roots' coefficients for every (ray, cone) pair through
    matrix products; the roots only for the few pairs with a real one."""
    base, axis, h, r0, r1 = cs
    wy = o @ axis.T - np.sum(base * axis, axis=1)
    dy = d @ axis.T
    wp2 = (np.sum(o * o, axis=1)[:, None] - 2.0 * (o @ base.T) + np.sum(base * base, axis=1)) - wy * wy   # |w_perp|^2
    wpdp = (np.sum(o * d, axis=1)[:, None] - d @ base.T) - wy * dy                                      # w_perp . d_perp
    dp2 = np.sum(d * d, axis=1)[:, None] - dy * dy                                                      # |d_perp|^2
    dy2 = dy * dy
    out = []
    for grow in grows:
        g = 1.0 + R_MARGIN * grow
        s = (r0 - r1) * g / h
        rr = r0 * g - s * wy
        A = dp2 - (s * s) * dy2
        B = wpdp + s * dy * rr
        C = wp2 - rr * rr
        ri, ci = np.nonzero(B * B - A * C >= 0.0)
        lo, hi, ok_lo, ok_hi = _solve(A[ri, ci], B[ri, ci], C[ri, ci], wy[ri, ci], dy[ri, ci], h[ci], grow)
        t = np.where(ok_lo, lo, hi)
        hit = ok_lo | ok_hi
        out.append(_closest_per_ray(len(o), ri[hit], ci[hit], t[hit]))
    return out


# ---- triangles -----------------------------------------------------------------------------
def _tri_setup(scene):
    v = np.asarray(scene.tri_v, np.float64).reshape(-1, 3, 3)
    A, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    n = np.cross(e1, e2)
    # Moeller-Trumbore with the ray's moment m = o x d, so that every term is a
    # (ray, triangle) matrix product:
    #   det   = e1 . (d x e2)      = -d . n
    #   u det = (o - A) . (d x e2) =  e2 . m - d . (e2 x A)
    #   v det = d . ((o - A) x e1) = -e1 . m - d . (A x e1)
    #   t det = e2 . ((o - A) x e1) = (o - A) . n
    return A, e1, e2, n, np.cross(e2, A), np.cross(A, e1), np.sum(A * n, axis=1)


def _tris_block(ts, o, d, grows):
    """Closest triangle hit of each ray of a block, for each grow: [(t, index)].
    u for every (ray, triangle) pair; v and t only for the pairs whose u passes."""
    A, e1, e2, n, e2xA, Axe1, An = ts
    m = np.cross(o, d)
    e = UV_MARGIN * max(max(grows), 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        inv = -1.0 / (d @ n.T)                       # inf where the ray lies in the plane: u is inf or NaN
        u = (m @ e2.T - d @ e2xA.T) * inv
        ri, ci = np.nonzero((u >= -e) & (u <= 1.0 + e))
        u, inv = u[ri, ci], inv[ri, ci]
        mr, dr, orr = m[ri], d[ri], o[ri]
        v = (-np.sum(mr * e1[ci], axis=1) - np.sum(dr * Axe1[ci], axis=1)) * inv
        t = (np.sum(orr * n[ci], axis=1) - An[ci]) * inv
        out = []
        for grow in grows:
            e = UV_MARGIN * grow
            hit = np.isfinite(inv) & (t >= 0.0) & (u >= -e) & (v >= -e) & (u + v <= 1.0 + e)
            out.append(_closest_per_ray(len(o), ri[hit], ci[hit], t[hit]))
    return out


def _closest_per_ray(n, ri, ci, t):
    """(ray, object, t) hit triples -> per ray the smallest t and its object; inf / -1 without one."""
    tt = np.full(n, np.inf)
    kk = np.full(n, -1, np.int64)
    if len(ri):
        order = np.lexsort((t, ri))                  # by ray, then by t: the first of each ray is its closest
        ri, ci, t = ri[order], ci[order], t[order]
        first = np.nonzero(np.r_[True, ri[1:] != ri[:-1]])[0]
        tt[ri[first]] = t[first]
        kk[ri[first]] = ci[first]
    return tt, kk


def triangle_hit_plain(scene, orig, d):
    """One ray against every triangle by textbook Moeller-Trumbore (grow 0): the
    cross-check of _tris_block's matrix-product form."""
    v = np.asarray(scene.tri_v, np.float64).reshape(-1, 3, 3)
    o, d = np.asarray(orig, np.float64), np.asarray(d, np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    p = np.cross(d, e2)
    det = np.sum(e1 * p, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = o - v[:, 0]
        u = np.sum(s * p, axis=1) / det
        q = np.cross(s, e1)
        vv = np.sum(q * d, axis=1) / det
        t = np.sum(e2 * q, axis=1) / det
        hit = (det != 0) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (t >= 0)
    if not hit.any():
        return np.inf, -1
    k = int(np.argmin(np.where(hit, t, np.inf)))
    return float(t[k]), k


# ---- queries -------------------------------------------------------------------------------
def brute_force_variants(scene, orig, d, grows=(-1, 0, 1)):
    """[(t, obj)] for each grow; t float64 (inf on a miss), obj int64 (-1 on a miss)."""
    o = np.asarray(orig, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    nt, nc = len(scene.tri_v), len(scene.cone_base_r0)
    ts = _tri_setup(scene) if nt else None
    cs = cone_setup(scene) if nc else None
    T = [np.full(len(o), np.inf) for _ in grows]
    K = [np.full(len(o), -1, np.int64) for _ in grows]
    for i in range(0, len(o), _CHUNK):
        ob, db = o[i:i + _CHUNK], d[i:i + _CHUNK]
        sl = slice(i, i + len(ob))
        if nt:
            for gi, (t, k) in enumerate(_tris_block(ts, ob, db, grows)):
                T[gi][sl], K[gi][sl] = t, k
        if nc:
            for gi, (t, k) in enumerate(_cones_block(cs, ob, db, grows)):
                nearer = t < T[gi][sl]
                T[gi][sl] = np.where(nearer, t, T[gi][sl])
                K[gi][sl] = np.where(nearer, k + nt, K[gi][sl])
    return list(zip(T, K))


def brute_force(scene, orig, d, grow=0):
    """Closest hit of every ray over every object: (t, obj); inf / -1 on a miss."""
    return brute_force_variants(scene, orig, d, (grow,))[0]


class Truth:
    """The reference for one ray set: t, obj (grow 0), the decisive rays of the
    closest-hit query and, for the any-hit query at tmax, answer and decisive rays."""

    def __init__(self, scene, orig, d, tmax):
        self.orig = np.ascontiguousarray(orig, np.float32)
        self.d = np.ascontiguousarray(d, np.float32)
        self.tmax = np.ascontiguousarray(tmax, np.float32)
        (tm, km), (t0, k0), (tp, kp) = brute_force_variants(scene, self.orig, self.d)
        self.t, self.obj = t0, k0
        same_obj = (km == k0) & (kp == k0)
        tol = tau(t0)
        with np.errstate(invalid="ignore"):
            same_t = (k0 < 0) | ((np.abs(tm - t0) <= tol) & (np.abs(tp - t0) <= tol))
        self.decisive = same_obj & same_t
        self.any = t0 <= self.tmax.astype(np.float64)
        with np.errstate(invalid="ignore"):
            clear = (k0 < 0) | (np.abs(t0 - self.tmax) > tol)
        self.any_decisive = self.decisive & clear


# ---- ray families --------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def hair_aimed_rays(scene, n, seed):
    """Family (a): aimed at a random point of a random cone's axis, jittered by
    N(0, (1.5 r)^2) with r the radius there, from 0.02 .. 1.0 away; the any-hit
    tmax is 0.2 .. 1.8 of that distance.  float32 (orig, d, tmax), d unit length."""
    rng = np.random.default_rng(seed)
    base, axis, h, r0, r1 = cone_setup(scene)
    k = rng.integers(0, len(h), n)
    f = rng.uniform(0.0, 1.0, n)
    r = r0[k] + f * (r1[k] - r0[k])
    target = base[k] + (f * h[k])[:, None] * axis[k] + rng.normal(size=(n, 3)) * (1.5 * r)[:, None]
    dist = rng.uniform(0.02, 1.0, n)
    orig = (target + _unit(rng, n) * dist[:, None]).astype(np.float32)
    d = target - orig
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)      # unit length in float32, as the queries get it
    tmax = (dist * rng.uniform(0.2, 1.8, n)).astype(np.float32)
    return orig, d, tmax


def unaimed_rays(n, seed):
    """Family (b): the rays of test_gpu_parity.test_trace_queries."""
    rng = np.random.default_rng(seed)
    orig = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32) + np.float32([0, 1, 0])
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rng.uniform(0.01, 2.0, n).astype(np.float32)
    return orig, d, tmax


# ---- geometry samples for the bounds checks ------------------------------------------------
def object_points(scene, n_rim=64):
    """Float64 points every object's bound must contain: (n_objects, P, 3), P =
    2 n_rim; a cone's are n_rim points on each rim circle of the frustum, a
    triangle's its three vertices (repeated to fill P)."""
    P = 2 * n_rim
    out = []
    if len(scene.tri_v):
        v = np.asarray(scene.tri_v, np.float64).reshape(-1, 3, 3)
        out.append(v[:, np.arange(P) % 3])
    if len(scene.cone_base_r0):
        base, axis, h, r0, r1 = cone_setup(scene)
        # any orthonormal pair perpendicular to the axis
        helper = np.where(np.abs(axis[:, 1:2]) < 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
        e1 = np.cross(axis, helper)
        e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = np.cross(axis, e1)
        phi = 2 * np.pi * np.arange(n_rim) / n_rim
        ring = np.cos(phi)[None, :, None] * e1[:, None] + np.sin(phi)[None, :, None] * e2[:, None]
        apex = base + h[:, None] * axis
        out.append(np.concatenate([base[:, None] + r0[:, None, None] * ring,
                                   apex[:, None] + r1[:, None, None] * ring], axis=1))
    return np.concatenate(out)
