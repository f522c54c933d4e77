"""numpy restatement of the thin-lens camera (include/kirk_hip.h "a thin-lens camera")
for the tests, written from the definition and nothing of csrc/lens.h:

  * lens_rays: the definition in float32, one numpy operation per step in the order written, on top of
    _aovref.camera_rays / normalize32 (the pinhole ray); sine and cosine are kmath.h's k_sinf / k_cosf
    restated here operation by operation, as _furref restates lowbias32 and draw_u01;
  * truth64: the geometry in float64 from the same float32 inputs, independently of the steps -- the
    focus point from the pinhole model, the lens plane through `position` -- and what a ray misses it by;
  * disk64: the concentric map in float64 with libm's sine and cosine.
"""
import numpy as np

import _aovref as A
from _furref import draw_u01

F32 = np.float32
P_LENS_U, P_LENS_V = 10, 11
FOCUS_KIRK, FOCUS_PLANE = 0, 1
PI_4 = np.float32(np.pi / 4)     # 0x3F490FDB
PI_2 = np.float32(np.pi / 2)     # 0x3FC90FDB

# kmath.h: Cephes sinf / cosf
FOPI = F32(1.27323954473516)
DP1, DP2, DP3 = F32(0.78515625), F32(2.4187564849853515625e-4), F32(3.77489497744594108e-8)
DP3A, DP3B = F32(float.fromhex("0x1.444p-25")), F32(float.fromhex("0x1.68c234p-40"))
S0, S1, S2 = F32(-1.9515295891E-4), F32(8.3321608736E-3), F32(1.6666654611E-1)
C0, C1, C2 = F32(2.443315711809948E-005), F32(1.388731625493765E-003), F32(4.166664568298827E-002)


def _sin_poly(z, x):
    return (((S0 * z + S1) * z - S2) * z) * x + x


def _cos_poly(z):
    y = (((C0 * z - C1) * z + C2) * z) * z
    y = y - F32(0.5) * z
    return y + F32(1.0)


def _reduce(x):
    """|x| reduced to an octant: (j, the remainder, its square), as k_sinf and k_cosf both do it."""
    j = (FOPI * x).astype(np.int32)
    y = j.astype(F32)
    odd = (j & 1) != 0
    j = np.where(odd, j + 1, j)
    y = np.where(odd, y + F32(1.0), y).astype(F32)
    j = j & 7
    r2 = (x - y * DP1) - y * DP2
    r = r2 - y * DP3
    r = np.where(np.abs(r) < F32(2.0 ** -20), (r2 - y * DP3A) - y * DP3B, r).astype(F32)   # k_reduce's second take
    return j, r, r * r


def k_sinf(x):
    x = np.asarray(x, F32)
    neg = x < 0
    j, r, z = _reduce(np.where(neg, -x, x).astype(F32))
    hi = j > 3
    neg = neg ^ hi
    j = np.where(hi, j - 4, j)
    y = np.where((j == 1) | (j == 2), _cos_poly(z), _sin_poly(z, r)).astype(F32)
    return np.where(neg, -y, y).astype(F32)


def k_cosf(x):
    x = np.asarray(x, F32)
    j, r, z = _reduce(np.abs(x))
    hi = j > 3
    neg = hi.copy()
    j = np.where(hi, j - 4, j)
    neg = neg ^ (j > 1)
    y = np.where((j == 1) | (j == 2), _sin_poly(z, r), _cos_poly(z)).astype(F32)
    return np.where(neg, -y, y).astype(F32)


def disk32(u, v):
    """Step 3, the concentric map, in float32: the point of the unit disk for (u, v) in [0, 1)^2."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    a, b = F32(2.0) * u - F32(1.0), F32(2.0) * v - F32(1.0)
    first = np.abs(a) > np.abs(b)
    zero = (a == 0) & (b == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(first, a, b)
        phi = np.where(first, PI_4 * (b / a), PI_2 - PI_4 * (a / b)).astype(F32)
        x, y = r * k_cosf(phi), r * k_sinf(phi)
    return np.where(zero, F32(0.0), x).astype(F32), np.where(zero, F32(0.0), y).astype(F32)


def disk64(u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    a, b = 2.0 * u - 1.0, 2.0 * v - 1.0
    first = np.abs(a) > np.abs(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(first, a, b)
        phi = np.where(first, (np.pi / 4) * (b / a), np.pi / 2 - (np.pi / 4) * (a / b))
        phi = np.where((a == 0) & (b == 0), 0.0, phi)
    return r * np.cos(phi), r * np.sin(phi)


def _v(a, n):
    return np.tile(F32(list(a)), (n, 1))


def dot32(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0],
                     a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1).astype(F32)


def lens_rays(cam, width, pixels, seed, samples, radius, focus_distance, focus, unnormalised=False):
    """The definition, steps 1-5: (origins, directions) of the camera rays, float32.  unnormalised: the
    directions before the last normalisation (a batch query normalises what it is given, as KIRK::Ray does)."""
    p, raw, key = A.camera_rays(cam, width, pixels, seed, samples)             # 1: the pinhole ray
    d = A.normalize32(raw)
    if not radius > 0:
        return p, (raw if unnormalised else d)
    n = len(p)
    radius, fd = F32(radius), F32(focus_distance)
    u, v = draw_u01(key, P_LENS_U), draw_u01(key, P_LENS_V)                     # 2: the draws (bounce 0: dim = purpose)
    dx, dy = disk32(u, v)                                                       # 3: the disk
    lx, ly = radius * dx, radius * dy
    ax, ay = _v(cam.axis_x, n), _v(cam.axis_y, n)
    ft = np.full(n, fd, F32)                                                    # 4: the focus point
    if focus == FOCUS_PLANE:
        fwd = A.normalize32(cross32(ay, ax))
        c = dot32(d, fwd)
        with np.errstate(invalid="ignore", divide="ignore"):
            ft = np.where(c > 0, fd / c, fd).astype(F32)
    f = p + d * ft[:, None]
    start = (p + ax * lx[:, None]) + ay * ly[:, None]                           # 5: the lens ray
    to = (f - start).astype(F32)
    return start.astype(F32), (to if unnormalised else A.normalize32(to))


def truth64(cam, width, pixels, seed, samples, focus_distance, focus):
    """float64, from the float32 camera and the float32 draws: the focus point of every path from the
    pinhole model (the pixel's sensor point seen from `position`), and the lens plane's frame."""
    pixels = np.asarray(pixels, np.uint64)
    key = A.path_key(seed, pixels, samples)
    x, y = (pixels % np.uint64(width)).astype(np.float64), (pixels // np.uint64(width)).astype(np.float64)
    c = {k: np.array(list(getattr(cam, k)), np.float64) for k in ("position", "bottom_left", "axis_x", "axis_y")}
    ps = float(cam.pixel_size)
    s1 = (x + draw_u01(key, A.P_CAM_X).astype(np.float64)) * ps
    s2 = (y + draw_u01(key, A.P_CAM_Y).astype(np.float64)) * ps
    to = c["bottom_left"] + c["axis_x"] * s1[:, None] + c["axis_y"] * s2[:, None] - c["position"]
    d = to / np.linalg.norm(to, axis=1)[:, None]
    fwd = np.cross(c["axis_y"], c["axis_x"])
    fwd /= np.linalg.norm(fwd)
    fd = float(F32(focus_distance))
    ft = np.full(len(pixels), fd)
    if focus == FOCUS_PLANE:
        cosine = d @ fwd
        ft = np.where(cosine > 0, fd / np.where(cosine > 0, cosine, 1.0), fd)
    return {"p": c["position"], "f": c["position"] + d * ft[:, None], "fwd": fwd, "axis_x": c["axis_x"],
            "axis_y": c["axis_y"], "fd": fd}


def deviations(t, o, d, radius):
    """What rays (o, d) miss the float64 truth `t` by, each as an absolute length:
    plane: the origin's distance from the lens plane; disk: by how much it lies outside the lens;
    focus: the line's distance from the focus point; kirk / planar: |f - p| and dot(f - p, fwd)
    against focus_distance, measured at the point of the line nearest to f."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = np.cross(t["axis_x"], t["axis_y"])
    n /= np.linalg.norm(n)
    rel = o - t["p"]
    w = t["f"] - o
    along = np.einsum("ij,ij->i", w, d) / np.einsum("ij,ij->i", d, d)
    near = o + d * along[:, None]
    return {"plane": np.abs(rel @ n),
            "disk": np.maximum(np.linalg.norm(rel, axis=1) - float(F32(radius)), 0.0),
            "focus": np.linalg.norm(near - t["f"], axis=1),
            "kirk": np.abs(np.linalg.norm(near - t["p"], axis=1) - t["fd"]),
            "planar": np.abs((near - t["p"]) @ t["fwd"] - t["fd"])}
