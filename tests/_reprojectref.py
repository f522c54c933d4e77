"""numpy float32 restatement of khp_reproject / khp_reproject_host (include/kirk_hip.h)
for the tests: what the definition says, operation by operation, and nothing of the kernel.

Every operation is one float32 operation in the definition's order (numpy keeps float32 for float32
operands; sums of three are written (x*x + y*y) + z*z).  The four taps are a Python loop in the
definition's order, dy outer and dx inner, each vectorised over all pixels.  Besides the four outputs
the restatement returns what it saw on the way (`info`), so a test can assert that its cases hold the
situations they are meant to hold.  The seeded frames of the CPU and the GPU tests are made here too.
"""
import numpy as np

from _denoiseref import F32, _unit, bits  # noqa: F401

DEFAULTS = dict(samples=1.0, max_history=32.0, depth_tol=0.05, normal_tol=0.0, tangent_tol=0.25, coverage_tol=0.5,
                match_object=False)
NAN = np.uint32(0x7FC00000).view(F32)
INF = F32(np.inf)


def cam_arrays(cam):
    """(position, bottom_left, axis_x, axis_y, pixel_size) of an N.Camera as float32."""
    v = lambda a: np.array(list(a), F32)
    return v(cam.position), v(cam.bottom_left), v(cam.axis_x), v(cam.axis_y), F32(cam.pixel_size)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    """kmath.h cross: (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)."""
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1).astype(F32)


def _known(v):
    return np.isfinite(v) & (v >= 0)


def reproject(W, H, cur, hist=None, **params):
    """The definition on frames given as HipContext.reproject takes them.  Returns a dict of new arrays
    colour, length, variance, motion, and `info`."""
    prm = dict(DEFAULTS)
    for k, v in params.items():
        assert k in prm, k
        prm[k] = v
    s, maxh = F32(prm["samples"]), F32(prm["max_history"])
    tol_d, tol_n, tol_t, tol_c = (F32(prm[k]) for k in ("depth_tol", "normal_tol", "tangent_tol", "coverage_tol"))
    on_d, on_n, on_t, on_c, on_o = tol_d > 0, tol_n > 0, tol_t > 0, tol_c > 0, bool(prm["match_object"])
    g = cur["aov"]
    with np.errstate(all="ignore"):
        # ---- locate ----
        pos, bl, ax, ay, ps = cam_arrays(cur["camera"])
        xs, ys = np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32))
        px, py = xs.astype(F32) + F32(0.5), ys.astype(F32) + F32(0.5)
        sx, sy = px * ps, py * ps
        dirv = ((bl + ax * sx[..., None]) + ay * sy[..., None]) - pos
        u = dirv / np.sqrt((dirv[..., 0] * dirv[..., 0] + dirv[..., 1] * dirv[..., 1]) + dirv[..., 2] * dirv[..., 2])[..., None]
        cv = np.asarray(g["coverage"], F32)
        surf = cv > 0
        inv_cv = np.where(surf, F32(1.0) / np.where(surf, cv, F32(1.0)), F32(0.0)).astype(F32)
        d = np.where(surf, np.asarray(g["depth"], F32) * inv_cv, F32(0.0)).astype(F32)
        assert u.dtype == F32 and d.dtype == F32

        # ---- project ----
        zero, false = np.zeros((H, W), F32), np.zeros((H, W), bool)
        fx, fy, dist, exists, det, t = zero, zero, zero, false, zero, zero
        if hist is not None:
            hpos, hbl, hax, hay, hps = cam_arrays(hist["camera"])
            wsurf = (pos + u * d[..., None]) - hpos
            w = np.where(surf[..., None], wsurf, u).astype(F32)
            dist = np.where(surf, np.sqrt(_dot(w, w)), F32(0.0)).astype(F32)
            n = _cross(hax, hay)
            det = _dot(w, n)
            e = hbl - hpos
            t = _dot(e, n) / det
            hvec = w * t[..., None] - e
            a, b = _dot(hvec, hax) / _dot(hax, hax), _dot(hvec, hay) / _dot(hay, hay)
            fx, fy = a / hps, b / hps
            exists = np.isfinite(det) & (det != 0) & np.isfinite(t) & (t > 0)
            assert fx.dtype == F32 and det.dtype == F32 and t.dtype == F32
        motion = np.stack([np.where(exists, fx - px, NAN), np.where(exists, fy - py, NAN)], -1).astype(F32)

        # ---- taps ----
        ws, al, va, wk = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        ac = np.zeros((H, W, 3), F32)
        gx, gy = fx - F32(0.5), fy - F32(0.5)
        cand = exists & (gx > F32(-1.0)) & (gx < F32(W)) & (gy > F32(-1.0)) & (gy < F32(H))
        x0f, y0f = np.floor(np.where(cand, gx, F32(0.0))), np.floor(np.where(cand, gy, F32(0.0)))
        wx, wy = np.where(cand, gx, F32(0.0)) - x0f, np.where(cand, gy, F32(0.0)) - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        counted = np.zeros((4, H, W), bool)
        if hist is not None:
            hg = hist.get("aov") or {}
            hcol, hlen = np.asarray(hist["colour"], F32), np.asarray(hist["length"], F32)
            hvar = np.asarray(hist["variance"], F32) if hist.get("variance") is not None else np.full((H, W), -1.0, F32)
            if on_n:
                an = _unit(np.asarray(g["normal"], F32), inv_cv)
                has_n = (an != 0).any(-1)
            if on_t:
                at = _unit(np.asarray(g["tangent"], F32), inv_cv)
                has_t = (at != 0).any(-1)
            for k in range(4):
                dx, dy = k & 1, k >> 1
                xq, yq = x0 + dx, y0 + dy
                inside = (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                xc, yc = np.clip(xq, 0, W - 1), np.clip(yq, 0, H - 1)
                bw = ((wy if dy else F32(1.0) - wy) * (wx if dx else F32(1.0) - wx)).astype(F32)
                cq, lq, vq = hcol[yc, xc], hlen[yc, xc], hvar[yc, xc]
                ok = cand & inside & (bw > 0) & np.isfinite(cq).all(-1) & np.isfinite(lq) & (lq > 0)
                if on_d or on_n or on_t or on_c:
                    cvq = np.asarray(hg["coverage"], F32)[yc, xc]
                    surf_q = cvq > 0
                    inv_q = np.where(surf_q, F32(1.0) / np.where(surf_q, cvq, F32(1.0)), F32(0.0)).astype(F32)
                if on_d:
                    dq = np.asarray(hg["depth"], F32)[yc, xc] * inv_q
                    both = surf & surf_q
                    ok &= (surf == surf_q) & (~both | (np.abs(dq - dist) <= tol_d * dist))
                if on_n:
                    bn = _unit(np.asarray(hg["normal"], F32)[yc, xc], inv_q)
                    tested = has_n & (bn != 0).any(-1)
                    ok &= ~tested | (F32(1.0) - _dot(an, bn) <= tol_n)
                if on_t:
                    bt = _unit(np.asarray(hg["tangent"], F32)[yc, xc], inv_q)
                    tested = has_t & (bt != 0).any(-1)
                    ok &= ~tested | (F32(1.0) - _dot(at, bt) <= tol_t)
                if on_c:
                    ok &= np.abs(cv - cvq) <= tol_c
                if on_o:
                    ok &= np.asarray(g["object"], np.int32) == np.asarray(hg["object"], np.int32)[yc, xc]
                counted[k] = ok
                ws = np.where(ok, ws + bw, ws)
                ac = np.where(ok[..., None], ac + bw[..., None] * cq, ac)
                al = np.where(ok, al + bw * lq, al)
                kn = ok & _known(vq)
                va = np.where(kn, va + (bw * bw) * vq, va)
                wk = np.where(kn, wk + bw, wk)
            assert ws.dtype == F32 and ac.dtype == F32 and al.dtype == F32 and va.dtype == F32 and wk.dtype == F32
        have = ws > 0
        h = ac / ws[..., None]
        N = al / ws
        vh_known = wk > 0
        vh = va / (wk * wk)

        # ---- blend ----
        c = np.asarray(cur["colour"], F32)
        fin = np.isfinite(c).all(-1)
        vc = np.asarray(cur["variance"], F32) if cur.get("variance") is not None else np.full((H, W), -1.0, F32)
        vc_known = _known(vc)
        Nc = np.where(maxh < N, maxh, N).astype(F32) if maxh > 0 else N        # gmin(N, max_history)
        alpha = s / (Nc + s)
        om = F32(1.0) - alpha
        blend = h + alpha[..., None] * (c - h)
        v_blend = np.where(vc_known, np.where(vh_known, (om * om) * vh + (alpha * alpha) * vc, vc), INF)
        hf, hn, nf = have & fin, have & ~fin, ~have & fin
        colour = np.where(hf[..., None], blend, np.where(hn[..., None], h, c)).astype(F32)
        # where the current colour is kept its bits are kept: np.where selects, it does not compute
        length = np.where(hf, Nc + s, np.where(hn, Nc, np.where(nf, s, F32(0.0)))).astype(F32)
        variance = np.where(hf, v_blend, np.where(hn, np.where(vh_known, vh, INF),
                                                  np.where(nf & vc_known, vc, INF))).astype(F32)
    info = dict(exists=exists, cand=cand, have=have, fin=fin, surf=surf, det=det, t=t, gx=gx, gy=gy, x0=x0, y0=y0,
                counted=counted, vc_known=vc_known, vh_known=vh_known, N=N)
    return dict(colour=colour, length=length, variance=variance, motion=motion, info=info)


# ---- seeded frames -------------------------------------------------------------------------------------
def look_camera(scenes, W, H, position, look, up=(0.0, 1.0, 0.0)):
    return scenes.camera(position, look, up, W, H)


def camera_pairs(scenes, W, H, seed):
    """Seeded (name, current camera, history camera) pairs from khp_camera_setup around a wall at z = 0
    seen from z = 2: the identity, small rotations, translations worth a few pixels, both together,
    a history camera that looks the other way (t <= 0) and a degenerate one (axis_x parallel to axis_y)."""
    rng = np.random.default_rng(seed)
    base_p, base_l = np.array([0.1, -0.2, 2.0]), np.array([0.0, 0.02, -1.0])
    A = look_camera(scenes, W, H, base_p, base_l)
    ps = float(A.pixel_size)                                    # on the image plane at distance 1
    pairs = [("identity", A, A)]
    for i in range(2):
        rot = rng.uniform(-3.0, 3.0, 3) * ps * np.array([1.0, 1.0, 0.0])
        pairs.append((f"rotate{i}", A, look_camera(scenes, W, H, base_p, base_l + rot)))
    for i in range(2):
        shift = rng.uniform(-3.0, 3.0, 3) * ps * 2.0            # at depth 2 a shift of 2 ps is one pixel
        pairs.append((f"translate{i}", A, look_camera(scenes, W, H, base_p + shift, base_l)))
    rot, shift = rng.uniform(-2.0, 2.0, 3) * ps, rng.uniform(-2.5, 2.5, 3) * ps * 2.0
    pairs.append(("both", look_camera(scenes, W, H, base_p + shift, base_l + rot), A))
    pairs.append(("behind", A, look_camera(scenes, W, H, base_p, -base_l)))
    deg = type(A).from_buffer_copy(bytes(A))
    for i in range(3):
        deg.axis_y[i] = deg.axis_x[i]
    pairs.append(("degenerate", A, deg))
    return pairs


def random_frame(W, H, cam, seed, history, bad=True):
    """A seeded frame of a wall at z = 0 with noise on it, as a dict for HipContext.reproject: colours
    with non-finite pixels, a variance plane with unknown entries, a length plane with zeros (history),
    background pixels, fractional coverage, and planes premultiplied by coverage."""
    rng = np.random.default_rng(seed)
    pos, bl, ax, ay, ps = (np.asarray(a, np.float64) for a in cam_arrays(cam))
    xs, ys = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    dirv = bl + ax * (xs * ps)[..., None] + ay * (ys * ps)[..., None] - pos
    un = dirv / np.linalg.norm(dirv, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        tz = np.where(np.abs(un[..., 2]) > 1e-6, -pos[2] / un[..., 2], 2.0)
    depth = np.where((tz > 0.5) & (tz < 4.0), tz, 2.0) * (1.0 + rng.uniform(-0.02, 0.02, (H, W)))
    depth = np.where(rng.random((H, W)) < 0.06, depth * rng.uniform(0.6, 0.9, (H, W)), depth)   # nearer things
    cov = np.where(rng.random((H, W)) < 0.15, 0.0, np.where(rng.random((H, W)) < 0.3, rng.uniform(0.1, 0.9, (H, W)), 1.0))
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    normal = unit(np.array([0.0, 0.0, 1.0]) + rng.normal(0, 0.35, (H, W, 3)))
    tangent = unit(np.array([0.0, 1.0, 0.0]) + rng.normal(0, 0.6, (H, W, 3)))
    if bad and W * H > 8:
        normal[rng.random((H, W)) < 0.04] = 0.0                 # no length: the test is skipped
        tangent[rng.random((H, W)) < 0.04] = 0.0
    aov = {"normal": (normal * cov[..., None]).astype(F32), "tangent": (tangent * cov[..., None]).astype(F32),
           "depth": (depth * cov).astype(F32), "coverage": cov.astype(F32),
           "object": np.where(cov > 0, rng.integers(0, 3, (H, W)), -1).astype(np.int32)}
    colour = (rng.random((H, W, 3)) * 2.0).astype(F32)
    variance = rng.gamma(2.0, 0.02, (H, W)).astype(F32)
    length = rng.integers(1, 40, (H, W)).astype(F32)
    if bad and W * H > 8:
        for val in (np.nan, np.inf, -np.inf):
            colour[rng.random((H, W)) < 0.03, rng.integers(0, 3)] = val
        for val in (np.nan, np.inf, -1.0):
            variance[rng.random((H, W)) < 0.04] = val
        variance[rng.random((H, W)) < 0.03] = 0.0
        length[rng.random((H, W)) < 0.05] = 0.0
        length[rng.random((H, W)) < 0.02] = np.nan
        length[rng.random((H, W)) < 0.02] = -3.0
        aov["depth"][rng.random((H, W)) < 0.01] = np.nan
    f = {"camera": cam, "colour": colour, "variance": variance, "aov": aov}
    if history:
        f["length"] = length
    return f


def freeze(frame):
    for a in [frame["colour"], frame.get("variance"), frame.get("length")] + list(frame["aov"].values()):
        if a is not None:
            a.setflags(write=False)
    return frame
