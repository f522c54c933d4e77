"""numpy float32 restatement of khp_denoise_var / khp_denoise_var_host (include/kirk_hip.h,
DESIGN.md §17) for the tests: what the definition says, operation by operation, and nothing of
the kernels.

It is _denoiseref.denoise's loop (the same tap order, weights and counting rule) with the three
changes of §17: the colour distance is multiplied by icv = inv_sc / (vbar + floor) per pixel, vbar
being the pixel's own variance or the trimmed 3 x 3 prefilter of it; the variance is filtered along
the taps with the weights squared; and it is returned, +inf where unknown.  The prefilter is a
function argument so that a test can substitute another one and show what the trimming is for.
"""
import numpy as np

from _denoiseref import DEFAULTS, F32, H5, _d2, _unit, bits, k_expf, random_case  # noqa: F401

G3 = (F32(0.25), F32(0.5), F32(0.25))
SCAN3 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _window(Hh, Ww, oy, ox):
    """(P, Q): the pixels that have the tap at offset (oy, ox) and the taps themselves, or None."""
    y0, y1, x0, x1 = max(0, -oy), min(Hh, Hh - oy), max(0, -ox), min(Ww, Ww - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def prepare_noise(shape, variance=None, moments=None):
    """(v, known) of the definition's prepare: `variance` a plane, or `moments` with m2 and count."""
    with np.errstate(all="ignore"):
        if variance is not None:
            u = np.array(variance, F32).reshape(shape)
            has = np.ones(shape, bool)
        else:
            m2 = np.asarray(moments["m2"], F32).reshape(shape + (3,))
            n = np.asarray(moments["count"], np.uint32).reshape(shape)
            nf = n.astype(F32)
            s = (m2[..., 0] + m2[..., 1]) + m2[..., 2]
            has = n >= 2
            u = np.where(has, s / np.where(has, nf * (nf - F32(1.0)), F32(1.0)), F32(0.0)).astype(F32)
        known = has & np.isfinite(u) & (u >= 0)
        return np.where(known, u, F32(0.0)).astype(F32), known


def trimmed_prefilter(v, known):
    """(vbar, kbar): the 3 x 3 Gaussian over the known taps inside the image, dy outer and dx inner,
    without the first tap in scan order holding the largest v when two or more are known."""
    Hh, Ww = v.shape
    cnt = np.zeros((Hh, Ww), np.int64)
    best = np.full((Hh, Ww), -1, np.int64)
    bestv = np.zeros((Hh, Ww), F32)
    for k, (dy, dx) in enumerate(SCAN3):
        win = _window(Hh, Ww, dy, dx)
        if win is None:
            continue
        P, Q = win
        kq = known[Q]
        cnt[P] += kq
        better = kq & ((best[P] < 0) | (v[Q] > bestv[P]))
        best[P] = np.where(better, k, best[P])
        bestv[P] = np.where(better, v[Q], bestv[P])
    best = np.where(cnt >= 2, best, -1)
    gs, gw = np.zeros((Hh, Ww), F32), np.zeros((Hh, Ww), F32)
    for k, (dy, dx) in enumerate(SCAN3):
        win = _window(Hh, Ww, dy, dx)
        if win is None:
            continue
        P, Q = win
        g = G3[dy + 1] * G3[dx + 1]
        use = known[Q] & (best[P] != k)
        gs[P] = np.where(use, gs[P] + g * v[Q], gs[P])
        gw[P] = np.where(use, gw[P] + g, gw[P])
    kbar = gw > 0
    assert gs.dtype == F32 and gw.dtype == F32
    return np.where(kbar, gs / np.where(kbar, gw, F32(1.0)), F32(0.0)).astype(F32), kbar


def denoise_var(colour, guides, variance=None, moments=None, prefilter=1, floor=1e-6, prefilter_fn=trimmed_prefilter,
                **params):
    """The definition on an (H, W, 3) float32 frame.  Returns (out, out_variance), new arrays."""
    prm = dict(DEFAULTS)
    for k, val in params.items():
        assert k in prm, k
        prm[k] = val
    c = np.array(colour, F32)
    Hh, Ww = c.shape[:2]
    floor = F32(floor)
    sig = {k: F32(prm["sigma_" + k]) for k in ("color", "normal", "tangent", "depth", "coverage")}
    on = {k: bool(s > 0) for k, s in sig.items()}
    with np.errstate(all="ignore"):
        inv_s = {k: (F32(1.0) / (s * s) if on[k] else F32(0.0)) for k, s in sig.items()}
        # ---- prepare (§13's, without demodulation; then the variance)
        reads_cov = on["normal"] or on["tangent"] or on["depth"] or on["coverage"]
        cv = np.asarray(guides["coverage"], F32) if reads_cov else np.zeros((Hh, Ww), F32)
        inv = np.where(cv > 0, F32(1.0) / np.where(cv > 0, cv, F32(1.0)), F32(0.0)).astype(F32)
        n = _unit(np.asarray(guides["normal"], F32), inv) if on["normal"] else None
        t = _unit(np.asarray(guides["tangent"], F32), inv) if on["tangent"] else None
        d = (np.asarray(guides["depth"], F32) * inv).astype(F32) if on["depth"] else None
        clamp = F32(prm["clamp"])
        if clamp > 0:
            c = np.where(c > clamp, clamp, c).astype(F32)
        v, known = prepare_noise((Hh, Ww), variance, moments)
        # ---- iterate
        for it in range(int(prm["iterations"])):
            s = 1 << it
            fin = np.isfinite(c).all(-1)
            if prefilter:
                vbar, kbar = prefilter_fn(v, known)
            else:
                vbar, kbar = v, known
            colour_on = fin & kbar if on["color"] else np.zeros((Hh, Ww), bool)
            icv = (inv_s["color"] / (vbar + floor)).astype(F32)
            acc = np.zeros((Hh, Ww, 3), F32)
            ws, va, wk = np.zeros((Hh, Ww), F32), np.zeros((Hh, Ww), F32), np.zeros((Hh, Ww), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    win = _window(Hh, Ww, dy * s, dx * s)
                    if win is None:
                        continue
                    P, Q = win
                    X = np.zeros(ws[P].shape, F32)
                    if on["color"]:
                        X = np.where(colour_on[P], X + _d2(c[P], c[Q]) * icv[P], X)
                    if on["normal"]:
                        X = X + _d2(n[P], n[Q]) * inv_s["normal"]
                    if on["tangent"]:
                        X = X + _d2(t[P], t[Q]) * inv_s["tangent"]
                    if on["depth"]:
                        e = d[P] - d[Q]
                        X = X + (e * e) * inv_s["depth"]
                    if on["coverage"]:
                        e = cv[P] - cv[Q]
                        X = X + (e * e) * inv_s["coverage"]
                    w = (H5[dy + 2] * H5[dx + 2]) * k_expf(-X)
                    assert w.dtype == F32 and X.dtype == F32
                    counts = fin[Q] & (w > 0)
                    acc[P] = np.where(counts[..., None], acc[P] + w[..., None] * c[Q], acc[P])
                    ws[P] = np.where(counts, ws[P] + w, ws[P])
                    kq = counts & known[Q]
                    va[P] = np.where(kq, va[P] + (w * w) * v[Q], va[P])
                    wk[P] = np.where(kq, wk[P] + w, wk[P])
            has = ws > 0
            c = np.where(has[..., None], acc / np.where(has, ws, F32(1.0))[..., None], c).astype(F32)
            k2 = wk > 0
            v2 = np.where(k2, va / np.where(k2, wk * wk, F32(1.0)), F32(0.0)).astype(F32)
            v = np.where(has, v2, v).astype(F32)
            known = np.where(has, k2, known)
        # ---- finish
        out_variance = np.where(known, v, F32(np.inf)).astype(F32)
    return c, out_variance


def random_noise(width, height, seed, source="plane"):
    """Seeded noise for a width x height frame.  source "plane": an (H, W) variance plane of gamma
    values with some 0, NaN, +inf, negative and 1e30 entries and one 1e6 firefly (where the frame has
    room).  source "moments": {"m2": (H, W, 3), "count": (H, W) in 0..5}, some m2 entries bad too."""
    rng = np.random.default_rng(seed)
    shape = (height, width)
    npix = width * height
    bad = (0.0, np.nan, np.inf, -0.5, 1e30, 0.0, np.nan, -1e-3)
    if source == "plane":
        v = rng.gamma(2.0, 0.02, size=shape).astype(F32)
        if npix > 1:
            idx = rng.choice(npix, size=min(len(bad) + 1, npix // 2), replace=False)
            flat = v.reshape(-1)
            flat[idx[0]] = 1e6                                     # the firefly
            for k, val in zip(idx[1:], bad):
                flat[k] = val
        return v
    m2 = rng.gamma(2.0, 0.05, size=shape + (3,)).astype(F32)
    count = rng.integers(0, 6, size=shape).astype(np.uint32)
    if npix > 1:
        idx = rng.choice(npix, size=min(len(bad), npix // 2), replace=False)
        flat = m2.reshape(-1, 3)
        for k, val in zip(idx, bad):
            flat[k, rng.integers(0, 3)] = val
    return {"m2": m2, "count": count}
