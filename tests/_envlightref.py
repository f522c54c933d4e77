"""A numpy restatement of the environment light (khp_set_env_light), written from the definition in
DESIGN.md §23 alone and nothing of csrc/env_light.h:

  * tables: the sampling table in the definition's own float32 steps -- the weights are integers, so this
    must equal the library's word for word.  The sine is kmath.h's k_sinf as _lensref restates it.
  * sample / evaluate: the sampler and the evaluation for a dtype T.  T = float64 with numpy's own sine,
    arcsine and arctangent is the truth; T = float32 measures what the arithmetic itself loses.  The walk
    through the table is integer arithmetic in both.  Each returns the texel it used: an item is decisive
    when that texel is the same under every jitter of its inputs.
"""
import numpy as np

from _lensref import k_sinf

F32 = np.float32
ONE_M = 1.0 - 2.0 ** -24
SCALE = 524288.0   # 2^19


def tables(rgb):
    """weight (H, W) uint32, row_cdf (H, W + 1) uint32, marginal (H + 1) uint64 of the map rgb (H, W, 3)."""
    rgb = np.asarray(rgb, F32)
    H, W = rgb.shape[:2]
    y = (F32(0.2126) * rgb[..., 0] + F32(0.7152) * rgb[..., 1]) + F32(0.0722) * rgb[..., 2]
    dth = F32(np.pi) / F32(H)
    s = k_sinf((np.arange(H).astype(F32) + F32(0.5)) * dth)
    p = (y * s[:, None]).astype(F32)
    m = p.max()
    assert m > 0, "a black map has no table"
    q = ((p / m).astype(F32) * F32(SCALE)).astype(np.uint32)
    weight = np.where(p > 0, np.maximum(q, 1), 0).astype(np.uint32)
    row_cdf = np.zeros((H, W + 1), np.uint64)
    row_cdf[:, 1:] = np.cumsum(weight.astype(np.uint64), axis=1)
    assert row_cdf.max() < 2 ** 32
    marginal = np.zeros(H + 1, np.uint64)
    marginal[1:] = np.cumsum(row_cdf[:, W])
    return {"weight": weight, "row_cdf": row_cdf.astype(np.uint32), "marginal": marginal}


def consts(T, W, H):
    """pi / H, 2 pi / W, 2 pi, 2 pi^2, pi / 2 as T has them (float32: the rounded constants' quotients)."""
    if T is F32:
        two_pi = F32(2 * np.pi)
        return F32(np.pi) / F32(H), two_pi / F32(W), two_pi, F32(2 * np.pi ** 2), F32(np.pi / 2)
    return np.pi / H, 2 * np.pi / W, 2 * np.pi, 2 * np.pi ** 2, np.pi / 2


def evaluate(tab, rgb, dirs, scale=1.0, rotation=0.0, T=np.float64):
    """Radiance (n, 3), pdf (n) and texel (n) of the directions dirs (n, 3), any length."""
    rgb = np.asarray(rgb, F32)
    H, W = rgb.shape[:2]
    dth, dph, two_pi, two_pi_sq, pio2 = consts(T, W, H)
    d = np.asarray(dirs, F32).astype(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        n = d * (T(1) / ln)[:, None]
        ok = np.isfinite(n).all(-1)
        n = np.where(ok[:, None], n, T(0))
        ny = np.clip(n[:, 1], T(-1), T(1))
        th = np.arcsin(ny) + pio2
        ph = np.arctan2(n[:, 2], n[:, 0]) - T(rotation)
        j = np.clip(np.floor(th / dth).astype(np.int64), 0, H - 1)
        t0 = ph / two_pi
        t = t0 - np.floor(t0)
        i = np.clip(np.floor(t * T(W)).astype(np.int64), 0, W - 1)
        texel = j * W + i
        rad = rgb.reshape(-1, 3)[texel].astype(T) * T(scale)
        root = np.sqrt(n[:, 0] * n[:, 0] + n[:, 2] * n[:, 2])
        total = tab["marginal"][H]
        share = tab["weight"].reshape(-1)[texel].astype(T) / T(total)
        pdf = np.where(root > 0, (share * T(W * H)) / (two_pi_sq * root), T(0))
    rad = np.where(ok[:, None], rad, T(0))
    pdf = np.where(ok, pdf, T(0))
    return {"radiance": rad, "pdf": pdf, "texel": np.where(ok, texel, 0)}


def sample(tab, rgb, draws, scale=1.0, rotation=0.0, T=np.float64, dir_rng=None):
    """One direction per pair of draws (n, 2): dir, pdf, radiance, valid, the texel the walk chose and the
    texel the evaluation of the direction found.  dir_rng: jitter the float32 direction by up to 16
    spacings before it is evaluated: float32 arithmetic produces it up to ten away (M_REF32 of `dir`)."""
    rgb = np.asarray(rgb, F32)
    H, W = rgb.shape[:2]
    dth, dph, two_pi, two_pi_sq, pio2 = consts(T, W, H)
    u = np.asarray(draws, F32).astype(np.float64)
    U = np.minimum(np.floor(u * 2.0 ** 24), 2.0 ** 24 - 1).astype(np.uint64)
    marg = tab["marginal"]
    total = marg[H]
    hi, lo = total >> np.uint64(24), total & np.uint64(0xFFFFFF)
    X = U[:, 0] * hi + ((U[:, 0] * lo) >> np.uint64(24))      # floor(U0 total / 2^24) without overflow
    j = np.searchsorted(marg, X, side="right").astype(np.int64) - 1
    rows = tab["row_cdf"][j].astype(np.uint64)                # (n, W + 1)
    rowsum = rows[:, W]
    Y = (U[:, 1] * rowsum) >> np.uint64(24)
    i = (rows[:, :W] <= Y[:, None]).sum(1).astype(np.int64) - 1
    k = np.arange(len(j))
    wt = rows[k, i + 1] - rows[k, i]
    assert (rowsum > 0).all() and (wt > 0).all()
    fy = np.minimum(((X - marg[j]).astype(T) + T(0.5)) / rowsum.astype(T), T(ONE_M))
    fx = np.minimum(((Y - rows[k, i]).astype(T) + T(0.5)) / wt.astype(T), T(ONE_M))
    th = (j.astype(T) + fy) * dth
    ph = (i.astype(T) + fx) * dph + T(rotation)
    st, ct = np.sin(th), np.cos(th)
    d = np.stack([st * np.cos(ph), -ct, st * np.sin(ph)], -1).astype(T)
    # the evaluation of the direction as the next stage receives it: a float32 vector
    d32 = d.astype(F32)
    if dir_rng is not None:
        d32 = jitter(d32, dir_rng, 16)
    e = evaluate(tab, rgb, d32, scale, rotation, T)
    return {"dir": d, "pdf": e["pdf"], "radiance": e["radiance"], "valid": e["pdf"] > 0, "texel": j * W + i,
            "eval_texel": e["texel"]}


def texel_bounds(texel, W, H, rotation=0.0):
    """(theta_lo, theta_hi, phi_lo, phi_hi) of the texels, in float64."""
    j, i = texel // W, texel % W
    return j * np.pi / H, (j + 1) * np.pi / H, i * 2 * np.pi / W + rotation, (i + 1) * 2 * np.pi / W + rotation


def solid_angles(W, H):
    """The solid angle of a texel of each row (H), exact: d phi (cos theta_j - cos theta_{j+1})."""
    th = np.arange(H + 1) * (np.pi / H)
    return (2 * np.pi / W) * (np.cos(th[:-1]) - np.cos(th[1:]))


def centres(W, H, rotation=0.0):
    """The directions of the texel centres (H, W, 3), float64."""
    th = (np.arange(H) + 0.5) * (np.pi / H)
    ph = (np.arange(W) + 0.5) * (2 * np.pi / W) + rotation
    st, ct = np.sin(th)[:, None], np.cos(th)[:, None]
    return np.stack([st * np.cos(ph)[None, :], np.broadcast_to(-ct, (H, W)), st * np.sin(ph)[None, :]], -1)


def jitter(a, rng, ulps=2, lo=None, hi=None):
    """a (float32: unit vectors, or draws in [0, 1)) with every element moved by a whole number in
    [-ulps, ulps] of 2^-24, the float32 spacing just below 1."""
    a = np.ascontiguousarray(a, F32)
    k = rng.integers(-ulps, ulps + 1, a.shape)
    b = (a.astype(np.float64) + k * 2.0 ** -24).astype(F32)
    return b if lo is None else np.clip(b, F32(lo), F32(hi))
