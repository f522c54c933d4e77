"""A numpy restatement of BSDF kind 11 (ChiangHairBSDF), written from the definition in DESIGN.md §22
alone: float64 for the truth, float32 to measure what the arithmetic itself loses.

Every function works on arrays of items and takes the dtype T.  `hair()` returns the value f, the sample
(out, pdf, f, valid), sum A_p, and a branch signature: one row of small integers per item that names every
data-dependent decision the item took (the lobe, the x <= 8 branches, the clamps and wraps, 1 - T F > 0).
An item is decisive when its signature is the same under every +-2 ulp jitter of its inputs.
"""
import numpy as np

F32 = np.float32


def dot(a, b):
    return (a * b).sum(-1)


def normalize(a):
    return a / np.sqrt(dot(a, a))[..., None]


class Sig:
    """Collects the branch decisions of a run, one integer column each."""

    def __init__(self):
        self.cols = []

    def __call__(self, x):
        self.cols.append(np.asarray(x).astype(np.int8))
        return x

    def rows(self):
        n = max(len(c) for c in self.cols if c.ndim)
        return np.concatenate([np.broadcast_to(c.reshape(len(c), -1) if c.ndim else c, (n, c.size // n if c.ndim else 1))
                               for c in self.cols], -1)


def ssqrt(x, sig):
    sig(x < 0)
    return np.sqrt(np.maximum(x, 0))


def sasin(x, sig):
    sig((x < -1).astype(int) - (x > 1).astype(int))
    return np.arcsin(np.clip(x, -1, 1))


def i0s(x):
    v = np.zeros_like(x)
    fact = 1.0
    for i in range(10):
        if i > 1:
            fact *= i
        v = v + x ** (2 * i) / (4.0 ** i * fact * fact)
    return v


def log_i0(x, sig):
    small = sig(x <= 8)
    xs = np.where(small, x, 1)
    xl = np.where(small, 9, x)
    T = x.dtype.type
    big = xl - T(0.5) * np.log(T(2 * np.pi) * xl) + 1 / (8 * xl) + 1 / (16 * xl * xl)
    return np.where(small, np.log(i0s(xs)), big)


def i0(x, sig):
    small = sig(x <= 8)
    return np.where(small, i0s(np.where(small, x, 1)), np.exp(log_i0(np.where(small, 9, x), Sig())))


def mp(cti, cto, sti, sto, v, sig):
    T = v.dtype.type
    a = cti * cto / v
    b = sti * sto / v
    thin = v <= T(0.1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m_thin = np.exp(log_i0(np.where(thin, a, 1), sig) - b - 1 / v + T(np.log(2.0)) + np.log(1 / (2 * v)))
        m_wide = np.exp(-b) * i0(np.where(thin, 1, a), sig) / (np.sinh(1 / np.where(thin, 1, v)) * 2 * v)
    return np.where(thin, m_thin, m_wide)


def logistic(x, s):
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(x) / s)
    return e / (s * (1 + e) ** 2)


def cdf(x, s):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x / s))


def big_phi(p, go, gt, T):
    return 2 * p * gt - 2 * go + p * T(np.pi)


def wrap(d, sig, T):
    pi = T(np.pi)
    k = np.zeros(d.shape, np.int8)
    for _ in range(4):
        hi, lo = d > pi, d < -pi
        d = d - 2 * pi * hi + 2 * pi * lo
        k = k + hi - lo
    sig(k)
    return d


def np_lobe(phi, p, s, go, gt, sig, T):
    d = wrap(phi - big_phi(p, go, gt, T), sig, T)
    pi = T(np.pi)
    return logistic(d, s) / (cdf(pi, s) - cdf(-pi, s))


def fresnel(ci, eta, sig):
    """fresnel_dielectric(ci, 1, eta) for ci in [0, 1]: ci <= 0 swaps the media (then total reflection)."""
    ci = np.clip(ci, -1, 1)
    grazing = sig(ci <= 0)
    si = np.sqrt(np.maximum(0, 1 - ci * ci))
    st = si / eta
    ct = np.sqrt(np.maximum(0, 1 - st * st))
    rparl = (eta * ci - ct) / (eta * ci + ct)
    rperp = (ci - eta * ct) / (ci + eta * ct)
    return np.where(grazing, 1, (rparl * rparl + rperp * rperp) / 2)


def hit(m, U, V, W, n, wo, sig, T):
    pi = T(np.pi)
    eta = m["eta"].astype(T)
    bm = np.clip(m["bm"].astype(T), T(0.01), 1)
    bn = np.clip(m["bn"].astype(T), T(0.01), 1)
    H = {}
    H["sto"] = dot(wo, V)
    H["cto"] = ssqrt(1 - H["sto"] ** 2, sig)
    H["phio"] = np.arctan2(dot(wo, W), dot(wo, U))
    front = sig(dot(wo, n) >= 0)
    npr = np.where(front[..., None], n, -n)
    H["np"] = npr
    phin = np.arctan2(dot(npr, W), dot(npr, U))
    go = wrap(H["phio"] - phin, sig, T)
    h = np.clip(np.sin(go), -1, 1)
    H["h"] = h
    H["go"] = sasin(h, sig)
    v0 = (T(0.726) * bm + T(0.812) * bm ** 2 + T(3.7) * bm ** 20) ** 2
    H["v"] = np.stack([v0, T(0.25) * v0, 4 * v0, 4 * v0], -1)
    H["s"] = T(0.626657069) * (T(0.265) * bn + T(1.194) * bn ** 2 + T(5.372) * bn ** 22)
    s2k = [np.sin(m["alpha"].astype(T) * T(np.pi / 180))]
    c2k = [np.sqrt(np.maximum(1 - s2k[0] ** 2, 0))]
    for i in (1, 2):
        s2k.append(2 * c2k[i - 1] * s2k[i - 1])
        c2k.append(c2k[i - 1] ** 2 - s2k[i - 1] ** 2)
    H["s2k"], H["c2k"] = s2k, c2k
    stt = H["sto"] / eta
    ctt = ssqrt(1 - stt ** 2, sig)
    with np.errstate(divide="ignore", invalid="ignore"):
        etap = np.sqrt(eta ** 2 - H["sto"] ** 2) / H["cto"]
        sgt = h / etap
    cgt = ssqrt(1 - sgt ** 2, sig)
    H["gt"] = sasin(sgt, sig)
    ln = 2 * cgt / ctt
    Tr = np.exp(-m["sigma"].astype(T) * ln[..., None])
    F = fresnel(H["cto"] * ssqrt(1 - h * h, sig), eta, sig)[..., None]
    A0 = F * np.ones_like(Tr)
    A1 = (1 - F) ** 2 * Tr
    A2 = A1 * Tr * F
    den = 1 - Tr * F
    ok = sig(den > 0)
    A3 = np.where(ok, A2 * F * Tr / np.where(ok, den, 1), 0)
    H["A"] = [A0, A1, A2, A3]
    return H


def tilt(H, p):
    st, ct = H["sto"], H["cto"]
    if p == 0:
        s, c = st * H["c2k"][1] - ct * H["s2k"][1], ct * H["c2k"][1] + st * H["s2k"][1]
    elif p == 3:
        s, c = st, ct
    else:
        k = 0 if p == 1 else 2
        s, c = st * H["c2k"][k] + ct * H["s2k"][k], ct * H["c2k"][k] - st * H["s2k"][k]
    return s, np.abs(c)


def lobes(H, U, V, W, wi, sig, T):
    sti = dot(wi, V)
    cti = ssqrt(1 - sti ** 2, sig)
    phi = np.arctan2(dot(wi, W), dot(wi, U)) - H["phio"]
    M, Nn = [], []
    for p in range(4):
        s, c = tilt(H, p)
        M.append(mp(cti, c, sti, s, H["v"][..., p], sig))
    for p in range(3):
        Nn.append(np_lobe(phi, p, H["s"], H["go"], H["gt"], sig, T))
    return M, Nn


def total(M, Nn, a, T):
    """S with the weights a[p] (each (n,) or (n, 3)) in place of A_p."""
    ex = (lambda x: x[..., None]) if a[0].ndim == 2 else (lambda x: x)
    return (ex(M[0] * Nn[0]) * a[0] + ex(M[1] * Nn[1]) * a[1] + ex(M[2] * Nn[2]) * a[2] +
            ex(M[3]) * a[3] / T(2 * np.pi))


def value(H, M, Nn, n, wi, sig, T):
    S = total(M, Nn, H["A"], T)
    c = np.abs(dot(wi, n))
    nz = sig(c != 0)
    return np.where(nz[..., None], S / np.where(nz, c, 1)[..., None], S)


def mats(eta, bm, bn, alpha, sigma, n):
    b = lambda x: np.broadcast_to(np.asarray(x, np.float64), (n,)).copy()
    return {"eta": b(eta), "bm": b(bm), "bn": b(bn), "alpha": b(alpha),
            "sigma": np.broadcast_to(np.asarray(sigma, np.float64), (n, 3)).copy()}


def hair_eval(m, U, V, W, n, wo, wi, T=np.float64):
    """f(w_o, w_i) and the signature."""
    U, V, W, n, wo, wi = (np.asarray(a).astype(T) for a in (U, V, W, n, wo, wi))
    sig = Sig()
    zero_v = sig((V == 0).all(-1))
    wo, wi = normalize(wo), normalize(wi)
    with np.errstate(all="ignore"):
        H = hit(m, U, V, W, n, wo, sig, T)
        M, Nn = lobes(H, U, V, W, wi, sig, T)
        f = value(H, M, Nn, n, wi, sig, T)
    f = np.where(zero_v[..., None], 0, f)
    return {"f": f, "sig": sig.rows(), "A": sum(H["A"])}


def hair_sample(m, U, V, W, n, wo, draws, T=np.float64):
    """The sample of the draws (u_l, u_n, u_0, u_1): out, pdf, f, valid, sum A_p and the signature."""
    U, V, W, n, wo, draws = (np.asarray(a).astype(T) for a in (U, V, W, n, wo, draws))
    pi = T(np.pi)
    sig = Sig()
    zero_v = sig((V == 0).all(-1))
    wo = normalize(wo)
    ul, un, u0, u1 = (draws[..., k] for k in range(4))
    with np.errstate(all="ignore"):
        H = hit(m, U, V, W, n, wo, sig, T)
        w = [a.sum(-1) for a in H["A"]]
        tot = w[0] + w[1] + w[2] + w[3]
        lit = sig(tot > 0)
        q = [x / np.where(lit, tot, 1) for x in w]
        p = np.full(ul.shape, 3)
        run = q[0] + q[1] + q[2]
        p = np.where(ul < run, 2, p)
        p = np.where(ul < q[0] + q[1], 1, p)
        p = np.where(ul < q[0], 0, p)
        sig(p)
        tl = [tilt(H, k) for k in range(4)]
        stp = np.choose(p, [t[0] for t in tl])
        ctp = np.choose(p, [t[1] for t in tl])
        vp = np.take_along_axis(H["v"], p[..., None], -1)[..., 0]
        sig(u0 < T(1e-5))
        u0 = np.maximum(u0, T(1e-5))
        ct = 1 + vp * np.log(u0 + (1 - u0) * np.exp(-2 / vp))
        st = ssqrt(1 - ct * ct, sig)
        sti = -ct * stp + st * np.cos(2 * pi * u1) * ctp
        cti = ssqrt(1 - sti * sti, sig)
        cm, cp = cdf(-pi, H["s"]), cdf(pi, H["s"])
        x = -H["s"] * np.log(1 / (un * (cp - cm) + cm) - 1)
        sig((x < -pi).astype(int) - (x > pi).astype(int))
        ph = np.choose(np.minimum(p, 2), [big_phi(k, H["go"], H["gt"], T) for k in range(3)])
        dphi = np.where(p < 3, ph + np.clip(x, -pi, pi), 2 * pi * un)
        phii = H["phio"] + dphi
        out = V * sti[..., None] + U * (cti * np.cos(phii))[..., None] + W * (cti * np.sin(phii))[..., None]
        wi = normalize(out)
        M, Nn = lobes(H, U, V, W, wi, sig, T)
        pdf = total(M, Nn, q, T)
        f = value(H, M, Nn, n, wi, sig, T)
    valid = lit & ~zero_v
    out = np.where(valid[..., None], out, np.asarray([0, 0, 1], T))
    return {"out": out, "pdf": np.where(valid, pdf, 0), "f": np.where(valid[..., None], f, 0), "valid": valid,
            "sig": sig.rows(), "A": sum(H["A"])}


def jitter(a, rng, ulps=2, lo=None, hi=None):
    """a (float32: unit vectors, or draws in [0, 1)) with every element moved by a whole number in
    [-ulps, ulps] of 2^-24, the float32 spacing just below the vector's length 1: a component that is
    exactly 0 moves too, as it does when float32 arithmetic produces the vector."""
    a = np.ascontiguousarray(a, F32)
    k = rng.integers(-ulps, ulps + 1, a.shape)
    b = (a.astype(np.float64) + k * 2.0 ** -24).astype(F32)
    return b if lo is None else np.clip(b, F32(lo), F32(hi))
