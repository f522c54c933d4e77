"""numpy float32 restatement of khp_denoise / khp_denoise_host (include/kirk_hip.h)
for the tests: what the definition says, operation by operation, and nothing of the kernels.

Every operation is one float32 operation in the definition's order (numpy keeps float32 for
float32 operands; sums of three are written (x*x + y*y) + z*z).  The 25 taps are a Python loop
in the definition's order, dy outer and dx inner; each tap is vectorised over the pixels it
exists for.  k_expf is kmath.h's, restated: floor, the two range-reduction multiplies, the
Horner steps each rounded to float32, and k_ldexpf's multiplications by exact powers of two.
"""
import numpy as np

F32 = np.float32
H5 = (F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625))
DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_normal=0.35, sigma_tangent=0.35, sigma_depth=0.05,
                sigma_coverage=0.25, clamp=0.0)


def _pow2(n):
    """f_from_bits((n + 127) << 23) for n in -126 .. 127: 2^n exactly."""
    return ((np.asarray(n, np.int64) + 127).astype(np.uint32) << np.uint32(23)).view(F32)


def k_ldexpf(x, n):
    """kmath.h k_ldexpf: x * 2^n by one or two float32 multiplications with exact powers of two."""
    x = np.asarray(x, F32)
    n = np.asarray(n, np.int64)
    hi, lo = n > 127, n < -126
    with np.errstate(all="ignore"):
        x = np.where(hi, x * _pow2(127), np.where(lo, x * _pow2(-126), x)).astype(F32)
        n = np.where(hi, np.minimum(n - 127, 127), np.where(lo, np.maximum(n + 126, -126), n))
        return (x * _pow2(n)).astype(F32)


def k_expf(x):
    """kmath.h k_expf on a float32 array."""
    x = np.asarray(x, F32)
    nan, big, small = np.isnan(x), x > F32(88.72283905206835), x < F32(-103.278929903431851103)
    a = np.where(nan | big | small, F32(0.0), x).astype(F32)
    with np.errstate(all="ignore"):
        z = np.floor(F32(1.44269504088896341) * a + F32(0.5))
        a = a - z * F32(0.693359375)
        a = a - z * F32(-2.12194440e-4)
        n = z.astype(np.int64)
        z = a * a
        z = (((((F32(1.9875691500E-4) * a + F32(1.3981999507E-3)) * a + F32(8.3334519073E-3)) * a
               + F32(4.1665795894E-2)) * a + F32(1.6666665459E-1)) * a + F32(5.0000001201E-1)) * z + a + F32(1.0)
        assert z.dtype == F32
        r = k_ldexpf(z, n)
    r = np.where(small, F32(0.0), np.where(big, F32(np.inf), r)).astype(F32)
    return np.where(nan, x, r).astype(F32)


def _d2(a, b):
    e = a - b
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def _unit(v, inv):
    n = v * inv[..., None]
    l = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    has = l > 0
    return np.where(has[..., None], n / np.where(has, l, F32(1.0))[..., None], F32(0.0)).astype(F32)


def _fin(c):
    return np.isfinite(c).all(-1)


def denoise(colour, guides, demodulate=False, **params):
    """The definition on an (H, W, 3) float32 frame; guides: dict of planes as khp_render_aov
    writes them (a plane whose term is off may be missing or None).  Returns a new (H, W, 3) array."""
    prm = dict(DEFAULTS)
    for k, v in params.items():
        assert k in prm, k
        prm[k] = v
    c = np.array(colour, F32)
    Hh, Ww = c.shape[:2]
    sig = {k: F32(prm["sigma_" + k]) for k in ("color", "normal", "tangent", "depth", "coverage")}
    on = {k: bool(s > 0) for k, s in sig.items()}
    with np.errstate(all="ignore"):
        inv_s = {k: (F32(1.0) / (s * s) if on[k] else F32(0.0)) for k, s in sig.items()}
        # ---- prepare
        reads_cov = on["normal"] or on["tangent"] or on["depth"] or on["coverage"] or demodulate
        cv = np.asarray(guides["coverage"], F32) if reads_cov else np.zeros((Hh, Ww), F32)
        inv = np.where(cv > 0, F32(1.0) / np.where(cv > 0, cv, F32(1.0)), F32(0.0)).astype(F32)
        n = _unit(np.asarray(guides["normal"], F32), inv) if on["normal"] else None
        t = _unit(np.asarray(guides["tangent"], F32), inv) if on["tangent"] else None
        d = (np.asarray(guides["depth"], F32) * inv).astype(F32) if on["depth"] else None
        clamp = F32(prm["clamp"])
        if clamp > 0:
            c = np.where(c > clamp, clamp, c).astype(F32)
        if demodulate:
            m = (np.asarray(guides["albedo"], F32) + (F32(1.0) - cv)[..., None]).astype(F32)
            m = np.where(m < F32(1e-3), F32(1e-3), m).astype(F32)          # gmax(m, 1e-3f)
            c = (c / m).astype(F32)
        # ---- iterate
        for it in range(int(prm["iterations"])):
            s = 1 << it
            fin = _fin(c)
            acc = np.zeros((Hh, Ww, 3), F32)
            ws = np.zeros((Hh, Ww), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * s, dx * s
                    y0, y1, x0, x1 = max(0, -oy), min(Hh, Hh - oy), max(0, -ox), min(Ww, Ww - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue                                           # the tap is outside for every pixel
                    P = (slice(y0, y1), slice(x0, x1))                     # the pixels that have this tap
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    X = np.zeros(ws[P].shape, F32)
                    if on["color"]:
                        X = np.where(fin[P], X + _d2(c[P], c[Q]) * inv_s["color"], X)
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
                    counts = fin[Q] & (w > 0)                              # a NaN weight fails the comparison
                    acc[P] = np.where(counts[..., None], acc[P] + w[..., None] * c[Q], acc[P])
                    ws[P] = np.where(counts, ws[P] + w, ws[P])
            has = ws > 0
            c = np.where(has[..., None], acc / np.where(has, ws, F32(1.0))[..., None], c).astype(F32)
        # ---- finish
        if demodulate:
            c = (c * m).astype(F32)
    return c


def bits(a):
    """An array's bits with every NaN made one pattern (an invalid operation's NaN differs
    between hosts and devices in sign and payload; no definition above depends on it)."""
    a = np.ascontiguousarray(a, F32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def random_case(width, height, seed, bad=True):
    """Seeded colours and guide planes shaped as khp_render_aov writes them: coverage in
    {0, 1/4, .., 1}, the other planes premultiplied by it.  With `bad`, some colour pixels are
    NaN, +inf, -inf and 1e38, one NaN pixel has only NaN neighbours (a 7 x 7 patch of NaN, where
    the frame has room).  The centre pixel has coverage 0 (every plane 0 there) among covered ones."""
    rng = np.random.default_rng(seed)
    shape = (height, width)
    cov = (rng.integers(0, 5, size=shape) / 4.0).astype(F32)
    unit = lambda: (lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True))(rng.normal(size=shape + (3,)))
    g = {"normal": (unit() * cov[..., None]).astype(F32),
         "albedo": (rng.random(shape + (3,)) * cov[..., None]).astype(F32),
         "tangent": (unit() * cov[..., None]).astype(F32),
         "depth": ((2.0 + rng.random(shape)) * cov).astype(F32),
         "coverage": cov}
    c = (rng.random(shape + (3,)) * 3.0).astype(F32)
    if bad and width * height > 1:
        flat = c.reshape(-1, 3)
        idx = rng.choice(width * height, size=min(8, width * height // 2), replace=False)
        for k, v in zip(idx, (np.nan, np.inf, -np.inf, 1e38, np.nan, np.inf, -np.inf, 1e38)):
            flat[k, rng.integers(0, 3)] = v
        if width >= 9 and height >= 9:
            c[1:8, 1:8] = np.nan
    if width * height > 1:
        y, x = height // 2, width // 2
        for ch in g:
            g[ch][y, x] = 0
    return c, g
