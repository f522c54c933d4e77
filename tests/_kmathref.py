"""csrc/kmath.h twice over, for tests/test_kmath_truth.py and tests/test_gpu_kmath.py.

Two things, kept apart:

* a *restatement*: every op of csrc/kmath_ops.h in numpy float32 / float64 / unsigned
  arithmetic, one rounding per statement, written from the text of kmath.h.  It is the
  fourth independent statement of these functions, after the g++ compile
  (khp_kmath_host), the gfx950 compile (khp_debug_kmath) and the oracle's C (ko_*).
  `apply(op, items)` takes and returns the entries' own (n, 3) uint64 words.
* a *truth*: float64 libm (numpy) for every float32 function, mpmath at 80 digits for
  k_j0 and the double log / exp / pow.  Nothing of the truth is derived from kmath.h.

Also the inputs both test files share: the strided walks of float32 bit patterns and the
lattices of branch thresholds and special values.
"""
import math

import numpy as np

F = np.float32
D = np.float64
U32 = np.uint32
U64 = np.uint64
M32 = U64(0xFFFFFFFF)

OPS = ("mul", "add", "div", "sqrt", "rsqrt", "muladd", "floor", "f2i", "f2u", "i2f", "u2f", "u642f", "d2i2d",
       "dmul", "dadd", "ddiv", "umulhi", "ldexpf", "sinf", "cosf", "atanf", "atan2f", "asinf", "acosf", "expf",
       "sinhf", "hypotf", "logf_d", "powf_d", "j0", "log_d", "exp_d", "pow_d", "lowbias32", "path_key",
       "draw_u32", "draw_u01", "dot", "cross", "normalize", "reflect", "refract", "rotate_rowvec", "angle",
       "faceforward", "gmin", "gmax", "gclamp")

PIF = F(3.14159265358979323846)
PIO2F = F(1.57079632679489661923)
PIO4F = F(0.785398163397448309616)
SINCOS_DOMAIN = F(8192.0) + F(2.0) * PIF   # beyond it the two compilers are not compared


# ---- words ---------------------------------------------------------------------------------
def fbits(x):
    return np.ascontiguousarray(x, F).view(U32)


def from_fbits(u):
    return np.ascontiguousarray(u, U32).view(F)


def dbits(x):
    return np.ascontiguousarray(x, D).view(U64)


def from_dbits(u):
    return np.ascontiguousarray(u, U64).view(D)


def items_f(*cols):
    """(n, 3) words of up to three float32 columns (the low half of each word)."""
    n = len(np.atleast_1d(cols[0]))
    w = np.zeros((n, 3), U64)
    for k, c in enumerate(cols):
        w[:, k] = fbits(np.broadcast_to(np.asarray(c, F), (n,))).astype(U64)
    return w


def items_u(*cols):
    """(n, 3) words of up to three unsigned integer columns."""
    n = len(np.atleast_1d(cols[0]))
    w = np.zeros((n, 3), U64)
    for k, c in enumerate(cols):
        w[:, k] = np.broadcast_to(np.asarray(c, U64), (n,))
    return w


def items_d(*cols):
    n = len(np.atleast_1d(cols[0]))
    w = np.zeros((n, 3), U64)
    for k, c in enumerate(cols):
        w[:, k] = dbits(np.broadcast_to(np.asarray(c, D), (n,)))
    return w


def items_v(six):
    """(n, 3) words of an (n, 6) float32 array: f0..f5 are the low and high halves of words 0, 1, 2."""
    b = fbits(six).astype(U64).reshape(-1, 6)
    return b[:, 0::2] | (b[:, 1::2] << U64(32))


def out_f(o, k=0):
    return from_fbits((o[:, k] & M32).astype(U32))


def out_d(o, k=0):
    return from_dbits(o[:, k])


def same_bits(a, b, kind):
    """Elementwise: equal bit for bit, or both NaN whatever the encoding.  kind: 'f', 'd' or 'u'
    over (n,) or (n, 3) output words."""
    a, b = np.asarray(a, U64), np.asarray(b, U64)
    eq = a == b
    if kind == "f":
        nan = lambda w: ((w & U64(0x7F800000)) == U64(0x7F800000)) & ((w & U64(0x007FFFFF)) != 0) & ((w >> U64(32)) == 0)
    elif kind == "d":
        nan = lambda w: ((w & U64(0x7FF0000000000000)) == U64(0x7FF0000000000000)) & ((w & U64(0x000FFFFFFFFFFFFF)) != 0)
    else:
        return eq
    return eq | (nan(a) & nan(b))


# ---- the restatement: float functions --------------------------------------------------------
def _pow2(n):
    return ((np.asarray(n, np.int64) + 127).astype(U32) << U32(23)).view(F)


def k_ldexpf(x, n):
    x = np.asarray(x, F)
    n = np.asarray(n, np.int64)
    hi, lo = n > 127, n < -126
    x = np.where(hi, x * _pow2(127), np.where(lo, x * _pow2(-126), x))
    n = np.where(hi, np.minimum(n - 127, 127), np.where(lo, np.maximum(n + 126, -126), n))
    return x * _pow2(n)


def _sin_poly(z, x):
    y = ((F(-1.9515295891E-4) * z + F(8.3321608736E-3)) * z - F(1.6666654611E-1)) * z
    y = y * x
    return y + x


def _cos_poly(z):
    y = ((F(2.443315711809948E-005) * z - F(1.388731625493765E-003)) * z + F(4.166664568298827E-002)) * z
    y = y * z
    y = y - F(0.5) * z
    return y + F(1.0)


DP1, DP2, DP3, FOPI = F(0.78515625), F(2.4187564849853515625e-4), F(3.77489497744594108e-8), F(1.27323954473516)
DP3A, DP3B = F(float.fromhex("0x1.444p-25")), F(float.fromhex("0x1.68c234p-40"))


def _octant(ax, second_take=True):
    """j, y and the reduced argument of |x|, as k_sinf and k_cosf begin.  (int) of a product that
    leaves int's range is not defined by the source: such items get j = 0 here and are compared nowhere."""
    t = FOPI * ax
    j = np.where(t < F(2147483648.0), t, F(0.0)).astype(np.int32).astype(np.int64)
    y = j.astype(F)
    odd = (j & 1) != 0
    j = np.where(odd, j + 1, j)
    y = np.where(odd, y + F(1.0), y)
    j = j & 7
    r2 = ax - y * DP1
    r2 = r2 - y * DP2
    r = r2 - y * DP3
    tiny = r2 - y * DP3A          # k_reduce: below 2^-20 the reduction is taken again with DP3 in two parts
    tiny = tiny - y * DP3B
    return j, (np.where(np.abs(r) < F(2.0 ** -20), tiny, r) if second_take else r), r


def k_sinf(x, second_take=True):
    """second_take=False: the three-constant reduction alone, as kmath.h had it before k_reduce."""
    x = np.asarray(x, F)
    neg = x < F(0.0)
    j, r, _ = _octant(np.where(neg, -x, x), second_take)
    hi = j > 3
    neg = neg ^ hi
    j = np.where(hi, j - 4, j)
    z = r * r
    y = np.where((j == 1) | (j == 2), _cos_poly(z), _sin_poly(z, r))
    return np.where(np.isnan(x), x, np.where(neg, -y, y))


def k_cosf(x, second_take=True):
    x = np.asarray(x, F)
    j, r, _ = _octant(np.where(x < F(0.0), -x, x), second_take)
    hi = j > 3
    j = np.where(hi, j - 4, j)
    neg = hi ^ (j > 1)
    z = r * r
    y = np.where((j == 1) | (j == 2), _sin_poly(z, r), _cos_poly(z))
    return np.where(np.isnan(x), x, np.where(neg, -y, y))


def k_atanf(x):
    x = np.asarray(x, F)
    neg = x < F(0.0)
    a = np.where(neg, -x, x)
    big = a > F(2.414213562373095)
    mid = ~big & (a > F(0.4142135623730950))
    y = np.where(big, PIO2F, np.where(mid, PIO4F, F(0.0)))
    r = np.where(big, -(F(1.0) / a), np.where(mid, (a - F(1.0)) / (a + F(1.0)), a))
    z = r * r
    p = (((F(8.05374449538e-2) * z - F(1.38776856032E-1)) * z + F(1.99777106478E-1)) * z - F(3.33329491539E-1)) * z
    p = p * r
    p = p + r
    y = y + p
    return np.where(neg, -y, y)


def k_atan2f(y, x):
    y, x = np.asarray(y, F), np.asarray(x, F)
    xneg, yneg = x < F(0.0), y < F(0.0)
    w = np.where(xneg & ~yneg, PIF, np.where(xneg & yneg, -PIF, F(0.0)))
    r = w + k_atanf(y / x)
    r = np.where(y == F(0.0), np.where(xneg, PIF, F(0.0)), r)
    r = np.where(x == F(0.0), np.where(yneg, -PIO2F, np.where(y == F(0.0), F(0.0), PIO2F)), r)
    return np.where(np.isnan(x) | np.isnan(y), x + y, r)


def k_asinf(x):
    x = np.asarray(x, F)
    neg = x < F(0.0)
    a = np.where(neg, -x, x)
    flag = a > F(0.5)
    zf = F(0.5) * (F(1.0) - a)
    xx = np.where(flag, np.sqrt(zf), a)
    z = np.where(flag, zf, xx * xx)
    p = ((((F(4.2163199048E-2) * z + F(2.4181311049E-2)) * z + F(4.5470025998E-2)) * z + F(7.4953002686E-2)) * z
         + F(1.6666752422E-1)) * z
    p = p * xx
    p = p + xx
    p2 = p + p
    p = np.where(flag, PIO2F - p2, p)
    p = np.where(a < F(1.0e-4), a, p)
    p = np.where(neg, -p, p)
    p = np.where(a > F(1.0), F(np.nan), p)
    return np.where(np.isnan(x), x, p)


def k_acosf(x):
    x = np.asarray(x, F)
    lo = PIF - F(2.0) * k_asinf(np.sqrt(F(0.5) * (F(1.0) + x)))
    hi = F(2.0) * k_asinf(np.sqrt(F(0.5) * (F(1.0) - x)))
    r = np.where(x < F(-0.5), lo, np.where(x > F(0.5), hi, PIO2F - k_asinf(x)))
    r = np.where((x < F(-1.0)) | (x > F(1.0)), F(np.nan), r)
    return np.where(np.isnan(x), x, r)


EXP_HI, EXP_LO = F(88.72283905206835), F(-103.278929903431851103)


def k_expf(x):
    x = np.asarray(x, F)
    big, small = x > EXP_HI, x < EXP_LO
    a = np.where(big | small | np.isnan(x), F(0.0), x)
    z = np.floor(F(1.44269504088896341) * a + F(0.5))
    a = a - z * F(0.693359375)
    a = a - z * F(-2.12194440e-4)
    n = z.astype(np.int64)
    z = a * a
    p = (((((F(1.9875691500E-4) * a + F(1.3981999507E-3)) * a + F(8.3334519073E-3)) * a + F(4.1665795894E-2)) * a
          + F(1.6666665459E-1)) * a + F(5.0000001201E-1)) * z
    p = p + a
    p = p + F(1.0)
    r = k_ldexpf(p, n)
    r = np.where(small, F(0.0), np.where(big, F(np.inf), r))
    return np.where(np.isnan(x), x, r)


def k_sinhf(x):
    x = np.asarray(x, F)
    neg = x < F(0.0)
    a = np.where(neg, -x, x)
    e = k_expf(a)
    big = F(0.5) * e - (F(0.5) / e)
    big = np.where(neg, -big, big)
    z = x * x
    p = ((F(2.03721912945E-4) * z + F(8.33028376239E-3)) * z + F(1.66667160211E-1)) * z
    p = p * x
    p = p + x
    return np.where(a > F(1.0), big, p)


def k_hypotf(x, y):
    x, y = np.asarray(x, F), np.asarray(y, F)
    return np.sqrt(x * x + y * y)


# ---- the restatement: double functions -------------------------------------------------------
def k_j0(x):
    x = np.asarray(x, D)
    q = D(-0.25) * x * x
    term = np.ones_like(x)
    s = np.ones_like(x)
    for k in range(1, 41):
        term = term * q / (D(k) * D(k))
        s = s + term
    return s


LN2_HI_D, LN2_LO_D, INV_LN2_D = D(6.93147180369123816490e-01), D(1.90821492927058770002e-10), D(1.44269504088896338700e+00)
DINF, DNAN = D(np.inf), D(np.nan)


def _dpow2(k):
    return ((np.asarray(k, np.int64) + 1023).astype(U64) << U64(52)).view(D)


def k_log_d(x):
    x = np.asarray(x, D)
    pos = x > 0.0
    a = np.where(pos & (x != DINF), x, D(1.0))
    sub = a < D(2.2250738585072014e-308)
    a = np.where(sub, a * D(18014398509481984.0), a)
    e = np.where(sub, -54, 0).astype(np.int64)
    b = dbits(a)
    e = e + ((b >> U64(52)) & U64(0x7FF)).astype(np.int64) - 1023
    m = from_dbits((b & U64(0x000FFFFFFFFFFFFF)) | U64(0x3FF0000000000000))
    fold = m > D(1.41421356237309504880)
    m = np.where(fold, m * D(0.5), m)
    e = np.where(fold, e + 1, e)
    f = m - D(1.0)
    s = f / (m + D(1.0))
    z = s * s
    p = D(1.0) / D(25.0)
    for d in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * z
        p = p + D(1.0) / D(d)
    s2 = D(2.0) * s
    lm = s2 + s2 * (z * p)
    de = e.astype(D)
    r = de * LN2_HI_D + (de * LN2_LO_D + lm)
    r = np.where(x == DINF, x, r)
    return np.where(pos, r, np.where(x == 0.0, -DINF, DNAN))


_EXP_COEF = (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0)


def k_exp_d(x):
    x = np.asarray(x, D)
    big, small, nan = x > D(709.782712893384), x < D(-745.2), np.isnan(x)
    a = np.where(big | small | nan, D(0.0), x)
    kd = np.trunc(a * INV_LN2_D + np.where(a < 0.0, D(-0.5), D(0.5)))
    k = kd.astype(np.int64)
    r = (a - kd * LN2_HI_D) - kd * LN2_LO_D
    p = D(1.0) / D(87178291200.0)
    for c in _EXP_COEF:
        p = p * r
        p = p + D(1.0) / D(c)
    for c in (D(0.5), D(1.0), D(1.0)):
        p = p * r
        p = p + c
    lo, hi = k < -1021, k > 1023
    r_lo = (p * _dpow2(np.where(lo, k + 54, 0))) * (D(1.0) / D(18014398509481984.0))
    r_hi = (p * D(2.0)) * _dpow2(np.where(hi, k - 1, 0))
    r_mid = p * _dpow2(np.where(lo | hi, 0, k))
    res = np.where(lo, r_lo, np.where(hi, r_hi, r_mid))
    res = np.where(small, D(0.0), np.where(big, DINF, res))
    return np.where(nan, x, res)


_TWO53 = D(9007199254740992.0)


def k_pow_d(x, y):
    x, y = np.asarray(x, D), np.asarray(y, D)
    huge = (y > _TWO53) | (y < -_TWO53)
    ysafe = np.where(huge | ~np.isfinite(y), D(0.0), y)
    yi = np.trunc(ysafe)
    is_int = (ysafe == yi) | huge
    odd = ~huge & (ysafe == yi) & ((yi.astype(np.int64) & 1) != 0) & np.isfinite(y)
    ax = np.where(x < 0.0, -x, x)
    xneg_bit = (dbits(x) >> U64(63)) != 0
    fin = np.isfinite(ax) & (ax > 0.0)
    r = k_exp_d(y * k_log_d(np.where(fin, ax, D(1.0))))
    res = np.where(x < 0.0, np.where(is_int, np.where(odd, -r, r), DNAN), r)
    at_inf = np.where(x > 0.0, np.where(y < 0.0, D(0.0), DINF),
                      np.where(y < 0.0, np.where(odd, D(-0.0), D(0.0)), np.where(odd, -DINF, DINF)))
    res = np.where(ax == DINF, at_inf, res)
    at_zero = np.where(y < 0.0, np.where(odd & xneg_bit, -DINF, DINF), np.where(odd & xneg_bit, x, D(0.0)))
    res = np.where(x == 0.0, at_zero, res)
    y_inf = np.where(ax == 1.0, D(1.0), np.where((ax > 1.0) == (y > 0.0), DINF, D(0.0)))
    res = np.where((y == DINF) | (y == -DINF), y_inf, res)
    res = np.where(np.isnan(x) | np.isnan(y), DNAN, res)
    return np.where((y == 0.0) | (x == 1.0), D(1.0), res)


def k_logf_d(x):
    return k_log_d(np.asarray(x, F).astype(D)).astype(F)


def k_powf_d(x, y):
    return k_pow_d(np.asarray(x, F).astype(D), np.asarray(y, F).astype(D)).astype(F)


# ---- the restatement: integers -----------------------------------------------------------------
def lowbias32(x):
    x = np.asarray(x, U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x7FEB352D)
    x ^= x >> U32(15)
    x *= U32(0x846CA68B)
    x ^= x >> U32(16)
    return x


def path_key(seed, pixel, sample):
    seed, pixel, sample = (np.asarray(a, U32) for a in (seed, pixel, sample))
    return lowbias32(lowbias32(lowbias32(seed ^ U32(0x4B49524B)) ^ pixel) + sample * U32(0x9E3779B9))


def draw_u32(key, dim):
    key, dim = np.asarray(key, U32), np.asarray(dim, U32)
    return lowbias32(key ^ (dim * U32(0x85EBCA6B) + U32(0x632BE5AB)))


def draw_u01(key, dim):
    return (draw_u32(key, dim) >> U32(8)).astype(F) * F(1.0 / 16777216.0)


def umulhi(a, b):
    """The high 64 bits of a 64 x 64 product, by 32-bit limbs."""
    a, b = np.asarray(a, U64), np.asarray(b, U64)
    al, ah, bl, bh = a & M32, a >> U64(32), b & M32, b >> U64(32)
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> U64(32)) + (lh & M32) + (hl & M32)
    return hh + (lh >> U64(32)) + (hl >> U64(32)) + (mid >> U64(32))


# ---- the restatement: algebra (columns of float32) ------------------------------------------------
def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def normalize(a):
    s = F(1.0) / np.sqrt(dot(a, a))
    return (a[0] * s, a[1] * s, a[2] * s)


def gmin(x, y):
    return np.where(y < x, y, x)


def gmax(x, y):
    return np.where(x < y, y, x)


def gclamp(x, lo, hi):
    return gmin(gmax(x, lo), hi)


def reflect(i, n):
    d = dot(n, i)
    return tuple(i[k] - (n[k] * d) * F(2.0) for k in range(3))


def refract(i, n, eta):
    d = dot(n, i)
    k = F(1.0) - eta * eta * (F(1.0) - d * d)
    s = eta * d + np.sqrt(k)
    ok = k >= F(0.0)
    return tuple(np.where(ok, i[c] * eta - n[c] * s, F(0.0)) for c in range(3))


def rotate_rowvec(d, ang, axis):
    c, s = k_cosf(ang), k_sinf(ang)
    a = normalize(axis)
    omc = F(1.0) - c
    t = (a[0] * omc, a[1] * omc, a[2] * omc)
    r00, r01, r02 = c + t[0] * a[0], t[0] * a[1] + s * a[2], t[0] * a[2] - s * a[1]
    r10, r11, r12 = t[1] * a[0] - s * a[2], c + t[1] * a[1], t[1] * a[2] + s * a[0]
    r20, r21, r22 = t[2] * a[0] + s * a[1], t[2] * a[1] - s * a[0], c + t[2] * a[2]
    return ((r00 * d[0] + r01 * d[1]) + r02 * d[2], (r10 * d[0] + r11 * d[1]) + r12 * d[2],
            (r20 * d[0] + r21 * d[1]) + r22 * d[2])


def angle(x, y):
    return k_acosf(gclamp(dot(x, y), F(-1.0), F(1.0)))


def faceforward(n, i, nref):
    keep = dot(nref, i) < F(0.0)
    return tuple(np.where(keep, n[k], -n[k]) for k in range(3))


# ---- apply: the op table over the entries' own words ------------------------------------------------
def _lo(w, k):
    return from_fbits((w[:, k] & M32).astype(U32))


def _hi(w, k):
    return from_fbits((w[:, k] >> U64(32)).astype(U32))


def _wf(*cols):
    o = np.zeros((len(cols[0]), 3), U64)
    for k, c in enumerate(cols):
        o[:, k] = fbits(np.asarray(c, F)).astype(U64)
    return o


def _w64(c):
    o = np.zeros((len(c), 3), U64)
    o[:, 0] = c
    return o


def apply(op, w):
    """The restatement of op (a name of OPS) over (n, 3) uint64 words; returns (n, 3) words."""
    w = np.ascontiguousarray(w, U64)
    a, b, c = _lo(w, 0), _lo(w, 1), _lo(w, 2)
    ua, ub, uc = ((w[:, k] & M32).astype(U32) for k in range(3))
    da, db = from_dbits(w[:, 0]), from_dbits(w[:, 1])
    p = (_lo(w, 0), _hi(w, 0), _lo(w, 1))
    q = (_hi(w, 1), _lo(w, 2), _hi(w, 2))
    with np.errstate(all="ignore"):
        if op == "mul": return _wf(a * b)
        if op == "add": return _wf(a + b)
        if op == "div": return _wf(a / b)
        if op == "sqrt": return _wf(np.sqrt(a))
        if op == "rsqrt": return _wf(F(1.0) / np.sqrt(a))
        if op == "muladd":
            t = a * b
            return _wf(t + c)
        if op == "floor": return _wf(np.floor(a))
        if op == "f2i": return _w64(a.astype(np.int32).view(U32).astype(U64))
        if op == "f2u": return _w64(a.astype(np.int64).astype(U32).astype(U64))
        if op == "i2f": return _wf(ua.view(np.int32).astype(F))
        if op == "u2f": return _wf(ua.astype(F))
        if op == "u642f": return _wf(w[:, 0].astype(F))
        if op == "d2i2d": return _w64(dbits(da.astype(np.int64).astype(D)))
        if op == "dmul": return _w64(dbits(da * db))
        if op == "dadd": return _w64(dbits(da + db))
        if op == "ddiv": return _w64(dbits(da / db))
        if op == "umulhi": return _w64(umulhi(w[:, 0], w[:, 1]))
        if op == "ldexpf": return _wf(k_ldexpf(a, ub.view(np.int32)))
        if op == "sinf": return _wf(k_sinf(a))
        if op == "cosf": return _wf(k_cosf(a))
        if op == "atanf": return _wf(k_atanf(a))
        if op == "atan2f": return _wf(k_atan2f(a, b))
        if op == "asinf": return _wf(k_asinf(a))
        if op == "acosf": return _wf(k_acosf(a))
        if op == "expf": return _wf(k_expf(a))
        if op == "sinhf": return _wf(k_sinhf(a))
        if op == "hypotf": return _wf(k_hypotf(a, b))
        if op == "logf_d": return _wf(k_logf_d(a))
        if op == "powf_d": return _wf(k_powf_d(a, b))
        if op == "j0": return _w64(dbits(k_j0(da)))
        if op == "log_d": return _w64(dbits(k_log_d(da)))
        if op == "exp_d": return _w64(dbits(k_exp_d(da)))
        if op == "pow_d": return _w64(dbits(k_pow_d(da, db)))
        if op == "lowbias32": return _w64(lowbias32(ua).astype(U64))
        if op == "path_key": return _w64(path_key(ua, ub, uc).astype(U64))
        if op == "draw_u32": return _w64(draw_u32(ua, ub).astype(U64))
        if op == "draw_u01": return _wf(draw_u01(ua, ub))
        if op == "dot": return _wf(dot(p, q))
        if op == "cross": return _wf(*cross(p, q))
        if op == "normalize": return _wf(*normalize(p))
        if op == "reflect": return _wf(*reflect(p, q))
        if op == "refract": return _wf(*refract(p, q, q[2]))
        if op == "rotate_rowvec": return _wf(*rotate_rowvec(p, q[0], (q[1], q[2], p[2])))
        if op == "angle": return _wf(angle(p, q))
        if op == "faceforward": return _wf(*faceforward(p, q, p))
        if op == "gmin": return _wf(gmin(a, b))
        if op == "gmax": return _wf(gmax(a, b))
        if op == "gclamp": return _wf(gclamp(a, b, c))
    raise KeyError(op)


# the type of each op's output words, for same_bits
KIND = {op: "f" for op in OPS}
KIND.update({op: "d" for op in ("d2i2d", "dmul", "dadd", "ddiv", "j0", "log_d", "exp_d", "pow_d")})
KIND.update({op: "u" for op in ("f2i", "f2u", "umulhi", "lowbias32", "path_key", "draw_u32")})


# ---- the truth ---------------------------------------------------------------------------------------
def ulp32(got, want):
    """|got - want| in units of the float32 spacing at want (float64 truth); 1e-45 at want = 0."""
    got, want = np.asarray(got, F).astype(D), np.asarray(want, D)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.abs(want).astype(F)).astype(D)
        sp = np.where(want == 0.0, D(1e-45), sp)
        return np.abs(got - want) / sp


def mp_truth(fn, xs, ys=None):
    """fn of mpmath (a name) over float64 arguments at 80 digits; returns mpf values."""
    import mpmath
    mpmath.mp.dps = 80
    f = {"j0": lambda x: mpmath.besselj(0, x), "log": mpmath.log, "exp": mpmath.exp,
         "pow": lambda x, y: mpmath.power(x, y)}[fn]
    if ys is None:
        return [f(mpmath.mpf(float(x))) for x in xs]
    return [f(mpmath.mpf(float(x)), mpmath.mpf(float(y))) for x, y in zip(xs, ys)]


def ulp64_mp(got, want):
    """Each |got - want| in units of the float64 spacing at want, want an mpf."""
    import mpmath
    out = []
    for g, t in zip(np.asarray(got, D), want):
        sp = np.spacing(abs(float(t))) if t != 0 else 5e-324
        out.append(float(abs(mpmath.mpf(float(g)) - t) / mpmath.mpf(float(sp))))
    return np.array(out)


# ---- inputs --------------------------------------------------------------------------------------------
def _next_prime(n):
    n = max(int(n), 2)
    while any(n % k == 0 for k in range(2, int(math.isqrt(n)) + 1)):
        n += 1
    return n


def walk(hi, lo=0.0, target=1 << 20):
    """The float32 bit patterns of [lo, hi] walked with a prime stride, then the same with the sign set:
    between target / 2 and target items in all (the stride is the first prime that fits them)."""
    b0, b1 = int(fbits(F(lo))[0]), int(fbits(F(hi))[0])
    stride = _next_prime(-(-2 * (b1 - b0 + 1) // target))
    pos = np.arange(b0, b1 + 1, stride, dtype=np.int64).astype(U32)
    return from_fbits(np.concatenate([pos, pos | U32(0x80000000)])), stride


def neighbours(values, k=3):
    """Each float32 value with the k floats on either side (by bit pattern, within its sign)."""
    v = fbits(np.asarray(values, F)).astype(np.int64)
    out = (v[:, None] + np.arange(-k, k + 1)[None, :]).ravel()
    mag = out & 0x7FFFFFFF
    ok = ((out >= 0) & (out <= 0xFFFFFFFF)) & (((out ^ np.repeat(v, 2 * k + 1)) & 0x80000000) == 0) & (mag <= 0x7F800000)
    return from_fbits(out[ok].astype(U32))


SPECIALS = from_fbits(np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,
                                0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000],
                               U32))
THRESHOLDS = np.array([0.4142135623730950, 2.414213562373095, 1e-4, 0.5, 1.0, 88.72283905206835,
                       -103.278929903431851103, 1.41421356237309504880, 12.0, 8192.0, float(SINCOS_DOMAIN)], D).astype(F)


def first_subnormal_exp_arg():
    """The largest float32 x whose exp(x) is below FLT_MIN, by the truth: the first argument with a subnormal result."""
    x = F(math.log(1.1754943508222875e-38))
    while math.exp(float(x)) >= 1.1754943508222875e-38:
        x = np.nextafter(x, F(-np.inf))
    return x


def octant_lattice(kmax=10431):
    """Every octant boundary k pi / 4, k = 0..kmax, with the 3 floats on either side, both signs."""
    k = np.arange(0, kmax + 1, dtype=D)
    v = neighbours((k * (math.pi / 4.0)).astype(F))
    return np.concatenate([v, -v])


def lattice():
    """Branch thresholds of kmath.h with their neighbours (both signs), and the special values."""
    t = np.concatenate([THRESHOLDS, -THRESHOLDS, [first_subnormal_exp_arg()]]).astype(F)
    return np.concatenate([neighbours(t), neighbours(SPECIALS[:10], 2), SPECIALS]).astype(F)


def exponent_pairs(rng, n):
    """n float32 pairs over all exponent combinations (subnormals included): random sign, exponent and mantissa."""
    def col():
        e = rng.integers(0, 255, n, dtype=np.uint32)
        m = rng.integers(0, 1 << 23, n, dtype=np.uint32)
        s = rng.integers(0, 2, n, dtype=np.uint32)
        return from_fbits((s << U32(31)) | (e << U32(23)) | m)
    return col(), col()


def axis_pairs():
    """(y, x) on the axes with every sign of zero, and the special values against one another."""
    z = np.array([0.0, -0.0], F)
    v = np.concatenate([z, SPECIALS, np.array([1.0, -1.0, 0.5, -2.0, 3.0], F)])
    yy, xx = np.meshgrid(v, v, indexing="ij")
    return yy.ravel().astype(F), xx.ravel().astype(F)


# ---- the items of each op: (lattice, walk) as (n, 3) words, the same for every test ------------------------
POW_C99 = [(np.nan, 0.0), (1.0, np.nan), (0.0, -1.0), (-0.0, -1.0), (-0.0, 3.0), (0.0, 0.5), (-1.0, np.inf),
           (0.5, -np.inf), (2.0, -np.inf), (0.5, np.inf), (-np.inf, -3.0), (-np.inf, 3.0), (-np.inf, 2.0),
           (np.inf, -0.5), (-2.0, 3.0), (-2.0, 2.0), (-8.0, 1.0 / 3.0), (2.0, 10.0)]
UNARY_HI = {"sinf": float(SINCOS_DOMAIN), "cosf": float(SINCOS_DOMAIN), "atanf": 3.4028234663852886e38, "asinf": 1.0,
            "acosf": 1.0, "expf": 104.0, "sinhf": 89.0, "logf_d": 3.4028234663852886e38, "sqrt": 3.4028234663852886e38,
            "rsqrt": 3.4028234663852886e38, "floor": 3.4028234663852886e38, "f2i": 2147483520.0, "f2u": 4294967040.0}
WALK_STRIDE = {}
_CACHE = {}


def _rand_u64(rng, n):
    """uint64 of every bit length, so that the low and the high roundings both occur."""
    v = rng.integers(0, 1 << 63, n, dtype=np.uint64) * U64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return v >> rng.integers(0, 64, n, dtype=np.uint64)


def _rand_d(rng, n, emax=2046):
    """float64 of random sign, exponent field in [0, emax] and mantissa."""
    e = rng.integers(0, emax + 1, n, dtype=np.uint64)
    m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    s = rng.integers(0, 2, n, dtype=np.uint64)
    return from_dbits((s << U64(63)) | (e << U64(52)) | m)


def _dneigh(v, k=3):
    b = dbits(np.asarray(v, D)).astype(np.int64)
    return from_dbits((b[:, None] + np.arange(-k, k + 1)[None, :]).ravel().astype(U64))


DSPECIALS = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308,
                      -1.7976931348623157e308, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0], D)


def inputs(op):
    """(lattice, walk): the (n, 3) words every test of `op` runs, seeded by the op's number."""
    if op in _CACHE:
        return _CACHE[op]
    rng = np.random.default_rng(1000 + OPS.index(op))
    n = 1 << 19
    if op in UNARY_HI:
        w, WALK_STRIDE[op] = walk(UNARY_HI[op])
        lat = lattice()
        if op in ("sinf", "cosf"):
            lat = np.concatenate([lat, octant_lattice()])
        if op == "expf":  # the band of subnormal results is narrow in bit patterns: a denser walk of its own
            w = np.concatenate([w, -from_fbits(np.arange(int(fbits(F(87.3))[0]), int(fbits(F(103.3))[0]), 31, dtype=np.int64)
                                               .astype(U32))])
        if op == "f2i":   # in-range arguments only
            lat = lat[np.abs(lat) < F(2147483648.0)]
        if op == "f2u":
            lat = lat[(lat > F(-1.0)) & (lat < F(4294967296.0))]
            w = w[(w > F(-1.0))]
        res = items_f(lat), items_f(w)
    elif op in ("mul", "add", "div", "atan2f", "hypotf", "powf_d", "gmin", "gmax"):
        a, b = exponent_pairs(rng, n)
        ua, ub = rng.random(n, dtype=F), rng.random(n, dtype=F)
        sg = np.where(rng.integers(0, 2, n) == 1, F(-1.0), F(1.0))
        ya, xa = axis_pairs()
        if op == "powf_d":
            c = np.array(POW_C99, F)
            ya, xa = np.concatenate([ya, c[:, 0]]), np.concatenate([xa, c[:, 1]])
            ub = ub * F(8.0) - F(4.0)   # moderate exponents: |y log x| stays far below 40
            ua = ua * F(50.0)
        ta, tb = exponent_pairs(rng, 1 << 14)   # both operands tiny: subnormal sums and quotients
        ta, tb = from_fbits(fbits(ta) & U32(0x81FFFFFF)), from_fbits(fbits(tb) & U32(0x81FFFFFF))
        res = items_f(ya, xa), items_f(np.concatenate([a, ua * sg, ta]), np.concatenate([b, ub, tb]))
    elif op in ("muladd", "gclamp"):
        a, b = exponent_pairs(rng, n)
        c, _ = exponent_pairs(rng, n)
        a2 = (rng.random(n, dtype=F) + F(0.5)) * _pow2(rng.integers(-20, 21, n))
        b2 = (rng.random(n, dtype=F) + F(0.5)) * _pow2(rng.integers(-20, 21, n))
        c2 = -(a2 * b2)   # c ~ -a b: the fused result is the product's rounding error, the unfused one is 0
        v = np.concatenate([SPECIALS, np.array([1.0, -1.0, 0.5], F)])
        g = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
        res = items_f(g[:, 0], g[:, 1], g[:, 2]), items_f(np.concatenate([a, a2]), np.concatenate([b, b2]),
                                                          np.concatenate([c, c2]))
    elif op == "ldexpf":
        a, _ = exponent_pairs(rng, n)
        k = rng.integers(-300, 301, n).astype(np.int32)
        edge = np.array([127, 128, 254, 255, -126, -127, -252, -253, 0, 2147483647, -2147483648, 1000, -1000], np.int32)
        xs = np.concatenate([SPECIALS, np.array([1.0, 1.5, -1.5], F)])
        gx, gk = np.meshgrid(xs, edge, indexing="ij")
        res = (items_u(fbits(gx.ravel()), gk.ravel().view(U32)), items_u(fbits(a), k.view(U32)))
    elif op in ("i2f", "u2f", "u642f"):
        edge = np.array([0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 25) + 2,
                         (1 << 25) + 6, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, (1 << 40) + (1 << 16),
                         (1 << 40) + (1 << 16) + 1, 0xFFFFFF7FFFFFFFFF, 0xFFFFFF8000000000, 0xFFFFFFFFFFFFFFFF], U64)
        r = _rand_u64(rng, n)
        if op != "u642f":
            edge, r = edge & M32, r & M32
        res = items_u(edge), items_u(r)
    elif op == "d2i2d":
        d = _rand_d(rng, n, emax=1023 + 62)
        edge = np.array([0.0, -0.0, 0.5, -0.5, 0.99999999999999989, 1.0, -1.5, 2.5, 4503599627370495.5, 4503599627370496.0,
                         9007199254740993.0, -9223372036854775808.0, 9223372036854774784.0], D)
        res = items_d(edge), items_d(d)
    elif op in ("dmul", "dadd", "ddiv"):
        g = np.stack(np.meshgrid(DSPECIALS, DSPECIALS, indexing="ij"), -1).reshape(-1, 2)
        res = items_d(g[:, 0], g[:, 1]), items_d(_rand_d(rng, n), _rand_d(rng, n))
    elif op == "umulhi":
        edge = np.array([0, 1, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000], U64)
        g = np.stack(np.meshgrid(edge, edge, indexing="ij"), -1).reshape(-1, 2)
        u24 = rng.integers(0, 1 << 24, n, dtype=np.uint64) << U64(40)   # env_scale_u24's own first operand
        res = items_u(g[:, 0], g[:, 1]), items_u(np.concatenate([_rand_u64(rng, n), u24]),
                                                 np.concatenate([_rand_u64(rng, n), _rand_u64(rng, n)]))
    elif op == "j0":
        w, WALK_STRIDE[op] = walk(20.0)
        res = items_d(np.concatenate([DSPECIALS, _dneigh([6.0, -6.0, 2.404825557695773])])), \
            items_d(np.concatenate([w.astype(D), rng.uniform(-6.0, 6.0, n)]))
    elif op == "log_d":
        w, WALK_STRIDE[op] = walk(3.4028234663852886e38)
        lat = np.concatenate([DSPECIALS, _dneigh([1.41421356237309504880, 1.0, 0.5, 2.0, 2.2250738585072014e-308,
                                                  0.70710678118654752])])
        res = items_d(lat), items_d(np.concatenate([w.astype(D), np.abs(_rand_d(rng, n))]))
    elif op == "exp_d":
        w, WALK_STRIDE[op] = walk(746.0)
        ln2 = 0.6931471805599453
        lat = np.concatenate([DSPECIALS, _dneigh([709.782712893384, -745.2, -1021.0 * ln2, -1021.5 * ln2, -1022.0 * ln2,
                                                  -1020.5 * ln2, 1023.0 * ln2, 1023.5 * ln2, 1022.5 * ln2, -708.4, 0.5 * ln2,
                                                  -0.5 * ln2])])
        res = items_d(lat), items_d(np.concatenate([w.astype(D), rng.uniform(-746.0, 710.0, n)]))
    elif op == "pow_d":
        c = np.array(POW_C99, D)
        v = np.concatenate([DSPECIALS, [2.0, -2.0, 0.5, -0.5, 3.0, -3.0, 1e300, 9007199254740993.0, 1e19, -1e19]])
        g = np.stack(np.meshgrid(v, v, indexing="ij"), -1).reshape(-1, 2)
        x = np.concatenate([rng.uniform(1e-4, 50.0, n // 2), np.exp(rng.uniform(-700, 700, n // 2))])
        y = np.concatenate([rng.uniform(-4.0, 4.0, n // 2), rng.uniform(-1.5, 1.5, n // 2)])
        neg = rng.integers(0, 8, n) == 0   # an eighth with a negative base and an integer exponent
        x = np.where(neg, -x, x)
        y = np.where(neg, np.round(y * 8.0), y)
        res = items_d(np.concatenate([c[:, 0], g[:, 0]]), np.concatenate([c[:, 1], g[:, 1]])), items_d(x, y)
    elif op in ("lowbias32", "path_key", "draw_u32", "draw_u01"):
        edge = np.array([0, 1, 0x4B49524B, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], U64)
        g = np.stack(np.meshgrid(edge, edge, edge, indexing="ij"), -1).reshape(-1, 3)
        r = rng.integers(0, 1 << 32, (n, 3), dtype=np.uint64)
        r[: n // 4, 1] = np.arange(n // 4) % 4096          # small pixels / dims, as the renderer's
        r[: n // 4, 2] = np.arange(n // 4) // 4096
        res = items_u(g[:, 0], g[:, 1], g[:, 2]), items_u(r[:, 0], r[:, 1], r[:, 2])
    else:   # algebra over six floats
        unit = rng.normal(size=(n // 2, 6)).astype(F)
        unit[:, :3] /= np.linalg.norm(unit[:, :3], axis=1, keepdims=True).astype(F)
        unit[:, 3:] /= np.linalg.norm(unit[:, 3:], axis=1, keepdims=True).astype(F)
        unit[::3, 5] = F(1.5)                                # refract's eta = f5 beyond 1: both of its branches
        unit[::7, 3] = (rng.random(len(unit[::7]), dtype=F) * F(16404.0) - F(8202.0))   # rotate_rowvec's angle = f3
        e = np.stack(exponent_pairs(rng, 3 * (n // 2)), -1).reshape(-1, 6)
        v = np.concatenate([SPECIALS, np.array([1.0, -1.0], F)])
        g = np.stack([v[rng.integers(0, len(v), 4096)] for _ in range(6)], -1)
        res = items_v(g), items_v(np.concatenate([unit, e]))
    _CACHE[op] = res
    return res


def comparable(op, w):
    """The items of `op` on which two compilers are compared: all, but for k_sinf / k_cosf (and rotate_rowvec's
    angle) finite arguments beyond 8192 + 2 pi, where (int)(FOPI x) may leave int's range."""
    if op in ("sinf", "cosf"):
        x = _lo(w, 0)
    elif op == "rotate_rowvec":
        x = _hi(w, 1)
    else:
        return np.ones(len(w), bool)
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(x) & (np.abs(x) > SINCOS_DOMAIN))
