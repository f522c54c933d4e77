"""csrc/kmath.h as the host compiler builds it into the library, op by op, against a truth.

tests/test_kmath.py holds the oracle's C restatement (ko_*) to float64 references on a few
thousand points.  This file calls the product's own compile of kmath.h through
khp_kmath_host (csrc/kmath_ops.h) on about a million items per op -- a prime-strided walk
of the float32 bit patterns of each documented domain, a lattice of every branch
threshold, octant boundary and special value, seeded pairs over all exponents -- and asserts

* three-way equality, tolerance 0: khp_kmath_host == the numpy restatement of
  tests/_kmathref.py == the oracle's ko_* (where the oracle exports the function); a NaN
  matches a NaN, everything else matches bit for bit, the sign of zero included;
* that the private restatements in _lensref, _denoiseref, _furref and _aovref equal it too;
* accuracy against float64 libm / mpmath within the bounds DESIGN.md §2 states;
* the IEEE primitives against numpy (correctly rounded, unfused) and Python integers;
* the contract's edges as they are.

The device half is tests/test_gpu_kmath.py.  Measured worsts are printed before each
assertion (pytest -s shows them); DESIGN.md §2 records them.
"""
import ctypes
import math

import numpy as np
import pytest

import _kmathref as R
import oracle_ffi
from ba_pathtracing_fur_amd import kmath_host
from ba_pathtracing_fur_amd import native as N

F, D, U32, U64 = R.F, R.D, R.U32, R.U64
CHUNK = 1 << 20


def host(op, w):
    """khp_kmath_host over any number of items (the entry takes 2^20 at a time)."""
    w = np.ascontiguousarray(w, U64)
    return np.concatenate([kmath_host(op, w[s:s + CHUNK]) for s in range(0, len(w), CHUNK)])


def all_items(op):
    lat, wk = R.inputs(op)
    return np.concatenate([lat, wk])


def assert_same(op, got, want, w, what):
    ok = R.same_bits(got, want, R.KIND[op]).all(axis=1) | ~R.comparable(op, w)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (what, op, len(bad), [hex(int(x)) for x in w[bad[0]]], [hex(int(x)) for x in got[bad[0]]],
                           [hex(int(x)) for x in want[bad[0]]])


def test_op_names_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kirk_hip.h")).read()
    enum = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"KHP_KMATH_([A-Z0-9_]+) = (\d+)", hdr))
    assert enum.pop("op_count") == len(R.OPS) == len(N.KMATH_OPS)
    assert enum == {name: i for i, name in enumerate(R.OPS)} == N.KMATH_OP


def test_walks_have_a_prime_stride_and_the_issue_s_size():
    for op in R.UNARY_HI:
        lat, wk = R.inputs(op)
        s = R.WALK_STRIDE[op]
        assert s >= 2 and all(s % k for k in range(2, math.isqrt(s) + 1)), (op, s)
        if op != "f2u":   # one sign only
            assert (1 << 19) <= len(wk) <= (1 << 21), (op, len(wk))


# ---- three-way equality ----------------------------------------------------------------------
@pytest.mark.parametrize("op", R.OPS)
def test_host_equals_restatement(op):
    w = all_items(op)
    assert_same(op, host(op, w), R.apply(op, w), w, "host vs numpy restatement")


ORACLE_FN = {"sinf": 0, "cosf": 1, "atan2f": 2, "acosf": 3, "asinf": 4, "expf": 5, "sinhf": 6, "j0": 7, "log_d": 8,
             "exp_d": 9, "pow_d": 10}


def oracle(fn, w):
    L = oracle_ffi.load()
    w = np.ascontiguousarray(w, U64)
    o = np.zeros(len(w), U64)
    P = ctypes.POINTER(ctypes.c_uint64)
    assert L.ko_math_n(fn, len(w), w.ctypes.data_as(P), o.ctypes.data_as(P)) == 0
    return o


@pytest.mark.parametrize("op", sorted(ORACLE_FN))
def test_host_equals_oracle(op):
    """The oracle's C restatement, on every item.  Its (int) of an out-of-range product is the host
    compiler's too, but not defined: the same items are left out as between the two compilers."""
    w = all_items(op)
    got = host(op, w)
    want = np.zeros_like(got)
    want[:, 0] = oracle(ORACLE_FN[op], w)
    assert_same(op, got, want, w, "host vs oracle")


def test_host_rng_equals_oracle():
    """ko_rand_u32(seed, pixel, sample, dim) == draw_u32(path_key(seed, pixel, sample), dim)."""
    lat, wk = R.inputs("path_key")
    w = np.concatenate([lat, wk])
    key = host("path_key", w)[:, 0]
    dim = (w[:, 2] * U64(2654435761) + w[:, 1]) & R.M32 & U64(0x1FF)   # bounce * 16 + purpose stays small
    got = host("draw_u32", R.items_u(key, dim))[:, 0]
    packed = w.copy()
    packed[:, 2] = (w[:, 2] & R.M32) | (dim << U64(32))
    assert np.array_equal(got, oracle(11, packed))


def test_private_restatements_agree():
    """The four test references that carry a piece of kmath of their own, held to _kmathref on the lattice."""
    import _aovref
    import _denoiseref
    import _furref
    import _lensref
    lat = np.concatenate([R.lattice(), R.octant_lattice(), R.walk(float(R.SINCOS_DOMAIN), target=1 << 16)[0]])
    with np.errstate(all="ignore"):
        x = lat[np.isfinite(lat) & (np.abs(lat) <= R.SINCOS_DOMAIN)]   # _lensref's are written for finite arguments
        assert np.array_equal(R.fbits(_lensref.k_sinf(x)), R.fbits(R.k_sinf(x)))
        assert np.array_equal(R.fbits(_lensref.k_cosf(x)), R.fbits(R.k_cosf(x)))
        e = np.concatenate([R.lattice(), R.walk(104.0, target=1 << 16)[0]])
        assert R.same_bits(R.fbits(_denoiseref.k_expf(e)).astype(U64), R.fbits(R.k_expf(e)).astype(U64), "f").all()
        lx, lk = R.inputs("ldexpf")
        lw = np.concatenate([lx, lk[:1 << 16]])
        xs, ks = R._lo(lw, 0), (lw[:, 1] & R.M32).astype(U32).view(np.int32)
        assert R.same_bits(R.fbits(_denoiseref.k_ldexpf(xs, ks)).astype(U64), R.fbits(R.k_ldexpf(xs, ks)).astype(U64),
                           "f").all()
    ilat, iwk = R.inputs("draw_u01")
    iw = np.concatenate([ilat, iwk[:1 << 16]])
    keys = (iw[:, 0] & R.M32).astype(U32)
    assert np.array_equal(_furref.lowbias32(keys.astype(U64)), R.lowbias32(keys).astype(U64))
    for dim in (0, 1, 9, 16 * 7 + 11, 0xFFFFFFFF):
        got = _furref.draw_u01(keys.astype(U64), dim)
        assert got.dtype == F and np.array_equal(R.fbits(got), R.fbits(R.draw_u01(keys, np.full(len(keys), dim, U32))))
    pix, smp = (iw[:, 1] & R.M32), (iw[:, 2] & R.M32)
    for seed in (0, 0x4B49524B, 0xFFFFFFFF, 12345):
        assert np.array_equal(_aovref.path_key(seed, pix, smp), R.path_key(np.full(len(pix), seed, U32), pix.astype(U32),
                                                                           smp.astype(U32)).astype(U64))
    vl, vw = R.inputs("normalize")
    six = np.concatenate([vl, vw[:1 << 16]])
    a = np.stack([R._lo(six, 0), R._hi(six, 0), R._lo(six, 1)], 1)
    with np.errstate(all="ignore"):
        want = np.stack(R.normalize((a[:, 0], a[:, 1], a[:, 2])), 1)
        got = _aovref.normalize32(a)
    assert R.same_bits(R.fbits(got).astype(U64), R.fbits(want).astype(U64), "f").all()


# ---- accuracy against the truth ---------------------------------------------------------------
def _unary(op):
    w = all_items(op)
    return R._lo(w, 0), R.out_f(host(op, w))


SINCOS = [("sinf", np.sin), ("cosf", np.cos)]


def _sincos(op, ref):
    x, y = _unary(op)
    dom = np.isfinite(x) & (np.abs(x) <= R.SINCOS_DOMAIN)
    x, y = x[dom], y[dom]
    return x, y, ref(x.astype(D))


@pytest.mark.parametrize("op,ref", SINCOS)
def test_sin_cos_absolute(op, ref):
    """abs 2.5e-7 on the whole domain |x| <= 8192 + 2 pi.  Beyond 12 only this bound is stated: next to the
    zeros the relative error grows with |x| (printed)."""
    x, y, t = _sincos(op, ref)
    a = np.abs(y.astype(D) - t).max()
    outer = np.abs(x) > F(12.0)
    print(f"{op}: {len(x)} items on |x| <= 8192 + 2 pi, worst abs {a:.3e}; worst ulp beyond 12: "
          f"{R.ulp32(y[outer], t[outer]).max():.1f}")
    assert a < 2.5e-7


@pytest.mark.parametrize("op,ref", SINCOS)
def test_sin_cos_ulp(op, ref):
    """2 ulp on [-12, 12], the documented bound, over the walk and the octant lattice.

    The lattice found what no sparse sweep does: with the three-constant reduction alone the bound was missed
    at one argument of each function and its negative, an octant boundary next to a zero --
        k_sinf(+-9.42477798f) (the float nearest 3 pi):     2.38497364e-08 for 2.38497609e-08, 13.79 ulp
        k_cosf(+-4.71238899f) (the float nearest 3 pi / 2): 1.19248682e-08 for 1.19248805e-08, 13.79 ulp
    (a draw of exactly 0.75 reaches the second).  kmath.h's k_reduce now takes a reduced argument below
    2^-20 again with DP3 in two parts; the worst is 1.37 ulp, and every other argument keeps its bits."""
    x, y, t = _sincos(op, ref)
    inner = np.abs(x) <= F(12.0)
    u = R.ulp32(y[inner], t[inner])
    i = int(np.argmax(u))
    print(f"{op}: {inner.sum()} items on [-12, 12], worst {u.max():.3f} ulp at x = {x[inner][i]!r}: got {y[inner][i]!r}, "
          f"truth {t[inner][i]!r}")
    assert u.max() <= 2.0


def test_reduction_second_take_changes_tiny_residuals_only():
    """k_reduce against the three-constant sequence it replaced (the restatement with second_take=False): the
    results differ only where that sequence's reduced argument is below 2^-20, which on |x| <= 2 pi is three
    floats at 3 pi / 2 for k_cosf and none for k_sinf."""
    for op, fn in (("sinf", R.k_sinf), ("cosf", R.k_cosf)):
        x, y = _unary(op)
        dom = np.isfinite(x) & (np.abs(x) <= R.SINCOS_DOMAIN)
        x, y = x[dom], y[dom]
        with np.errstate(all="ignore"):
            old = fn(x, second_take=False)
            r3 = R._octant(np.abs(x))[2]
        changed = R.fbits(old) != R.fbits(y)
        assert changed.any() and not (changed & (np.abs(r3) >= F(2.0 ** -20))).any(), op
        near = np.unique(np.abs(x)[changed & (np.abs(x) <= F(6.2832))]).tolist()
        assert near == ([] if op == "sinf" else [4.712388038635254, 4.71238899230957, 4.7123894691467285]), (op, near)


@pytest.mark.parametrize("op,ref,tol", [("asinf", np.arcsin, 3.0), ("acosf", np.arccos, 3.0)])
def test_asin_acos_accuracy(op, ref, tol):
    x, y = _unary(op)
    dom = np.abs(x) <= F(1.0)
    u = R.ulp32(y[dom], ref(x[dom].astype(D))).max()
    print(f"{op}: {dom.sum()} items on [-1, 1], worst {u:.3f} ulp")
    assert u <= tol
    with np.errstate(invalid="ignore"):
        assert np.isnan(y[np.abs(x) > F(1.0)]).all()


def test_exp_accuracy():
    """2 ulp between the two cuts, subnormal results included (their ulp is 2^-149)."""
    x, y = _unary("expf")
    dom = (x >= R.EXP_LO) & (x < R.EXP_HI)   # from the float of the upper cut on, e^x is beyond FLT_MAX
    with np.errstate(all="ignore"):
        t = np.exp(x[dom].astype(D))
    u = R.ulp32(y[dom], t)
    sub = t < 1.1754943508222875e-38
    print(f"expf: {dom.sum()} items on [{R.EXP_LO}, {R.EXP_HI}], worst {u.max():.3f} ulp; {sub.sum()} subnormal results, "
          f"worst {u[sub].max():.3f} ulp")
    assert sub.sum() > 500 and u.max() <= 2.0


def test_sinh_accuracy():
    x, y = _unary("sinhf")
    dom = (np.abs(x) > 0) & (np.abs(x) <= F(88.72))
    u = R.ulp32(y[dom], np.sinh(x[dom].astype(D))).max()
    print(f"sinhf: {dom.sum()} items on 0 < |x| <= 88.72, worst {u:.3f} ulp")
    assert u <= 3.0


def test_atan_atan2_accuracy():
    """No relative bound is stated for either: the measured worst is printed, the absolute bound asserted."""
    x, y = _unary("atanf")
    ok = ~np.isnan(x)
    t = np.arctan(x[ok].astype(D))
    print(f"atanf: {ok.sum()} items, worst {R.ulp32(y[ok], t).max():.3f} ulp, abs {np.abs(y[ok].astype(D) - t).max():.3e}")
    assert np.abs(y[ok].astype(D) - t).max() < 5e-7
    w = all_items("atan2f")
    yy, xx, got = R._lo(w, 0), R._lo(w, 1), R.out_f(host("atan2f", w))
    with np.errstate(all="ignore"):
        # left out: NaN, and the edges of the contract that are not atan2's values (test_contract_edges):
        # both arguments infinite, both zero, and -0 over a negative x
        ok = (~(np.isnan(yy) | np.isnan(xx)) & ~(np.isinf(yy) & np.isinf(xx)) & ~((yy == 0) & (xx == 0)) &
              ~((yy == 0) & np.signbit(yy) & (xx < 0)))
    t = np.arctan2(yy[ok].astype(D), xx[ok].astype(D))
    a = np.abs(got[ok].astype(D) - t)
    print(f"atan2f: {ok.sum()} pairs, worst {R.ulp32(got[ok], t).max():.3f} ulp, abs {a.max():.3e}")
    assert a.max() < 5e-7


def test_logf_powf_accuracy():
    x, y = _unary("logf_d")
    ok = x > 0
    with np.errstate(all="ignore"):
        u = R.ulp32(y[ok & np.isfinite(x)], np.log(x[ok & np.isfinite(x)].astype(D))).max()
    print(f"logf_d: {ok.sum()} positive floats, worst {u:.3f} ulp")
    assert u <= 1.0
    w = all_items("powf_d")
    a, b, got = R._lo(w, 0), R._lo(w, 1), R.out_f(host("powf_d", w))
    with np.errstate(all="ignore"):
        t = np.power(a.astype(D), b.astype(D))
        ok = (a > 0) & np.isfinite(a) & np.isfinite(b) & (np.abs(b.astype(D) * np.log(a.astype(D))) < 40.0)
    u = R.ulp32(got[ok], t[ok]).max()
    print(f"powf_d: {ok.sum()} pairs with |y log x| < 40, worst {u:.3f} ulp")
    assert u <= 1.0


def test_hypot_accuracy():
    """sqrtf(x x + y y) where neither square leaves the normal range: three roundings, under 2 ulp."""
    w = all_items("hypotf")
    a, b, got = R._lo(w, 0), R._lo(w, 1), R.out_f(host("hypotf", w))
    with np.errstate(all="ignore"):
        m, s = np.maximum(np.abs(a), np.abs(b)), np.minimum(np.abs(a), np.abs(b))
        ok = np.isfinite(a) & np.isfinite(b) & (m < F(1e19)) & ((s > F(1e-18)) | (s == 0)) & (m > F(1e-18))
        u = R.ulp32(got[ok], np.hypot(a[ok].astype(D), b[ok].astype(D))).max()
    print(f"hypotf: {ok.sum()} pairs, worst {u:.3f} ulp")
    assert u <= 2.0


def test_j0_against_mpmath():
    """1e-12 on [-6, 6] against mpmath's Bessel function at 80 digits."""
    lat, wk = R.inputs("j0")
    x = R.from_dbits(np.concatenate([lat, wk])[:, 0])
    x = x[np.abs(x) <= 6.0]
    x = np.concatenate([x[:: max(1, len(x) // 1500)], [6.0, -6.0, 0.0, 2.404825557695773, 5.520078110286311]])
    got = R.out_d(host("j0", R.items_d(x)))
    want = np.array([float(t) for t in R.mp_truth("j0", x)])
    e = np.abs(got - want).max()
    print(f"j0: {len(x)} items on [-6, 6], worst abs {e:.3e}")
    assert e < 1e-12


def test_double_log_exp_pow_against_mpmath():
    """2 ulp for k_log_d and k_exp_d (normal results), 64 ulp for k_pow_d with |y log x| < 40."""
    rng = np.random.default_rng(7)
    lat, wk = R.inputs("log_d")
    x = R.from_dbits(np.concatenate([lat, wk[rng.integers(0, len(wk), 2500)]])[:, 0])
    x = x[(x > 0) & np.isfinite(x)]
    u = R.ulp64_mp(R.out_d(host("log_d", R.items_d(x))), R.mp_truth("log", x)).max()
    print(f"log_d: {len(x)} items, worst {u:.3f} ulp")
    assert u <= 2.0
    lat, wk = R.inputs("exp_d")
    x = R.from_dbits(np.concatenate([lat, wk[rng.integers(0, len(wk), 2500)]])[:, 0])
    x = x[(x > -708.39) & (x <= 709.782712893384)]   # results at or above DBL_MIN
    u = R.ulp64_mp(R.out_d(host("exp_d", R.items_d(x))), R.mp_truth("exp", x)).max()
    print(f"exp_d: {len(x)} items, worst {u:.3f} ulp")
    assert u <= 2.0
    lat, wk = R.inputs("pow_d")
    pw = wk[rng.integers(0, len(wk), 2500)]
    x, y = R.from_dbits(pw[:, 0]), R.from_dbits(pw[:, 1])
    ok = (x > 0) & (np.abs(y * np.log(np.where(x > 0, x, 1.0))) < 40.0)
    x, y = x[ok], y[ok]
    u = R.ulp64_mp(R.out_d(host("pow_d", R.items_d(x, y))), R.mp_truth("pow", x, y)).max()
    print(f"pow_d: {len(x)} pairs with |y log x| < 40, worst {u:.3f} ulp")
    assert u <= 64.0


def test_pow_special_cases_c99():
    """tests/test_kmath.py's list, on the product's own compile."""
    c = np.array(R.POW_C99, D)
    want = [1.0, 1.0, np.inf, -np.inf, -0.0, 0.0, 1.0, np.inf, 0.0, 0.0, -0.0, -np.inf, np.inf, 0.0, -8.0, 4.0, np.nan,
            1024.0]
    got = R.out_f(host("powf_d", R.items_f(c[:, 0], c[:, 1])))
    gd = R.out_d(host("pow_d", R.items_d(c[:, 0], c[:, 1])))
    for (x, y), g, g64, t in zip(R.POW_C99, got, gd, want):
        if np.isnan(t):
            assert np.isnan(g) and np.isnan(g64), (x, y)
        else:
            assert g == t and np.signbit(g) == np.signbit(t), (x, y, g)
            assert np.float32(g64) == t and np.signbit(g64) == np.signbit(t), (x, y, g64)


# ---- IEEE primitives against numpy and Python integers ----------------------------------------------
def test_fused_and_unfused_multiply_add_differ_on_the_items():
    """On the truth alone: at least a quarter of the seeded triples have a fused result (one rounding of
    a b + c, here through exact float64 products) that is not the unfused one, so a contracted
    multiply-add cannot pass test_host_equals_restatement['muladd'] or its device twin."""
    lat, wk = R.inputs("muladd")
    a, b, c = (R._lo(wk, k) for k in range(3))
    with np.errstate(all="ignore"):
        fused = (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)     # the product of two float32 is exact in float64
        unfused = (a * b) + c
    differ = ~R.same_bits(R.fbits(fused).astype(U64), R.fbits(unfused).astype(U64), "f")
    print(f"muladd: {differ.sum()} of {len(wk)} triples differ between fused and unfused")
    assert differ.mean() >= 0.25


@pytest.mark.parametrize("op", ["mul", "add", "div", "sqrt", "muladd"])
def test_primitives_cover_subnormals(op):
    """The seeded items have subnormal operands and subnormal results (equality is test_host_equals_restatement's)."""
    lat, wk = R.inputs(op)
    tiny = lambda v: (np.abs(v) < F(1.1754943508222875e-38)) & (v != 0)
    out = R.out_f(host(op, wk))
    assert tiny(R._lo(wk, 0)).sum() > 100, op
    if op != "sqrt":   # the root of a subnormal is normal
        assert tiny(out).sum() > 100, op


def test_conversions_against_python_integers():
    """(int)a, (uint32_t)a, the three integer -> float conversions, (double)(int64_t)d and the high product,
    against Python's integers and fractions on in-range arguments."""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    pick = lambda op, k=3000: (lambda lat, wk: np.concatenate([lat, wk[rng.integers(0, len(wk), k)]]))(*R.inputs(op))
    w = pick("f2i")
    want = [int(float(x)) & 0xFFFFFFFF for x in R._lo(w, 0)]
    assert [int(v) for v in host("f2i", w)[:, 0]] == want
    w = pick("f2u")
    assert [int(v) for v in host("f2u", w)[:, 0]] == [int(float(x)) for x in R._lo(w, 0)]

    def nearest_f32(i):   # round-to-nearest-even of the integer i, in integers
        if i == 0:
            return 0.0
        s, m = (-1 if i < 0 else 1), abs(i)
        sh = max(m.bit_length() - 24, 0)
        q, r = m >> sh, m & ((1 << sh) - 1)
        if sh and (r > (1 << (sh - 1)) or (r == (1 << (sh - 1)) and (q & 1))):
            q += 1
        return float(s * Fraction(q << sh))

    for op, conv in (("i2f", lambda v: v - (1 << 32) if v >= (1 << 31) else v), ("u2f", lambda v: v), ("u642f", lambda v: v)):
        w = pick(op)
        got = R.out_f(host(op, w))
        assert [float(g) for g in got] == [nearest_f32(conv(int(v))) for v in w[:, 0]], op
    w = pick("d2i2d")
    got = R.out_d(host("d2i2d", w))
    assert [float(g) for g in got] == [float(int(x)) for x in R.from_dbits(w[:, 0])]
    assert np.array_equal(np.signbit(got), np.zeros(len(got), bool) | (R.from_dbits(w[:, 0]) <= -1.0))   # (double)0 is +0
    w = pick("umulhi")
    assert [int(v) for v in host("umulhi", w)[:, 0]] == [(int(a) * int(b)) >> 64 for a, b in w[:, :2]]


# ---- the contract's edges, as they are ----------------------------------------------------------------
def _f1(op, *args):
    return R.out_f(host(op, R.items_f(*[np.array([a], F) for a in args])))[0]


def test_contract_edges():
    inf, nan = F(np.inf), F(np.nan)
    bits = lambda v: int(R.fbits(F(v))[0])
    assert bits(_f1("sinf", F(-0.0))) == 0x00000000                       # k_sinf(-0) is +0
    for y in (F(0.0), F(-0.0)):
        for x in (F(-1.0), F(-1e-30), F(-3e38)):
            assert bits(_f1("atan2f", y, x)) == bits(R.PIF)                # k_atan2f(+-0, -x) is +pi
    assert np.isnan(_f1("atan2f", inf, inf)) and np.isnan(_f1("atan2f", -inf, inf))
    assert bits(_f1("atan2f", F(0.0), F(0.0))) == 0 and bits(_f1("atan2f", F(-0.0), F(-0.0))) == 0
    assert bits(_f1("asinf", F(1.0))) == bits(R.PIO2F) and bits(_f1("asinf", F(-1.0))) == bits(-R.PIO2F)
    assert bits(_f1("acosf", F(1.0))) == 0
    below, down = np.nextafter(R.EXP_HI, -inf), np.nextafter(R.EXP_LO, -inf)
    # inf from the float of the upper cut on (e^x is beyond FLT_MAX there), finite below it
    assert _f1("expf", R.EXP_HI) == inf and _f1("expf", np.nextafter(R.EXP_HI, inf)) == inf
    assert _f1("expf", below) == F(3.4027985e+38)
    # 2^-149 down to the float of the lower cut, +0 below it
    assert bits(_f1("expf", R.EXP_LO)) == 1 and bits(_f1("expf", down)) == 0 and bits(_f1("expf", -inf)) == 0
    # k_sinhf is inf from k_expf's cut, although sinh is finite to 89.4
    assert _f1("sinhf", R.EXP_HI) == inf and _f1("sinhf", -R.EXP_HI) == -inf and np.isfinite(_f1("sinhf", below))
    for op in ("sinf", "cosf"):
        for v in (nan, -nan, inf, -inf):
            assert np.isnan(_f1(op, v)), (op, v)
    x0 = R.first_subnormal_exp_arg()
    assert 0 < _f1("expf", x0) < F(1.1754943508222875e-38) <= _f1("expf", np.nextafter(x0, inf))


def test_kmath_host_refuses_bad_arguments():
    lib = N.load_library()
    P = ctypes.POINTER(ctypes.c_uint64)
    w = np.zeros((4, 3), U64)
    o = np.zeros((4, 3), U64)
    a, b = w.ctypes.data_as(P), o.ctypes.data_as(P)
    null = ctypes.cast(None, P)
    assert lib.khp_kmath_host(0, 4, a, b) == N.KHP_OK
    for op in (len(R.OPS), 1000, 0xFFFFFFFF):
        assert lib.khp_kmath_host(op, 4, a, b) == N.KHP_EINVAL and b"unknown op" in lib.khp_last_error()
    for n in (0, (1 << 20) + 1, 0xFFFFFFFF):
        assert lib.khp_kmath_host(0, n, a, b) == N.KHP_EINVAL and b"n must be" in lib.khp_last_error()
    assert lib.khp_kmath_host(0, 4, null, b) == N.KHP_EINVAL and b"null" in lib.khp_last_error()
    assert lib.khp_kmath_host(0, 4, a, null) == N.KHP_EINVAL and b"null" in lib.khp_last_error()
    assert not o.any()
    assert lib.khp_debug_kmath(None, 0, 4, a, b) == N.KHP_EINVAL and b"null" in lib.khp_last_error()


# ---- the domain, closed where a scene could leave it ----------------------------------------------------
def _host_build_status(sd):
    lib = N.load_library()
    d = sd.desc()
    nn, dep = ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib.khp_host_build(ctypes.byref(d), ctypes.byref(nn), ctypes.byref(dep), None, None, None, None, None, None)
    return rc, lib.khp_last_error().decode()


def test_scene_angles_beyond_the_sine_domain_are_refused():
    """The two finite scene values that reach k_sinf / k_cosf unbounded (DESIGN.md §2's domain table): the
    roughness of a GlossyBSDF / MilkGlassBSDF material (sample_angle's cone is roughness * pi) and a spot
    light's outer_angle (degrees; the light-path variant samples its cone).  Refused where the scene is
    set, beyond 8192 radians either way, as khp_set_env_light refuses its rotation; NaN stays KIRK's."""
    from ba_pathtracing_fur_amd import scenes as S
    ok_r, bad_r = 2607.0, 2608.0            # roughness * pi: 8190.1 and 8193.3 radians
    ok_a, bad_a = 469360.0, 469380.0        # degrees: 8191.9 and 8192.2 radians
    for kind in ("GlossyBSDF", "MilkGlassBSDF"):
        for r, want in ((ok_r, N.KHP_OK), (-ok_r, N.KHP_OK), (bad_r, N.KHP_EINVAL), (-bad_r, N.KHP_EINVAL),
                        (3.0e38, N.KHP_EINVAL), (float("inf"), N.KHP_EINVAL), (float("nan"), N.KHP_OK)):
            sd = S.config1(8, 8)
            sd.materials[0] = S.material(kind, roughness=r)
            rc, msg = _host_build_status(sd)
            assert rc == want, (kind, r, msg)
            if want != N.KHP_OK:
                assert "material 0" in msg and "8192" in msg, msg
    sd = S.config1(8, 8)
    sd.materials[0] = S.material("LambertianReflectionBSDF", roughness=bad_r)   # the kind never reads it
    assert _host_build_status(sd)[0] == N.KHP_OK
    base = S.config1(8, 8)
    for a, want in ((ok_a, N.KHP_OK), (-ok_a, N.KHP_OK), (bad_a, N.KHP_EINVAL), (-bad_a, N.KHP_EINVAL),
                    (float("inf"), N.KHP_EINVAL)):
        sd = S.config1(8, 8)
        L = N.Light.from_buffer_copy(bytes(base.lights[0])) if base.lights else N.Light()
        L.kind, L.outer_angle, L.inner_angle = N.LIGHT_SPOT, a, 0.0
        L.direction[:] = [0.0, -1.0, 0.0]
        sd.lights = [L]
        rc, msg = _host_build_status(sd)
        assert rc == want, (a, msg)
        if want != N.KHP_OK:
            assert "light 0" in msg and "8192" in msg, msg
    L.kind = N.LIGHT_POINT                                                         # the kind never reads it
    assert _host_build_status(sd)[0] == N.KHP_OK
