"""csrc/kmath.h as hipcc compiles it for gfx950 against the host compile, op by op.

khp_debug_kmath runs kmath_ops.h's table one item per thread; khp_kmath_host is the plain
loop over the same table (tests/test_kmath_truth.py holds it to a truth).  For every op:
device == host on the lattice and on a 2^18-item subsample of the walk, one launch per op;
a NaN matches a NaN, everything else matches bit for bit.  The IEEE primitives are also
held to numpy directly on the device: a flushed subnormal, an approximate division or
square root or a contracted multiply-add shows here by name.  Finite k_sinf / k_cosf
arguments beyond 8192 + 2 pi are left out; nothing else is.
"""
import ctypes

import numpy as np
import pytest

import _kmathref as R
from ba_pathtracing_fur_amd import kmath_host
from ba_pathtracing_fur_amd import native as N

pytestmark = pytest.mark.gpu
U64 = R.U64
SUB = 1 << 18


def items(op):
    """The lattice and a seeded 2^18-item subsample of the walk: at most 2^20 items, one launch."""
    lat, wk = R.inputs(op)
    rng = np.random.default_rng(5000 + R.OPS.index(op))
    pick = np.sort(rng.choice(len(wk), SUB, replace=False)) if len(wk) > SUB else np.arange(len(wk))
    w = np.concatenate([lat, wk[pick]])
    assert len(w) <= (1 << 20)
    return w


def mismatches(op, got, want, w):
    ok = R.same_bits(got, want, R.KIND[op]).all(axis=1) | ~R.comparable(op, w)
    bad = np.flatnonzero(~ok)
    first = ([hex(int(x)) for x in w[bad[0]]], [hex(int(x)) for x in got[bad[0]]],
             [hex(int(x)) for x in want[bad[0]]]) if bad.size else None
    return bad.size, first


@pytest.mark.parametrize("op", R.OPS)
def test_device_equals_host(hip_ctx, op):
    w = items(op)
    n, first = mismatches(op, hip_ctx.debug_kmath(op, w), kmath_host(op, w), w)
    assert n == 0, (op, n, len(w), first)


@pytest.mark.parametrize("op", ["mul", "add", "div", "sqrt", "rsqrt", "muladd", "floor", "dmul", "dadd", "ddiv", "umulhi",
                                "i2f", "u2f", "u642f", "f2i", "f2u", "d2i2d"])
def test_device_primitives_equal_numpy(hip_ctx, op):
    """numpy is correctly rounded and unfused and keeps subnormals; the integer ops are exact.  The same
    arrays as on the host (test_kmath_truth.py shows that a quarter of muladd's triples tell fused from unfused)."""
    w = items(op)
    n, first = mismatches(op, hip_ctx.debug_kmath(op, w), R.apply(op, w), w)
    assert n == 0, (op, n, len(w), first)


def test_debug_kmath_refuses_bad_arguments(hip_ctx):
    """Every argument is checked on the host; a refused call launches nothing and leaves the framebuffer
    and khp_stats as they were.  The query needs no scene."""
    from ba_pathtracing_fur_amd import scenes as S
    from ba_pathtracing_fur_amd.pathtracer import HipContext
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    P = ctypes.POINTER(ctypes.c_uint64)
    w, o = np.zeros((4, 3), U64), np.full((4, 3), 7, U64)
    a, b, null = w.ctypes.data_as(P), o.ctypes.data_as(P), ctypes.cast(None, P)
    fresh = HipContext(0)                      # no scene: the query needs none
    try:
        assert lib.khp_debug_kmath(fresh.ptr, 0, 4, a, b) == N.KHP_OK, err()
        assert not o.any()
    finally:
        fresh.close()
    W, H = 16, 12
    hip_ctx.set_scene(S.config2(W, H, n_strands=20))
    hip_ctx.build_accel()
    hip_ctx.render(W, H, 1, 3)
    fb, st = hip_ctx.read_framebuffer(W, H).copy(), hip_ctx.stats()
    c = hip_ctx.ptr
    o[:] = 7
    for op in (len(R.OPS), 1000, 0xFFFFFFFF):
        assert lib.khp_debug_kmath(c, op, 4, a, b) == N.KHP_EINVAL and "unknown op" in err(), op
    for n in (0, (1 << 20) + 1, 0xFFFFFFFF):
        assert lib.khp_debug_kmath(c, 0, n, a, b) == N.KHP_EINVAL and "n must be" in err(), n
    assert lib.khp_debug_kmath(c, 0, 4, null, b) == N.KHP_EINVAL and "null" in err()
    assert lib.khp_debug_kmath(c, 0, 4, a, null) == N.KHP_EINVAL and "null" in err()
    assert lib.khp_debug_kmath(None, 0, 4, a, b) == N.KHP_EINVAL and "null" in err()
    assert (o == 7).all()
    assert lib.khp_debug_kmath(c, 0, 4, a, b) == N.KHP_OK, err()          # and a good call changes neither
    assert np.array_equal(hip_ctx.read_framebuffer(W, H).view(np.uint32), fb.view(np.uint32))
    assert hip_ctx.stats() == st
