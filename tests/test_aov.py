"""khp_render_aov without a device: the export, the struct, the refusals of bad arguments
(checked before the context is touched), and the restatement's ordered reduction
(tests/_aovref.py) on hand-made records."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ba_pathtracing_fur_amd as P
from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd.pathtracer import HipContext

import _aovref as A

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(width=8, height=8, spp=1, flags=0):
    return N.RenderParams(width, height, spp, 5, 1, 0, 0, 0, 1, flags)


def _buffers(n=64, **which):
    keep = {ch: np.zeros((n,) + tail, dt) for ch, (tail, dt) in N.AOV_CHANNELS.items() if which.get(ch, True)}
    buf = N.AovBuffers()
    for ch, a in keep.items():
        setattr(buf, ch, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32 if ch == "object" else ctypes.c_float)))
    return buf, keep


def test_symbol_is_exported_and_listed():
    lib = N.load_library()
    assert "khp_render_aov" in N.EXPORTED and hasattr(lib, "khp_render_aov")
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert re.search(r"\bT khp_render_aov\b", out)
    header = open(os.path.join(ROOT, "include", "kirk_hip.h")).read()
    assert "khp_status khp_render_aov(khp_ctx* ctx, const khp_render_params* p, const khp_aov_buffers* out);" in header
    assert "#define KHP_AOV_TANGENT_IS_FRAME_V 1" in header
    # khp_render_aov was added under ABI 16 (symbols added, nothing moved); 17 adds the light-path queries
    assert "#define KHP_ABI_VERSION 17" in header and N.ABI_VERSION == 17
    assert "render_aov" in open(os.path.join(ROOT, "include", "kirk_hip.hpp")).read()
    assert callable(HipContext.render_aov)
    assert HipContext.AOV_CHANNELS == ("normal", "albedo", "tangent", "depth", "coverage", "object")
    for name in ("AovBuffers", "AOV_CHANNELS"):
        assert name in P.__all__ and getattr(P, name) is getattr(N, name)


def test_struct_layout():
    assert ctypes.sizeof(N.AovBuffers) == 48
    assert [f[0] for f in N.AovBuffers._fields_] == list(N.AOV_CHANNELS) == list(A.CHANNELS)
    assert [getattr(N.AovBuffers, ch).offset for ch in A.CHANNELS] == [0, 8, 16, 24, 32, 40]


def test_null_arguments_need_no_device():
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    p, (buf, _keep) = _params(), _buffers()
    assert lib.khp_render_aov(None, ctypes.byref(p), ctypes.byref(buf)) == N.KHP_EINVAL and "null" in err()
    assert "ctx" in err()
    assert lib.khp_render_aov(None, None, ctypes.byref(buf)) == N.KHP_EINVAL and "null" in err()
    assert lib.khp_render_aov(None, ctypes.byref(p), None) == N.KHP_EINVAL and "null" in err()
    empty = N.AovBuffers()
    assert lib.khp_render_aov(None, ctypes.byref(p), ctypes.byref(empty)) == N.KHP_EINVAL and "null" in err()
    assert "buffer" in err()


def test_bad_parameters_are_refused_before_the_context():
    """The arguments are judged first, so each refusal names its own cause even without a context."""
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    buf, _keep = _buffers()
    call = lambda p: lib.khp_render_aov(None, ctypes.byref(p), ctypes.byref(buf))
    for flags in (N.RENDER_NO_READBACK, N.RENDER_STATS, N.RENDER_ASYNC, N.RENDER_OUT_DEVICE | N.RENDER_ASYNC, 1 << 4,
                  1 << 31):
        assert call(_params(flags=flags)) == N.KHP_EINVAL and "flags" in err(), flags
    assert call(_params(spp=0)) == N.KHP_EINVAL and "spp" in err()
    assert call(_params(spp=(1 << 24) + 1)) == N.KHP_EINVAL and "spp" in err()
    for w, h in ((0, 8), (8, 0), (0, 0)):
        assert call(_params(width=w, height=h)) == N.KHP_EINVAL and "width" in err(), (w, h)
    assert call(_params(width=1 << 16, height=1 << 15)) == N.KHP_EINVAL and "large" in err()
    bad_tile = _params()
    bad_tile.tile_size = 12
    assert call(bad_tile) == N.KHP_EINVAL and "tile_size" in err()
    bad_rank = _params()
    bad_rank.tile_rank, bad_rank.tile_nranks = 3, 3
    assert call(bad_rank) == N.KHP_EINVAL and "tile_rank" in err()
    # both accepted flag values reach the context check
    for flags in (0, N.RENDER_OUT_DEVICE):
        assert call(_params(flags=flags)) == N.KHP_EINVAL and "ctx is null" in err()


def test_wrapper_refuses_unknown_channels_and_wrong_arrays():
    ctx = HipContext.__new__(HipContext)                       # no device: the checks come before the call
    with pytest.raises(ValueError, match="no channel"):
        HipContext.render_aov(ctx, 4, 4, 1, channels=("normal", "colour"))
    with pytest.raises(ValueError, match="float32"):
        HipContext.render_aov(ctx, 4, 4, 1, channels=("depth",), out={"depth": np.zeros((4, 4), np.float64)})
    with pytest.raises(ValueError, match="shape"):
        HipContext.render_aov(ctx, 4, 4, 1, channels=("normal",), out={"normal": np.zeros((4, 4), F32)})
    ctx.ptr = None                                             # keep __del__ from closing what never opened


def test_library_without_the_symbol_asks_for_a_rebuild(tmp_path):
    """A library of this ABI number built before the symbol existed: the 'rebuild' RuntimeError, not AttributeError."""
    src = tmp_path / "old.c"
    src.write_text("int khp_abi_version(void) { return %d; }\n" % N.ABI_VERSION)
    so = tmp_path / "libold.so"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-shared", "-fPIC", "-o", str(so), str(src)])
    with pytest.raises(RuntimeError, match=r"no symbol khp_\w+.*rebuild"):
        N.load_library(str(so))


# ---- the restatement's reduction ---------------------------------------------------------------------------
def _records(per_pixel):
    """per_pixel: list (pixels) of lists (samples) of None (not a surface sample) or
    (normal, albedo, tangent, depth, object)."""
    cols = {ch: [] for ch in A.CHANNELS}
    for samples in per_pixel:
        for s in samples:
            surf = s is not None
            n, a, t, d, ob = s if surf else ((0, 0, 0), (0, 0, 0), (0, 0, 0), 0.0, -1)
            cols["normal"].append(n), cols["albedo"].append(a), cols["tangent"].append(t)
            cols["depth"].append(d), cols["coverage"].append(1.0 if surf else 0.0), cols["object"].append(ob)
    return {ch: np.asarray(v, np.int32 if ch == "object" else F32) for ch, v in cols.items()}


@pytest.mark.parametrize("spp", [1, 3, 5])
def test_reduction_is_the_ordered_float32_sum(spp):
    rng = np.random.default_rng(spp)
    mk = lambda k: (tuple(rng.normal(size=3)), tuple(rng.random(3)), tuple(rng.normal(size=3)),
                    float(rng.random() * 10.0 ** rng.integers(-3, 4)), 100 + k)
    px0 = [mk(k) for k in range(spp)]
    px1 = [mk(10 + k) for k in range(spp)]
    if spp >= 3:
        px1[spp // 2] = None                                    # a non-surface sample in the middle
    px2 = [None] * spp                                          # nothing but light / background
    out = A.reduce_records(_records([px0, px1, px2]), 3, spp)
    # by hand, one add at a time
    for p, samples in enumerate((px0, px1, px2)):
        s_d, s_c, s_n = F32(0.0), F32(0.0), np.zeros(3, F32)
        for s in samples:
            s_d = F32(s_d + (F32(s[3]) if s else F32(0.0)))
            s_c = F32(s_c + (F32(1.0) if s else F32(0.0)))
            s_n = (s_n + (F32(list(s[0])) if s else np.zeros(3, F32))).astype(F32)
        assert out["depth"][p].view(np.uint32) == F32(s_d / F32(spp)).view(np.uint32)
        assert out["coverage"][p].view(np.uint32) == F32(s_c / F32(spp)).view(np.uint32)
        assert np.array_equal(out["normal"][p].view(np.uint32), (s_n / F32(spp)).astype(F32).view(np.uint32))
    assert out["object"].tolist() == [100, 110, -1]
    for ch in A.FLOAT_CHANNELS:                                 # all samples non-surface: +0 everywhere
        assert not out[ch][2].view(np.uint32).any(), ch
    assert out["coverage"][0] == 1.0
    if spp >= 3:
        assert out["coverage"][1] == F32(F32(spp - 1) / F32(spp))


def test_reduction_depends_on_the_order():
    """float32 adds do not commute in general: the restatement must keep the sample order."""
    rec = F32([[1e8, 1.0, -1e8, 1.0]])
    assert A.reduce_samples(rec, 4)[0] == F32(0.25)             # ((1e8 + 1) - 1e8) + 1 = 1 in float32
    assert A.reduce_samples(rec[:, [0, 2, 1, 3]], 4)[0] == F32(0.5)


def test_camera_keys_follow_path_key():
    """path_key by hand for one (seed, pixel, sample): the three lowbias32 steps of kmath.h:330."""
    def lb(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    seed, pixel, sample = 0x1234ABCD, 767, 11
    want = lb((lb(lb(seed ^ 0x4B49524B) ^ pixel) + sample * 0x9E3779B9) & 0xFFFFFFFF)
    assert int(A.path_key(seed, [pixel], [sample])[0]) == want
