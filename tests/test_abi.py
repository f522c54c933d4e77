"""The C-ABI drop-in boundary (include/kirk_hip.h): library loads, exports what the
header declares, registries mirror KIRK's factories, errors are loud.  CPU only (khp_create is
checked to *fail* without a GPU), except the bad-argument cases of the ABI 15
and ABI 17 batch queries and of khp_debug_kmath, which need a context (`gpu`).
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ba_pathtracing_fur_amd import native as N
from ba_pathtracing_fur_amd import scenes as S
from ba_pathtracing_fur_amd.pathtracer import BsdfFactory, ShaderFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kirk_hip.h")


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(khp_[a-z_0-9]+)\s*\(", txt)))


def test_header_and_python_list_agree():
    assert header_functions() == sorted(N.EXPORTED)


def test_library_exports_every_symbol():
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [f for f in header_functions() if f not in syms]
    assert not missing, missing
    lib = N.load_library()
    for f in header_functions():
        assert getattr(lib, f) is not None


def test_library_is_gfx950_code_object():
    # the embedded offload bundle names its target; the build is gfx950-only
    # (host-side strings of rocPRIM's arch table name other targets; only the
    # offload-bundle target ids say which code objects are embedded)
    import re
    blob = open(N.LIB_PATH, "rb").read()
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", blob))
    assert targets == {b"gfx950"}, targets


def test_abi_version():
    """The library, the header and the ctypes mirror agree (load_library refuses a
    library of another ABI: its structs would be read with the wrong layout)."""
    m = re.search(r"#define KHP_ABI_VERSION (\d+)", open(HEADER).read())
    assert N.load_library().khp_abi_version() == int(m.group(1)) == N.ABI_VERSION


def test_comm_timeout_needs_a_context_and_a_bound():
    lib = N.load_library()
    assert lib.khp_comm_set_timeout(None, 1000) == N.KHP_EINVAL
    assert b"timeout" in lib.khp_last_error()


def test_bsdf_registry_matches_kirk_factory_names():
    # BsdfFactory::getBsdf / CPU_Scene.cpp name strings (SURVEY §2 "BSDF zoo")
    lib = N.load_library()
    for i, name in enumerate(N.BSDF_NAMES):
        assert lib.khp_bsdf_kind_from_name(name.encode()) == i
        assert lib.khp_bsdf_name(i).decode() == name
        assert BsdfFactory.get_bsdf(name) == i
    assert lib.khp_bsdf_kind_from_name(b"NoSuchBSDF") == -1
    assert lib.khp_bsdf_name(99) is None
    with pytest.raises(ValueError):
        BsdfFactory.get_bsdf("NoSuchBSDF")


def test_shader_registry():
    lib = N.load_library()
    for i, name in enumerate(N.SHADER_NAMES):
        assert lib.khp_shader_kind_from_name(name.encode()) == i
        assert ShaderFactory.get_shader(name) == i
    assert lib.khp_shader_kind_from_name(b"x") == -1


def test_struct_layouts_match_header_sizes():
    # sizes implied by the header's plain-C structs (no padding surprises across the boundary)
    assert ctypes.sizeof(N.Material) == 4 * (2 + 12 + 2)
    assert ctypes.sizeof(N.Light) == 4 * (1 + 3 + 3 + 3 + 2 + 1 + 3 + 2)
    assert ctypes.sizeof(N.RenderParams) == 40
    assert ctypes.sizeof(N.Camera) == 4 * 13


def test_null_and_invalid_arguments():
    lib = N.load_library()
    assert lib.khp_host_build(None, None, None, None, None, None, None, None, None) == N.KHP_EINVAL
    assert b"null" in lib.khp_last_error()
    assert lib.khp_fibers_to_cones(1, 1, None, None, None, None) == N.KHP_EINVAL     # < 2 vertices
    sd = S.config1(8, 8)
    d = sd.desc()
    d.tri_mat[0] = 10_000                                                              # material out of range
    nn, dep = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.khp_host_build(ctypes.byref(d), ctypes.byref(nn), ctypes.byref(dep), None, None, None, None, None,
                              None) == N.KHP_EINVAL
    assert b"material" in lib.khp_last_error()


def test_create_fails_loudly_without_gpu():
    import torch  # noqa: F401  (device probing only)
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_*.py")
    lib = N.load_library()
    ctx = ctypes.c_void_p()
    assert lib.khp_create(ctypes.byref(ctx), 0, 0) == N.KHP_EDEVICE
    assert not ctx.value
    from ba_pathtracing_fur_amd.pathtracer import HipContext
    with pytest.raises(N.KhpError):
        HipContext()


def test_missing_library_is_an_error(tmp_path):
    with pytest.raises(RuntimeError, match="not built"):
        N.load_library(str(tmp_path / "libkirk_hip.so"))


def test_product_does_not_link_the_oracle():
    out = subprocess.check_output(["ldd", N.LIB_PATH], text=True)
    assert "kirk_oracle" not in out
    import ba_pathtracing_fur_amd.pathtracer as pt
    import ba_pathtracing_fur_amd.native as nat
    src = "".join(open(m.__file__).read() for m in (pt, nat, S))
    assert "import oracle" not in src and "oracle_ffi" not in src


def test_package_exports_and_leaves_hw_queues_alone():
    """Importing the package changes no process setting: GPU_MAX_HW_QUEUES is set
    only by an explicit set_hw_queues() call of the host program."""
    code = ("import os, sys; sys.path.insert(0, %r); os.environ.pop('GPU_MAX_HW_QUEUES', None); "
            "import ba_pathtracing_fur_amd as P; [getattr(P, n) for n in P.__all__]; "
            "assert 'GPU_MAX_HW_QUEUES' not in os.environ; P.set_hw_queues(8); "
            "assert os.environ['GPU_MAX_HW_QUEUES'] == '8'") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", code])


def test_ctx_params_struct_matches_header():
    """khp_ctx_params defaults (no device needed) and the ctypes layout."""
    lib = N.load_library()
    prm = N.CtxParams()
    lib.khp_ctx_params_defaults(prm)
    assert prm.as_dict() == {"fuse_frames": 32, "frames_in_flight": 1, "chunk_paths": 0, "heavy_iters": 0xFFFFFFFF,
                             "dump_bounce": -1, "trace_kernels": 0, "shade_order": 0, "serial_stages": 0, "path_order": 1,
                             "wide_from": 2, "path_kernel": 0, "ray_sort_from": 0, "lds_nodes": 0,
                             "render_ahead": 3, "path_from": 0}
    assert ctypes.sizeof(N.CtxParams) == 64  # 15 fields: 8 + 8 + 12 x 4 bytes


# ---- ABI 15: the batch queries of the shading functions -------------------------------------
def _debug_query_calls(n, null=None, obj=0, mat=0, light=0, mask=(1 << 11) - 1):
    """(name, callable(lib, ctx)) for each of the five queries on n items (arrays of at most 4: a
    larger n is to be refused before anything is read); `null` names one argument to omit."""
    f = lambda *shape: np.zeros(shape, np.float32)
    i = lambda v=0: np.full(m, v, np.int32)
    keep = []

    def a(name, arr):
        if name == null:
            return None
        keep.append(arr)
        return arr.ctypes.data_as(ctypes.c_void_p)

    m = min(max(n, 1), 4)
    d = np.tile(np.float32([0, 0, -1]), (m, 1))
    up = np.tile(np.float32([0, 0, 1]), (m, 1))
    return [
        ("khp_debug_surface", lambda lib, c: lib.khp_debug_surface(
            c, n, *(ctypes.cast(a(k, v), ctypes.POINTER(t)) for k, v, t in (
                ("orig", f(m, 3), ctypes.c_float), ("dir", d, ctypes.c_float), ("t", f(m), ctypes.c_float),
                ("object", i(), ctypes.c_int32), ("normal", f(m, 3), ctypes.c_float), ("uvw", f(m, 9), ctypes.c_float),
                ("material", i(), ctypes.c_int32))))),
        ("khp_debug_bsdf_sample", lambda lib, c: lib.khp_debug_bsdf_sample(
            c, n, mask, *(ctypes.cast(a(k, v), ctypes.POINTER(t)) for k, v, t in (
                ("object", i(obj), ctypes.c_int32), ("material", i(mat), ctypes.c_int32), ("in", up, ctypes.c_float),
                ("normal", up, ctypes.c_float), ("sample", f(m, 2), ctypes.c_float), ("hair", f(m, 2), ctypes.c_float),
                ("flags_in", i(), ctypes.c_int32), ("out_dir", f(m, 3), ctypes.c_float), ("pdf", f(m), ctypes.c_float),
                ("f", f(m, 3), ctypes.c_float), ("sample_out", f(m, 2), ctypes.c_float),
                ("flags_out", i(), ctypes.c_int32), ("valid", i(), ctypes.c_int32))))),
        ("khp_debug_bsdf_eval", lambda lib, c: lib.khp_debug_bsdf_eval(
            c, n, *(ctypes.cast(a(k, v), ctypes.POINTER(t)) for k, v, t in (
                ("object", i(obj), ctypes.c_int32), ("material", i(mat), ctypes.c_int32), ("in", up, ctypes.c_float),
                ("normal", up, ctypes.c_float), ("out", up, ctypes.c_float), ("f", f(m, 3), ctypes.c_float))))),
        ("khp_debug_light_dir", lambda lib, c: lib.khp_debug_light_dir(
            c, n, *(ctypes.cast(a(k, v), ctypes.POINTER(t)) for k, v, t in (
                ("light", i(light), ctypes.c_int32), ("point", f(m, 3), ctypes.c_float), ("draws", f(m, 2), ctypes.c_float),
                ("ray_orig", f(m, 3), ctypes.c_float), ("ray_dir", f(m, 3), ctypes.c_float),
                ("attenuation", f(m), ctypes.c_float))))),
        ("khp_debug_light_isect", lambda lib, c: lib.khp_debug_light_isect(
            c, n, *(ctypes.cast(a(k, v), ctypes.POINTER(t)) for k, v, t in (
                ("light", i(light), ctypes.c_int32), ("orig", f(m, 3), ctypes.c_float), ("dir", d, ctypes.c_float),
                ("hit", np.zeros(m, np.uint8), ctypes.c_uint8), ("t", f(m), ctypes.c_float),
                ("emitted", f(m, 3), ctypes.c_float))))),
    ]


def test_debug_queries_need_a_context():
    lib = N.load_library()
    for name, call in _debug_query_calls(4):
        assert call(lib, None) == N.KHP_EINVAL, name
        assert b"null" in lib.khp_last_error(), name


@pytest.mark.gpu
def test_debug_queries_refuse_bad_arguments(hip_ctx):
    """Every argument of the ABI 15 queries is checked on the host: nothing out of range reaches a kernel."""
    from ba_pathtracing_fur_amd.pathtracer import HipContext
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    fresh = HipContext(0)                      # no scene yet
    try:
        for name, call in _debug_query_calls(4):
            assert call(lib, fresh.ptr) == N.KHP_ENOTREADY, name
            assert "khp_set_scene" in err(), name
        fresh.set_scene(S.config1(8, 8))       # a scene, but no tree
        for name, call in _debug_query_calls(4):
            assert call(lib, fresh.ptr) == N.KHP_ENOTREADY, name
            assert "khp_build_accel" in err(), name
    finally:
        fresh.close()
    sd = S.config2(8, 8, n_strands=20)         # 4 materials (3 Lambert + Marschner), 1 light
    hip_ctx.set_scene(sd)
    hip_ctx.build_accel()
    c = hip_ctx.ptr
    for name, call in _debug_query_calls(4):
        assert call(lib, c) == N.KHP_OK, (name, err())
    for n in (0, (1 << 20) + 1, 0xFFFFFFFF):
        for name, call in _debug_query_calls(n):
            assert call(lib, c) == N.KHP_EINVAL and "n must be" in err(), (name, n)
    args = {"khp_debug_surface": ["orig", "dir", "t", "object", "normal", "uvw", "material"],
            "khp_debug_bsdf_sample": ["object", "material", "in", "normal", "sample", "hair", "flags_in", "out_dir", "pdf",
                                      "f", "sample_out", "flags_out", "valid"],
            "khp_debug_bsdf_eval": ["object", "material", "in", "normal", "out", "f"],
            "khp_debug_light_dir": ["light", "point", "draws", "ray_orig", "ray_dir", "attenuation"],
            "khp_debug_light_isect": ["light", "orig", "dir", "hit", "t", "emitted"]}
    for k, (name, _) in enumerate(_debug_query_calls(4)):
        for arg in args[name]:
            call = _debug_query_calls(4, null=arg)[k][1]
            assert call(lib, c) == N.KHP_EINVAL and "null" in err(), (name, arg)
    bsdf = lambda **kw: [x for x in _debug_query_calls(4, **kw) if "bsdf" in x[0]]
    light = lambda **kw: [x for x in _debug_query_calls(4, **kw) if "light" in x[0]]
    for bad in (-1, sd.n_objects, 1 << 30):
        for name, call in bsdf(obj=bad):
            assert call(lib, c) == N.KHP_EINVAL and "object" in err(), (name, bad)
    for bad in (-1, len(sd.materials), 1 << 30):
        for name, call in bsdf(mat=bad):
            assert call(lib, c) == N.KHP_EINVAL and "material" in err(), (name, bad)
    for bad in (-1, len(sd.lights), 1 << 30):
        for name, call in light(light=bad):
            assert call(lib, c) == N.KHP_EINVAL and "light" in err(), (name, bad)
    # the fur instance accepts Lambert (material 0) and Marschner (3) only; any other mask is refused
    fur = (1 << 0) | (1 << 9)
    assert bsdf(mask=fur, mat=3)[0][1](lib, c) == N.KHP_OK
    assert bsdf(mask=0x7)[0][1](lib, c) == N.KHP_EINVAL and "kinds_mask" in err()


# ---- ABI 17: the queries of the light-path variant ------------------------------------------
def _bdpt_query_calls(n, null=None, light=0, j=0, bounce=0, wh=(16, 12)):
    """(name, callable(lib, ctx)) for khp_debug_bdpt_connect and khp_debug_img_connect on n items
    (arrays of at most 4) and khp_debug_light_paths; `null` names one argument to omit."""
    f = lambda *shape: np.zeros(shape, np.float32)
    keep = []

    def a(name, arr, t):
        if name == null:
            return ctypes.cast(None, ctypes.POINTER(t))
        keep.append(arr)
        return arr.ctypes.data_as(ctypes.POINTER(t))

    m = min(max(n, 1), 4)
    d = np.tile(np.float32([0, -1, 0]), (m, 1))
    o = np.tile(np.float32([0, 0.5, 0]), (m, 1))
    vert = np.tile(np.float32([1, 0, 0.9, 0, 0, -1, 0, 0.3, 0.3, 0.3]), (m, 1))
    u32, i32, u8, fl = ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint8, ctypes.c_float
    return [
        ("khp_debug_bdpt_connect", lambda lib, c: lib.khp_debug_bdpt_connect(
            c, n, a("orig", o, fl), a("dir", d, fl), a("bounce", np.full(m, bounce, np.uint32), u32),
            a("light", np.full(m, light, np.int32), i32), a("j", np.full(m, j, np.uint32), u32), a("vertex", vert, fl),
            a("hit", np.zeros(m, np.uint8), u8), a("accepted", np.zeros(m, np.uint8), u8), a("ray_orig", f(m, 3), fl),
            a("ray_dir", f(m, 3), fl), a("tmax", f(m), fl), a("cj", f(m, 3), fl))),
        ("khp_debug_img_connect", lambda lib, c: lib.khp_debug_img_connect(
            c, wh[0], wh[1], n, a("sensor", o, fl), a("j", np.full(m, j, np.uint32), u32), a("prev", vert, fl),
            a("cur", vert, fl), a("accepted", np.zeros(m, np.uint8), u8), a("dir", f(m, 3), fl), a("t", f(m), fl),
            a("cj", f(m, 3), fl))),
        ("khp_debug_light_paths", lambda lib, c: lib.khp_debug_light_paths(c, 1, 0, a("out", f(1 << 16), fl))),
    ]


BDPT_QUERY_ARGS = {"khp_debug_bdpt_connect": ["orig", "dir", "bounce", "light", "j", "vertex", "hit", "accepted", "ray_orig",
                                              "ray_dir", "tmax", "cj"],
                   "khp_debug_img_connect": ["sensor", "j", "prev", "cur", "accepted", "dir", "t", "cj"],
                   "khp_debug_light_paths": ["out"]}


def test_bdpt_queries_need_a_context():
    lib = N.load_library()
    for name, call in _bdpt_query_calls(4):
        assert call(lib, None) == N.KHP_EINVAL, name
        assert b"null" in lib.khp_last_error(), name


@pytest.mark.gpu
def test_bdpt_queries_refuse_bad_arguments(hip_ctx):
    """Every index and count of the ABI 17 queries is checked on the host: nothing out of range reaches a kernel."""
    from ba_pathtracing_fur_amd.pathtracer import HipContext
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    fresh = HipContext(0)                      # no scene yet
    try:
        for name, call in _bdpt_query_calls(4):
            assert call(lib, fresh.ptr) == N.KHP_ENOTREADY and "khp_set_scene" in err(), name
        fresh.set_scene(S.config1(8, 8))       # a scene, but no tree
        for name, call in _bdpt_query_calls(4):
            assert call(lib, fresh.ptr) == N.KHP_ENOTREADY and "khp_build_accel" in err(), name
    finally:
        fresh.close()
    sd = S.config2(8, 8, n_strands=20)         # 1 light
    hip_ctx.set_scene(sd)
    hip_ctx.build_accel()
    old = hip_ctx.set_bdpt(light_paths=16, vertices=4, image_plane=1)
    c = hip_ctx.ptr
    try:
        for name, call in _bdpt_query_calls(4):
            assert call(lib, c) == N.KHP_OK, (name, err())
        for n in (0, (1 << 20) + 1, 0xFFFFFFFF):
            for name, call in _bdpt_query_calls(n)[:2]:
                assert call(lib, c) == N.KHP_EINVAL and "n must be" in err(), (name, n)
        for k, (name, _) in enumerate(_bdpt_query_calls(4)):
            for arg in BDPT_QUERY_ARGS[name]:
                call = _bdpt_query_calls(4, null=arg)[k][1]
                assert call(lib, c) == N.KHP_EINVAL and "null" in err(), (name, arg)
        for bad in (-1, len(sd.lights), 1 << 30):
            assert _bdpt_query_calls(4, light=bad)[0][1](lib, c) == N.KHP_EINVAL and "light" in err(), bad
        for bad in (16, 1 << 31):
            for name, call in _bdpt_query_calls(4, j=bad)[:2]:
                assert call(lib, c) == N.KHP_EINVAL and "vertex index" in err(), (name, bad)
        assert _bdpt_query_calls(4, bounce=4096)[0][1](lib, c) == N.KHP_EINVAL and "bounce" in err()
        for wh in ((0, 12), (16, 0)):
            assert _bdpt_query_calls(4, wh=wh)[1][1](lib, c) == N.KHP_EINVAL and "width" in err()
        hip_ctx.set_bdpt(image_plane=0)
        assert _bdpt_query_calls(4)[1][1](lib, c) == N.KHP_EINVAL and "image_plane" in err()
        # light_paths x lights x vertices beyond 2^20 is refused before anything is allocated
        hip_ctx.set_bdpt(light_paths=65536, vertices=16, image_plane=1)
        assert 65536 * len(sd.lights) * 16 == 1 << 20
        hip_ctx.set_bdpt(light_paths=65536, vertices=16)
        two = S.config2(8, 8, n_strands=20)
        two.lights = two.lights * 2            # 2 lights: 2^21 vertices
        hip_ctx.set_scene(two)
        hip_ctx.build_accel()
        assert _bdpt_query_calls(4)[2][1](lib, c) == N.KHP_EINVAL and "2^20" in err()
        none = S.config2(8, 8, n_strands=20)
        none.lights = []
        hip_ctx.set_scene(none)
        hip_ctx.build_accel()
        hip_ctx.set_bdpt(light_paths=16, vertices=4)
        assert _bdpt_query_calls(4)[2][1](lib, c) == N.KHP_EINVAL and "no lights" in err()
    finally:
        hip_ctx.set_bdpt(**old)


# ---- kmath op by op: khp_kmath_host and khp_debug_kmath (no ABI change: new entries only) --------
def _kmath_call(entry, ctx, op=0, n=4, null=None):
    """entry(lib) over n items (arrays of 4: a larger n is to be refused before anything is read)."""
    P = ctypes.POINTER(ctypes.c_uint64)
    w, o = np.zeros((4, 3), np.uint64), np.full((4, 3), 7, np.uint64)
    a = ctypes.cast(None, P) if null == "in" else w.ctypes.data_as(P)
    b = ctypes.cast(None, P) if null == "out" else o.ctypes.data_as(P)
    lib = N.load_library()
    rc = lib.khp_kmath_host(op, n, a, b) if entry == "host" else lib.khp_debug_kmath(ctx, op, n, a, b)
    return rc, o


def _kmath_bad_arguments(entry, ctx):
    lib = N.load_library()
    err = lambda: lib.khp_last_error().decode()
    rc, o = _kmath_call(entry, ctx)
    assert rc == N.KHP_OK and not o.any(), err()                        # 0 * 0 = +0 in every item
    for op in (N.KMATH_OP["gclamp"] + 1, 1 << 16, 0xFFFFFFFF):
        rc, o = _kmath_call(entry, ctx, op=op)
        assert rc == N.KHP_EINVAL and "unknown op" in err() and (o == 7).all(), op
    for n in (0, (1 << 20) + 1, 0xFFFFFFFF):
        rc, o = _kmath_call(entry, ctx, n=n)
        assert rc == N.KHP_EINVAL and "n must be" in err() and (o == 7).all(), n
    for arg in ("in", "out"):
        rc, o = _kmath_call(entry, ctx, null=arg)
        assert rc == N.KHP_EINVAL and "null" in err() and (o == 7).all(), arg


def test_kmath_host_refuses_bad_arguments_and_debug_kmath_needs_a_context():
    _kmath_bad_arguments("host", None)
    rc, o = _kmath_call("device", None)
    assert rc == N.KHP_EINVAL and b"null" in N.load_library().khp_last_error() and (o == 7).all()
    assert len(N.KMATH_OPS) == N.KMATH_OP["gclamp"] + 1 == 48


@pytest.mark.gpu
def test_debug_kmath_refuses_bad_arguments(hip_ctx):
    """Every argument of khp_debug_kmath is checked on the host: an unknown op, a bad n or a null array launches nothing."""
    _kmath_bad_arguments("device", hip_ctx.ptr)
