"""KIRK-shaped host interface over the C-ABI.

Mirrors the plugin surface the HIP core drops in behind:
  * `PathTracer` ~ KIRK::CPU::PathTracer / CPU_Raytracer (CPU_PathTracer.h:33-166,
    CPU_Raytracer.h:16-78): init(scene), set_sample_count, set_depth, render()
    (one sample of every pixel, like one full pass of KIRK's segmented render),
    render_to_texture(), get_current_sample_count(), reset();
  * `BVH` ~ KIRK::CPU::CPU_DataStructure (CPU_DataStructure.h:25-28):
    closest_intersection / is_intersection, batched over ray arrays;
  * `BsdfFactory` / `ShaderFactory` ~ the name registries (BsdfFactory.cpp:28-55,
    ShaderFactory.cpp:29-67): unknown names raise ValueError where KIRK throws
    std::invalid_argument.
Everything runs on the GPU through libkirk_hip.so; nothing here computes pixels.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as N
from .scenes import SceneData


class BsdfFactory:
    @staticmethod
    def get_bsdf(name: str) -> int:
        lib = N.load_library()
        k = lib.khp_bsdf_kind_from_name(name.encode())
        if k < 0:
            raise ValueError(f"There is no BSDF registered with the name {name}")
        return k

    @staticmethod
    def names() -> list[str]:
        return list(N.BSDF_NAMES)


class ShaderFactory:
    @staticmethod
    def get_shader(name: str) -> int:
        lib = N.load_library()
        k = lib.khp_shader_kind_from_name(name.encode())
        if k < 0:
            raise ValueError(f"There is no Shader registered with the name {name}")
        return k


class DeviceBuffer:
    """A device allocation on a context's GPU (khp_device_alloc); freed with the object."""

    def __init__(self, ctx: "HipContext", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = ctypes.c_void_p()
        N.check(ctx.lib, ctx.lib.khp_device_alloc(ctx.ptr, self.nbytes, ctypes.byref(p)), "khp_device_alloc")
        self.ptr = p.value

    @classmethod
    def from_array(cls, ctx: "HipContext", a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(ctx, a.nbytes)
        N.check(ctx.lib, ctx.lib.khp_device_copy(ctx.ptr, b.ptr, a.ctypes.data_as(ctypes.c_void_p), a.nbytes, 1),
                "khp_device_copy")
        return b

    def to_array(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        N.check(self.ctx.lib, self.ctx.lib.khp_device_copy(self.ctx.ptr, out.ctypes.data_as(ctypes.c_void_p), self.ptr,
                                                           out.nbytes, 0), "khp_device_copy")
        return out

    def free(self):
        if self.ptr and self.ctx.ptr:
            self.ctx.lib.khp_device_free(self.ctx.ptr, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HipContext:
    """One khp_ctx: one GPU, one stream (one process per GPU)."""

    def __init__(self, device: int = 0, stats: bool = False, host_build: bool = False):
        self.lib = N.load_library()
        self.ptr = ctypes.c_void_p()
        flags = (N.CTX_STATS if stats else 0) | (N.CTX_HOST_BUILD if host_build else 0)
        N.check(self.lib, self.lib.khp_create(ctypes.byref(self.ptr), device, flags), "khp_create")
        self._scene = None

    def close(self):
        if self.ptr:
            self.lib.khp_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, scene: SceneData):
        d = scene.desc()
        N.check(self.lib, self.lib.khp_set_scene(self.ptr, ctypes.byref(d)), "khp_set_scene")
        self._scene = scene
        self._n_objects = scene.n_objects

    def hairball_device(self, n_strands: int, center, ball_radius: float, root_radius: float = 0.004,
                        verts: int = 10, seed: int = 0x4B49524B):
        """Seeded hairball cones generated in HBM (khp_gen_hairball_device): (base_r0, apex_r1, n_cones)."""
        nc = n_strands * (verts - 1)
        base, apex = DeviceBuffer(self, 16 * nc), DeviceBuffer(self, 16 * nc)
        c = np.asarray(center, np.float32)
        N.check(self.lib, self.lib.khp_gen_hairball_device(self.ptr, n_strands, verts, N.fptr(c), ball_radius,
                                                           root_radius, seed, base.ptr, apex.ptr),
                "khp_gen_hairball_device")
        return base, apex, nc

    def fur_device(self, tri_v_buf: DeviceBuffer, tri_n_buf: "DeviceBuffer | None", n_tris: int, **params):
        """Fur on a mesh that lives in HBM (khp_gen_fur_device; params: khp_fur_params
        fields): (base_r0, apex_r1, n_cones), the cones of scenes.fur_on_mesh followed
        by add_fibers, for set_scene_device(..., cones=(base, apex, n, mat))."""
        p = N.FurParams.defaults(**params)
        tv = tri_v_buf.ptr if tri_v_buf is not None else None
        tn = tri_n_buf.ptr if tri_n_buf is not None else None
        n = ctypes.c_uint64()
        N.check(self.lib, self.lib.khp_gen_fur_device(self.ptr, ctypes.byref(p), n_tris, tv, tn, 0, None, None,
                                                      ctypes.byref(n)), "khp_gen_fur_device")
        nc = n.value
        base, apex = DeviceBuffer(self, 16 * nc), DeviceBuffer(self, 16 * nc)
        N.check(self.lib, self.lib.khp_gen_fur_device(self.ptr, ctypes.byref(p), n_tris, tv, tn, nc, base.ptr, apex.ptr,
                                                      ctypes.byref(n)), "khp_gen_fur_device")
        return base, apex, nc

    def set_scene_device(self, scene: SceneData, cones=None):
        """khp_set_scene_device: the scene's geometry copied to HBM first, or, with
        cones=(base_r0, apex_r1, n, material) from hairball_device / fur_device, those cones in
        place of the scene's own (which must then be empty)."""
        d = scene.desc()
        keep = []

        def dev(a):
            b = DeviceBuffer.from_array(self, a)
            keep.append(b)
            return b.ptr

        if len(scene.tri_v):
            d.tri_v = ctypes.cast(dev(scene.tri_v), ctypes.POINTER(ctypes.c_float))
            d.tri_n = ctypes.cast(dev(scene.tri_n), ctypes.POINTER(ctypes.c_float))
            d.tri_mat = ctypes.cast(dev(scene.tri_mat), ctypes.POINTER(ctypes.c_uint32))
            d.tri_frame = ctypes.cast(dev(scene.frames()), ctypes.POINTER(ctypes.c_float))
            if scene.textures:
                d.tri_uv = ctypes.cast(dev(scene.uvs()), ctypes.POINTER(ctypes.c_float))
        if cones is not None:
            if len(scene.cone_base_r0):
                raise ValueError("scene already has cones")
            base, apex, nc, mat = cones
            d.n_cones = nc
            d.cone_base_r0 = ctypes.cast(base.ptr, ctypes.POINTER(ctypes.c_float))
            d.cone_apex_r1 = ctypes.cast(apex.ptr, ctypes.POINTER(ctypes.c_float))
            d.cone_mat = ctypes.cast(dev(np.full(nc, mat, np.uint32)), ctypes.POINTER(ctypes.c_uint32))
        elif len(scene.cone_base_r0):
            d.cone_base_r0 = ctypes.cast(dev(scene.cone_base_r0), ctypes.POINTER(ctypes.c_float))
            d.cone_apex_r1 = ctypes.cast(dev(scene.cone_apex_r1), ctypes.POINTER(ctypes.c_float))
            d.cone_mat = ctypes.cast(dev(scene.cone_mat), ctypes.POINTER(ctypes.c_uint32))
            if len(scene.cone_models):
                d.cone_model = ctypes.cast(dev(scene.cone_model), ctypes.POINTER(ctypes.c_uint32))
        N.check(self.lib, self.lib.khp_set_scene_device(self.ptr, ctypes.byref(d)), "khp_set_scene_device")
        for b in keep:
            b.free()
        self._scene = scene
        self._n_objects = d.n_tris + d.n_cones

    def build_accel(self):
        N.check(self.lib, self.lib.khp_build_accel(self.ptr), "khp_build_accel")

    def update_geometry(self, scene: SceneData) -> dict:
        """khp_update_geometry: the built tree refitted in place to `scene`'s moved vertices (the same
        object counts; only tri_v, tri_n, tri_frame, cone_base_r0 and cone_apex_r1 are read).  Returns
        khp_refit_info as a dict.  Restart the accumulation: render the next frame with first_sample = 0."""
        d = scene.desc()
        info = N.RefitInfo()
        N.check(self.lib, self.lib.khp_update_geometry(self.ptr, ctypes.byref(d), ctypes.byref(info)),
                "khp_update_geometry")
        self._scene = scene
        return info.as_dict()

    def update_geometry_device(self, scene: SceneData, cones=None) -> dict:
        """khp_update_geometry_device: as update_geometry with the geometry copied to HBM first, or, with
        cones=(base_r0, apex_r1, n) DeviceBuffers, those cones in place of the scene's own (mirrors
        set_scene_device; a fourth element, the material, is ignored)."""
        d = scene.desc()
        keep = []

        def dev(a):
            b = DeviceBuffer.from_array(self, a)
            keep.append(b)
            return ctypes.cast(b.ptr, ctypes.POINTER(ctypes.c_float))

        if len(scene.tri_v):
            d.tri_v = dev(scene.tri_v)
            d.tri_n = dev(scene.tri_n)
            d.tri_frame = dev(scene.frames())
        if cones is not None:
            if len(scene.cone_base_r0):
                raise ValueError("scene already has cones")
            base, apex, nc = cones[:3]
            d.n_cones = nc
            d.cone_base_r0 = ctypes.cast(base.ptr, ctypes.POINTER(ctypes.c_float))
            d.cone_apex_r1 = ctypes.cast(apex.ptr, ctypes.POINTER(ctypes.c_float))
        elif len(scene.cone_base_r0):
            d.cone_base_r0 = dev(scene.cone_base_r0)
            d.cone_apex_r1 = dev(scene.cone_apex_r1)
        info = N.RefitInfo()
        try:
            N.check(self.lib, self.lib.khp_update_geometry_device(self.ptr, ctypes.byref(d), ctypes.byref(info)),
                    "khp_update_geometry_device")
        finally:
            for b in keep:
                b.free()
        self._scene = scene
        return info.as_dict()

    def refit_info(self) -> dict:
        """khp_get_refit_info: the info of the last update_geometry (before the first: the built tree's)."""
        info = N.RefitInfo()
        N.check(self.lib, self.lib.khp_get_refit_info(self.ptr, ctypes.byref(info)), "khp_get_refit_info")
        return info.as_dict()

    def params(self) -> dict:
        """khp_get_params: the context's scheduling parameters (khp_ctx_params)."""
        prm = N.CtxParams()
        N.check(self.lib, self.lib.khp_get_params(self.ptr, ctypes.byref(prm)), "khp_get_params")
        return prm.as_dict()

    def set_params(self, **kw) -> dict:
        """khp_set_params with the given fields changed (fuse_frames, frames_in_flight,
        chunk_paths, heavy_iters, dump_bounce, trace_kernels, shade_order, serial_stages,
        path_order, wide_from, path_kernel, ray_sort_from, lds_nodes, render_ahead); returns the previous values."""
        prm = N.CtxParams()
        N.check(self.lib, self.lib.khp_get_params(self.ptr, ctypes.byref(prm)), "khp_get_params")
        old = prm.as_dict()
        for k, v in kw.items():
            if k not in old:
                raise AttributeError(f"khp_ctx_params has no field {k}")
            setattr(prm, k, int(v))
        N.check(self.lib, self.lib.khp_set_params(self.ptr, ctypes.byref(prm)), "khp_set_params")
        return old

    def set_camera(self, camera: "N.Camera"):
        """khp_set_camera (ABI 13): a new camera for the next render, nothing rebuilt
        (KIRK's GUI moving the Camera between PathTracer::render calls)."""
        N.check(self.lib, self.lib.khp_set_camera(self.ptr, ctypes.byref(camera)), "khp_set_camera")

    def set_bdpt(self, **kw) -> dict:
        """khp_set_bdpt with the given khp_bdpt_params fields changed (enabled,
        light_paths, vertices, bias, bounce_bias, min_pdf); returns the previous values."""
        prm = N.BdptParams()
        N.check(self.lib, self.lib.khp_get_bdpt(self.ptr, ctypes.byref(prm)), "khp_get_bdpt")
        old = prm.as_dict()
        for k, v in kw.items():
            if k not in old:
                raise AttributeError(f"khp_bdpt_params has no field {k}")
            setattr(prm, k, v)
        N.check(self.lib, self.lib.khp_set_bdpt(self.ptr, ctypes.byref(prm)), "khp_set_bdpt")
        return old

    def set_hair_lobes(self, lobes: int) -> int:
        """khp_set_hair_lobes (ABI 16): the lobes of Marschner's fibre model the next renders
        trace, a non-empty set of HAIR_LOBE_R / _TT / _TRT (the default, R, is KIRK as
        shipped); nothing is rebuilt.  Returns the previous set."""
        old = self.hair_lobes
        prm = N.HairLobes(int(lobes), 0)
        N.check(self.lib, self.lib.khp_set_hair_lobes(self.ptr, ctypes.byref(prm)), "khp_set_hair_lobes")
        return old

    @property
    def hair_lobes(self) -> int:
        """khp_get_hair_lobes: the enabled lobes (HAIR_LOBE_* bits)."""
        prm = N.HairLobes()
        N.check(self.lib, self.lib.khp_get_hair_lobes(self.ptr, ctypes.byref(prm)), "khp_get_hair_lobes")
        return int(prm.lobes)

    def set_lens(self, radius: float, focus_distance: float = 11.0, focus: int = N.LENS_FOCUS_KIRK) -> dict:
        """khp_set_lens: the thin-lens camera of the next renders (KIRK's Camera::transformToDof,
        which its path tracer never calls).  radius 0, the default, is the pinhole; focus is
        LENS_FOCUS_KIRK (in focus: a sphere about the camera) or LENS_FOCUS_PLANE (a plane at
        right angles to the axis); nothing is rebuilt.  Returns the previous lens()."""
        old = self.lens()
        prm = N.Lens(float(radius), float(focus_distance), int(focus), 0)
        N.check(self.lib, self.lib.khp_set_lens(self.ptr, ctypes.byref(prm)), "khp_set_lens")
        return old

    def lens(self) -> dict:
        """khp_get_lens: radius, focus_distance and focus of the context's lens."""
        prm = N.Lens()
        N.check(self.lib, self.lib.khp_get_lens(self.ptr, ctypes.byref(prm)), "khp_get_lens")
        return prm.as_dict()

    def set_env_light(self, rgb, scale: float = 1.0, rotation: float = 0.0, nee: bool = True, select: float = 0.5,
                      device_shape=None) -> None:
        """khp_set_env_light: light the next renders by a latitude-longitude map of float32 radiance,
        rgb (height, width, 3), row 0 the -y pole.  The map is copied and its sampling table built on the
        device; nee=False leaves the map to escaping rays alone; select is the chance that a hit's one
        shadow ray goes to the map when the scene also has lights.  rgb may be a device address (int) of
        this context's GPU with device_shape = (height, width)."""
        if device_shape is not None:
            h, w = (int(v) for v in device_shape)
            prm = N.EnvLight(w, h, N.ENV_LIGHT_DEVICE, int(bool(nee)), float(scale), float(rotation), float(select), 0,
                             rgb.ptr if isinstance(rgb, DeviceBuffer) else int(rgb))
        else:
            prm, _keep = _env_light_arg(rgb, scale, rotation, nee, select)
        N.check(self.lib, self.lib.khp_set_env_light(self.ptr, ctypes.byref(prm)), "khp_set_env_light")

    def clear_env_light(self) -> None:
        """khp_set_env_light with a 0 x 0 map: the context's renders are KIRK's again."""
        prm = N.EnvLight()
        self.lib.khp_env_light_defaults(ctypes.byref(prm))
        N.check(self.lib, self.lib.khp_set_env_light(self.ptr, ctypes.byref(prm)), "khp_set_env_light")

    def env_light(self) -> dict:
        """khp_get_env_light: width, height (0 x 0: off), nee, scale, rotation and select."""
        prm = N.EnvLight()
        N.check(self.lib, self.lib.khp_get_env_light(self.ptr, ctypes.byref(prm)), "khp_get_env_light")
        return prm.as_dict()

    def debug_env_light_tables(self) -> dict:
        """khp_debug_env_light_tables: the sampling table the context built on the device."""
        e = self.env_light()
        t = _env_tables(e["width"], e["height"])
        N.check(self.lib, self.lib.khp_debug_env_light_tables(self.ptr, N.uptr(t["weight"]), N.uptr(t["row_cdf"]),
                                                              _u64ptr(t["marginal"])), "khp_debug_env_light_tables")
        return t

    def debug_env_light(self, draws, dir_in) -> dict:
        """khp_debug_env_light: the renderer's own sampler over draws (n, 2) and evaluation over dir_in (n, 3)
        -> a dict of dir, pdf, radiance, valid (the samples) and e_radiance, e_pdf (the evaluations)."""
        u = np.ascontiguousarray(draws, np.float32).reshape(-1, 2)
        n = len(u)
        d = np.ascontiguousarray(dir_in, np.float32).reshape(n, 3)
        r = {"dir": np.empty((n, 3), np.float32), "pdf": np.empty(n, np.float32),
             "radiance": np.empty((n, 3), np.float32), "valid": np.empty(n, np.int32),
             "e_radiance": np.empty((n, 3), np.float32), "e_pdf": np.empty(n, np.float32)}
        N.check(self.lib, self.lib.khp_debug_env_light(
            self.ptr, n, N.fptr(u), N.fptr(d), N.fptr(r["dir"]), N.fptr(r["pdf"]), N.fptr(r["radiance"]),
            r["valid"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), N.fptr(r["e_radiance"]), N.fptr(r["e_pdf"])),
            "khp_debug_env_light")
        return r

    def debug_kmath(self, op, items) -> np.ndarray:
        """khp_debug_kmath: one op of csrc/kmath_ops.h (a name of native.KMATH_OPS or its number) over
        items (n, 3) of raw uint64 words, one thread per item on the device; returns the (n, 3) output words."""
        w, o = _kmath_items(items)
        N.check(self.lib, self.lib.khp_debug_kmath(self.ptr, _kmath_op(op), len(w), _u64ptr(w), _u64ptr(o)),
                "khp_debug_kmath")
        return o

    def debug_camera_rays(self, width: int, pixels, samples, seed: int = 0x4B49524B):
        """khp_debug_camera_rays: the renderer's own camera rays (origins, directions) of the
        (pixel, sample) pairs, with the context's camera and lens; nothing of the context is touched."""
        px, sm = _ray_items(pixels, samples)
        o, d = np.empty((len(px), 3), np.float32), np.empty((len(px), 3), np.float32)
        N.check(self.lib, self.lib.khp_debug_camera_rays(self.ptr, int(width), int(seed), len(px), N.uptr(px),
                                                         N.uptr(sm), N.fptr(o), N.fptr(d)), "khp_debug_camera_rays")
        return o, d

    def render(self, width, height, spp, depth, seed=0x4B49524B, first_sample=0, tile_size=64, tile_rank=0,
               tile_nranks=1, out: np.ndarray | None = None, readback=True, stats=False,
               async_: bool = False) -> np.ndarray | None:
        """khp_render.  async_=True (no readback, no stats) enqueues the frame and
        returns at once; frames in flight overlap; sync() completes them."""
        if async_:
            readback = False
        flags = ((0 if readback else N.RENDER_NO_READBACK) | (N.RENDER_STATS if stats else 0) |
                 (N.RENDER_ASYNC if async_ else 0))
        p = N.RenderParams(width, height, spp, depth, seed, first_sample, tile_size, tile_rank, tile_nranks, flags)
        if readback and out is None:
            out = np.zeros((height, width, 3), np.float32)
        ptr = out.ctypes.data_as(ctypes.c_void_p) if (readback and out is not None) else None
        N.check(self.lib, self.lib.khp_render(self.ptr, ctypes.byref(p), ptr), "khp_render")
        return out

    AOV_CHANNELS = tuple(N.AOV_CHANNELS)   # normal, albedo, tangent, depth, coverage, object

    def render_aov(self, width, height, spp, seed=0x4B49524B, first_sample=0, tile_size=64, tile_rank=0,
                   tile_nranks=1, channels=AOV_CHANNELS, out: dict | None = None) -> dict:
        """khp_render_aov: the first hit's features per pixel over samples first_sample ..
        first_sample + spp - 1 of the rays render() traces -- normal, albedo, tangent (H, W, 3),
        depth, coverage (H, W) float32, each the sample mean premultiplied by coverage, and
        object (H, W) int32, the first sample's object id or -1 -- as a dict of the `channels`
        asked for.  Renders nothing: framebuffer, sample counts and frames in flight stay as
        they are.  `out` supplies the arrays to write into (a tile rank leaves the pixels it
        does not own untouched); otherwise they start as zeros."""
        channels = tuple(channels)
        for ch in channels:
            if ch not in N.AOV_CHANNELS:
                raise ValueError(f"khp_render_aov has no channel {ch!r} (one of {', '.join(N.AOV_CHANNELS)})")
        res, buf = {}, N.AovBuffers()
        for ch in channels:
            tail, dtype = N.AOV_CHANNELS[ch]
            a = out[ch] if out is not None and ch in out else np.zeros((height, width) + tail, dtype)
            if a.dtype != dtype or a.shape != (height, width) + tail or not a.flags.c_contiguous:
                raise ValueError(f"channel {ch}: a C-contiguous {np.dtype(dtype).name} array of shape "
                                 f"{(height, width) + tail} is needed")
            setattr(buf, ch, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32 if ch == "object" else ctypes.c_float)))
            res[ch] = a
        p = N.RenderParams(width, height, spp, 0, seed, first_sample, tile_size, tile_rank, tile_nranks, 0)
        N.check(self.lib, self.lib.khp_render_aov(self.ptr, ctypes.byref(p), ctypes.byref(buf)), "khp_render_aov")
        return res

    def denoise(self, width, height, guides: dict, colour=None, out=None, device: bool = False, **params):
        """khp_denoise: the guided a-trous filter of an (H, W, 3) float32 frame
        over the planes render_aov returns.  `guides` is that dict (missing planes are NULL: a
        term whose sigma is > 0 needs its plane); `colour` is the frame, or None for the
        context's framebuffer (read, never written); `out` receives the result (may be
        `colour`), a new array if None.  device=True: guides, colour and out are DeviceBuffers
        of this context (out is then required).  **params: khp_denoise_params fields over
        khp_denoise_params_defaults (iterations, sigma_*, clamp, flags; demodulate=True sets
        KHP_DENOISE_DEMODULATE).  Returns out."""
        p, buf, keep = _denoise_args(width, height, guides, device, params)
        if device:
            for name, b in (("colour", colour), ("out", out)):
                if b is not None and not isinstance(b, DeviceBuffer):
                    raise ValueError(f"{name}: a DeviceBuffer is needed with device=True")
                if b is not None and b.nbytes < 12 * width * height:
                    raise ValueError(f"{name}: a DeviceBuffer of {12 * width * height} bytes is needed")
            if out is None:
                raise ValueError("out: a DeviceBuffer is needed with device=True")
            cptr, optr = (colour.ptr if colour is not None else None), out.ptr
        else:
            if colour is not None:
                _frame_check("colour", colour, width, height)
            if out is None:
                out = np.zeros((height, width, 3), np.float32)
            _frame_check("out", out, width, height)
            cptr = colour.ctypes.data_as(ctypes.c_void_p) if colour is not None else None
            optr = out.ctypes.data_as(ctypes.c_void_p)
        N.check(self.lib, self.lib.khp_denoise(self.ptr, ctypes.byref(p), cptr, ctypes.byref(buf), optr), "khp_denoise")
        del keep
        return out

    def denoise_var(self, width, height, guides: dict, colour=None, variance=None, moments=None, out=None,
                    out_variance=False, device: bool = False, **params):
        """khp_denoise_var: denoise()'s filter with sigma_color in standard deviations
        of each pixel's measured noise.  The noise is `variance`, an (H, W) float32 plane holding the
        variance of each pixel's mean (channels summed), or `moments`, the dict read_moments returns
        (its m2 and count are used); with neither it is this context's moments state, read in place
        (set_moments(True) first), and `colour=None` is then the moments' mean -- otherwise the
        framebuffer, as for denoise().  `out_variance`: True, or an (H, W) array to write into, to
        get the filtered variance too (+inf where unknown).  device=True: every array is a
        DeviceBuffer of this context (out is then required).  **params: khp_denoise_params fields
        as for denoise() (demodulate is refused: KHP_EUNSUPPORTED), and prefilter (0 / 1) and floor
        of khp_denoise_noise.  Returns out, or (out, out_variance) when that was asked for."""
        params = dict(params)
        z, ov, keep_z = _noise_args(self, width, height, variance, moments, out_variance, device, params, True)
        p, buf, keep = _denoise_args(width, height, guides, device, params)
        if device:
            for name, b in (("colour", colour), ("out", out)):
                if b is not None and not isinstance(b, DeviceBuffer):
                    raise ValueError(f"{name}: a DeviceBuffer is needed with device=True")
                if b is not None and b.nbytes < 12 * width * height:
                    raise ValueError(f"{name}: a DeviceBuffer of {12 * width * height} bytes is needed")
            if out is None:
                raise ValueError("out: a DeviceBuffer is needed with device=True")
            cptr, optr = (colour.ptr if colour is not None else None), out.ptr
        else:
            if colour is not None:
                _frame_check("colour", colour, width, height)
            if out is None:
                out = np.zeros((height, width, 3), np.float32)
            _frame_check("out", out, width, height)
            cptr = colour.ctypes.data_as(ctypes.c_void_p) if colour is not None else None
            optr = out.ctypes.data_as(ctypes.c_void_p)
        N.check(self.lib, self.lib.khp_denoise_var(self.ptr, ctypes.byref(p), cptr, ctypes.byref(buf), ctypes.byref(z), optr),
                "khp_denoise_var")
        del keep, keep_z
        return out if ov is None else (out, ov)

    def reproject(self, width, height, cur: dict, hist: dict | None = None, out: dict | None = None,
                  device: bool = False, **params) -> dict:
        """khp_reproject: carry the previous camera's frame `hist` into the current frame
        `cur` and blend.  A frame is a dict: "camera" (an N.Camera), "colour" (H, W, 3), "aov" (the dict
        render_aov returned with that camera; `cur` needs depth and coverage, the rest as the enabled
        tests ask), optionally "variance" (H, W: the variance of each pixel's mean, channels summed), and
        for `hist` "length" (H, W: the effective samples behind each pixel).  hist=None starts a history.
        Returns a dict of the outputs "colour", "length", "variance" (+inf where unknown) and "motion"
        (H, W, 2): new arrays, or those of `out` (a value of None leaves that output out; out["colour"]
        may be cur["colour"]).  The returned dict plus cur's camera and aov is the next call's `hist`.
        device=True: every array is a DeviceBuffer of this context.  **params: khp_reproject_params
        fields over khp_reproject_params_defaults (samples, max_history, depth_tol, normal_tol,
        tangent_tol, coverage_tol, flags; match_object=True sets KHP_REPROJECT_MATCH_OBJECT).  Touches no
        state of the context."""
        p, cf, hf, o, res, keep = _reproject_args(self, width, height, cur, hist, out, device, params)
        N.check(self.lib, self.lib.khp_reproject(self.ptr, ctypes.byref(p), ctypes.byref(cf),
                                                 ctypes.byref(hf) if hf is not None else None, ctypes.byref(o)),
                "khp_reproject")
        del keep
        return res

    MOMENTS_PLANES = tuple(N.MOMENTS_PLANES)   # mean, m2, count, bad, rel_error

    def set_moments(self, enabled: bool) -> bool:
        """khp_set_moments: switch the per-pixel sample moments on or off.  Enabling
        makes a zeroed state beside the framebuffer, folded by the renders that follow; disabling
        frees it; the value it already has is a no-op.  Frames and timings with it off are as
        without it.  Returns the previous value."""
        old = self.moments()
        m = N.Moments(1 if enabled else 0)
        N.check(self.lib, self.lib.khp_set_moments(self.ptr, ctypes.byref(m)), "khp_set_moments")
        return old

    def moments(self) -> bool:
        """khp_get_moments: whether the sample moments are on."""
        m = N.Moments()
        N.check(self.lib, self.lib.khp_get_moments(self.ptr, ctypes.byref(m)), "khp_get_moments")
        return bool(m.enabled)

    def read_moments(self, width, height, device: bool = False, planes=MOMENTS_PLANES, out: dict | None = None) -> dict:
        """khp_read_moments: the `planes` asked for of the moments state as a dict -- mean, m2
        (H, W, 3) float32: the finite samples' mean and sum of squared deviations; count, bad
        (H, W) uint32: finite and rejected samples; rel_error (H, W) float32: the relative standard
        error of the pixel's mean, +inf below two samples.  width and height are the framebuffer's.
        device=True: the planes are DeviceBuffers of this context (KHP_MOMENTS_DEVICE).  `out`
        supplies the arrays (or DeviceBuffers) to write into; otherwise they are made here."""
        planes = tuple(planes)
        for ch in planes:
            if ch not in N.MOMENTS_PLANES:
                raise ValueError(f"khp_read_moments has no plane {ch!r} (one of {', '.join(N.MOMENTS_PLANES)})")
        res, buf = {}, N.MomentsBuffers()
        for ch in planes:
            tail, dtype = N.MOMENTS_PLANES[ch]
            shape = (height, width) + tail
            a = out[ch] if out is not None and ch in out else None
            if device:
                need = int(np.prod(shape)) * 4
                if a is None:
                    a = DeviceBuffer(self, need)
                if not isinstance(a, DeviceBuffer) or a.nbytes < need:
                    raise ValueError(f"plane {ch}: a DeviceBuffer of {need} bytes is needed with device=True")
                ptr = a.ptr
            else:
                if a is None:
                    a = np.zeros(shape, dtype)
                if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape or not a.flags.c_contiguous:
                    raise ValueError(f"plane {ch}: a C-contiguous {np.dtype(dtype).name} array of shape {shape} is needed")
                ptr = a.ctypes.data
            setattr(buf, ch, ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float if dtype == np.float32 else ctypes.c_uint32)))
            res[ch] = a
        N.check(self.lib, self.lib.khp_read_moments(self.ptr, N.MOMENTS_DEVICE if device else 0, ctypes.byref(buf)),
                "khp_read_moments")
        return res

    def render_adaptive(self, width, height, spp, depth, seed=0x4B49524B, first_sample=0, threshold=None,
                        min_samples=None, max_samples=None, tile_size=64, tile_rank=0, tile_nranks=1, out=None,
                        readback=True):
        """khp_render_adaptive: samples first_sample .. first_sample + spp - 1 of the
        ACTIVE pixels only -- those whose rel_error (read_moments) is still above `threshold`, or that
        have fewer than `min_samples` samples, and fewer than `max_samples` (0: no cap); every owned
        pixel when first_sample == 0.  set_moments(True) first.  The moments are folded as render()
        folds them and the framebuffer takes `mean` on the active pixels; the others keep state and
        framebuffer.  Parameters left None are khp_adaptive_defaults' (0.05, 8, 0).  `out`: an
        (H, W, 3) float32 array, or a DeviceBuffer of this context (KHP_RENDER_OUT_DEVICE).  Returns
        (frame or None, {"owned": the rank's pixels, "active": those traced})."""
        a = _adaptive_params(threshold, min_samples, max_samples)
        flags = 0 if readback else N.RENDER_NO_READBACK
        ptr = None
        if readback and isinstance(out, DeviceBuffer):
            if out.nbytes < 12 * width * height:
                raise ValueError(f"out: a DeviceBuffer of {12 * width * height} bytes is needed")
            flags |= N.RENDER_OUT_DEVICE
            ptr = out.ptr
        elif readback:
            if out is None:
                out = np.zeros((height, width, 3), np.float32)
            _frame_check("out", out, width, height)
            ptr = out.ctypes.data_as(ctypes.c_void_p)
        p = N.RenderParams(width, height, spp, depth, seed, first_sample, tile_size, tile_rank, tile_nranks, flags)
        res = N.AdaptiveResult()
        N.check(self.lib, self.lib.khp_render_adaptive(self.ptr, ctypes.byref(p), ctypes.byref(a), ctypes.byref(res), ptr),
                "khp_render_adaptive")
        return (out if readback else None), {"owned": int(res.owned), "active": int(res.active)}

    def render_to_error(self, width, height, spp, depth, threshold, max_passes, seed=0x4B49524B, min_samples=None,
                        max_samples=None, tile_size=64, tile_rank=0, tile_nranks=1) -> list:
        """Adaptive passes of `spp` samples from sample 0 until no pixel is active or `max_passes`
        passes ran (nothing is read back; read_framebuffer and read_moments afterwards).  Returns the
        active count of every pass run, the first being every owned pixel."""
        counts = []
        for k in range(int(max_passes)):
            _f, res = self.render_adaptive(width, height, spp, depth, seed=seed, first_sample=k * spp,
                                           threshold=threshold, min_samples=min_samples, max_samples=max_samples,
                                           tile_size=tile_size, tile_rank=tile_rank, tile_nranks=tile_nranks,
                                           readback=False)
            counts.append(res["active"])
            if res["active"] == 0:
                break
        return counts

    def debug_adaptive_select(self, state: dict, owned, first_sample: int, **params) -> np.ndarray:
        """khp_debug_adaptive_select: the selection kernels of render_adaptive alone, over a caller's
        state (mean, m2, count, bad by pixel) and owned list, in scratch of their own: the active
        pixels, in owned order.  **params: threshold, min_samples, max_samples."""
        a = _adaptive_params(**params)
        buf, own, n_pix, keep = _select_args(state, owned)
        act = np.empty(max(1, own.size), np.uint32)
        n = ctypes.c_uint32()
        N.check(self.lib, self.lib.khp_debug_adaptive_select(self.ptr, ctypes.byref(a), int(first_sample), n_pix,
                                                             ctypes.byref(buf), own.size, N.uptr(own), N.uptr(act),
                                                             ctypes.byref(n)), "khp_debug_adaptive_select")
        del keep
        return act[:n.value].copy()

    def debug_adaptive_list(self, timing: bool = False):
        """khp_debug_adaptive_list: the last adaptive pass's active pixels, in owned order; with
        timing=True, (pixels, the device milliseconds of that pass's selection)."""
        n, ms = ctypes.c_uint32(), ctypes.c_double()
        N.check(self.lib, self.lib.khp_debug_adaptive_list(self.ptr, ctypes.byref(n), None, None),
                "khp_debug_adaptive_list")
        pix = np.empty(max(1, n.value), np.uint32)
        N.check(self.lib, self.lib.khp_debug_adaptive_list(self.ptr, ctypes.byref(n), N.uptr(pix), ctypes.byref(ms)),
                "khp_debug_adaptive_list")
        return (pix[:n.value].copy(), ms.value) if timing else pix[:n.value].copy()

    def sync(self):
        """khp_sync: complete every asynchronous frame; stats() then sums them."""
        N.check(self.lib, self.lib.khp_sync(self.ptr), "khp_sync")

    def read_bvh(self) -> dict:
        """The tree khp_build_accel built (khp_read_bvh), in khp_host_build's layout."""
        nn, dep = ctypes.c_uint32(), ctypes.c_uint32()
        N.check(self.lib, self.lib.khp_read_bvh(self.ptr, ctypes.byref(nn), ctypes.byref(dep), None, None, None, None),
                "khp_read_bvh")
        n = nn.value
        boxes = np.empty((n, 6), np.float32)
        first = np.empty(n, np.int32)
        count = np.empty(n, np.int32)
        ids = np.empty(getattr(self, "_n_objects", None) or self._scene.n_objects, np.int32)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        N.check(self.lib, self.lib.khp_read_bvh(self.ptr, ctypes.byref(nn), ctypes.byref(dep), N.fptr(boxes), ip(first),
                                                ip(count), ip(ids)), "khp_read_bvh")
        return {"boxes": boxes, "first": first, "count": count, "ids": ids, "depth": dep.value}

    def read_layout(self) -> dict:
        """The traversal records in HBM (khp_read_layout): node records as (n, 16)
        uint32 words, primitive records (n_slots, 16) float32, aux (n_slots, 4) uint32."""
        nr, ns = ctypes.c_uint32(), ctypes.c_uint32()
        N.check(self.lib, self.lib.khp_read_layout(self.ptr, ctypes.byref(nr), ctypes.byref(ns), None, None, None),
                "khp_read_layout")
        nodes = np.zeros((nr.value, 16), np.uint32)
        prims = np.zeros((ns.value, 16), np.float32)
        aux = np.zeros((ns.value, 4), np.uint32)
        N.check(self.lib, self.lib.khp_read_layout(self.ptr, ctypes.byref(nr), ctypes.byref(ns),
                                                   nodes.ctypes.data_as(ctypes.c_void_p), N.fptr(prims),
                                                   N.uptr(aux)), "khp_read_layout")
        return {"nodes": nodes, "prims": prims, "aux": aux}

    def read_framebuffer(self, width, height) -> np.ndarray:
        out = np.zeros((height, width, 3), np.float32)
        N.check(self.lib, self.lib.khp_read_framebuffer(self.ptr, N.fptr(out)), "khp_read_framebuffer")
        return out

    def read_rgba8(self, width, height, tonemap: "N.Tonemap | None" = None) -> np.ndarray:
        """Device output stage (khp_read_rgba8): (H, W, 4) uint8, row 0 = bottom.

        tonemap=None: Texture::setPixel of the running mean; otherwise
        Tonemapper::map first (PathTracer::applyToneMapping)."""
        out = np.zeros((height, width, 4), np.uint8)
        tm = ctypes.byref(tonemap) if tonemap is not None else None
        N.check(self.lib, self.lib.khp_read_rgba8(self.ptr, tm, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                "khp_read_rgba8")
        return out

    def read_rgba8_async(self, out: np.ndarray) -> int:
        """khp_read_rgba8_async: enqueue the 8-bit texture after the frames enqueued so
        far into `out` ((H, W, 4) uint8, kept alive by the caller); returns the ticket."""
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        t = ctypes.c_uint64()
        N.check(self.lib, self.lib.khp_read_rgba8_async(self.ptr, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                        ctypes.byref(t)), "khp_read_rgba8_async")
        return t.value

    def snapshot_wait(self, ticket: int, wait: bool = True) -> bool:
        """khp_snapshot_wait: True once snapshot `ticket` is in its buffer."""
        st = self.lib.khp_snapshot_wait(self.ptr, ticket, 1 if wait else 0)
        if st == N.KHP_ENOTREADY and not wait:
            return False
        N.check(self.lib, st, "khp_snapshot_wait")
        return True

    def trace_closest(self, orig, direction):
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        n = len(o)
        t = np.empty(n, np.float32)
        obj = np.empty(n, np.int32)
        uv = np.empty((n, 2), np.float32)
        N.check(self.lib, self.lib.khp_trace_closest(self.ptr, n, N.fptr(o), N.fptr(d), N.fptr(t),
                                                     obj.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                     N.fptr(uv)), "khp_trace_closest")
        return t, obj, uv

    def trace_any(self, orig, direction, tmax):
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        tm = np.ascontiguousarray(tmax, np.float32).reshape(-1)
        hit = np.empty(len(o), np.uint8)
        N.check(self.lib, self.lib.khp_trace_any(self.ptr, len(o), N.fptr(o), N.fptr(d), N.fptr(tm),
                                                 hit.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
                "khp_trace_any")
        return hit.astype(bool)

    # ---- ABI 15 batch queries of the shading functions (test hooks) ----
    KINDS_ALL = (1 << 11) - 1          # every khp_bsdf_kind
    KINDS_FUR = (1 << 0) | (1 << 9)    # Lambert + Marschner: the set compiled for fur-only scenes
    KINDS_ALL_HAIR = (1 << 12) - 1     # the eleven and ChiangHairBSDF: the set compiled for scenes with kind 11
    KINDS_FUR_HAIR = (1 << 0) | (1 << 11)   # Lambert + ChiangHairBSDF (the same instance)

    def debug_surface(self, orig, direction):
        """khp_debug_surface: closest hit and the surface there, per ray."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        n = len(o)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        r = {"t": np.empty(n, np.float32), "obj": np.empty(n, np.int32), "n": np.empty((n, 3), np.float32),
             "uvw": np.empty((n, 3, 3), np.float32), "mat": np.empty(n, np.int32)}
        N.check(self.lib, self.lib.khp_debug_surface(self.ptr, n, N.fptr(o), N.fptr(d), N.fptr(r["t"]), ip(r["obj"]),
                                                     N.fptr(r["n"]), N.fptr(r["uvw"]), ip(r["mat"])),
                "khp_debug_surface")
        return r

    def debug_bsdf_sample(self, obj, mat, ray_in, normal, sample, hair, flags_in, kinds_mask=None):
        """khp_debug_bsdf_sample on n items; kinds_mask: KINDS_ALL (default), KINDS_FUR, or, for items
        of kind 11, KINDS_ALL_HAIR or KINDS_FUR_HAIR."""
        ob = np.ascontiguousarray(obj, np.int32).reshape(-1)
        n = len(ob)
        mt = np.ascontiguousarray(mat, np.int32).reshape(-1)
        ri = np.ascontiguousarray(ray_in, np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        sm = np.ascontiguousarray(sample, np.float32).reshape(-1, 2)
        hu = np.ascontiguousarray(hair, np.float32).reshape(-1, 2)
        fl = np.ascontiguousarray(flags_in, np.int32).reshape(-1)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        r = {"out": np.empty((n, 3), np.float32), "pdf": np.empty(n, np.float32), "f": np.empty((n, 3), np.float32),
             "sample": np.empty((n, 2), np.float32), "flags": np.empty(n, np.int32), "valid": np.empty(n, np.int32)}
        N.check(self.lib, self.lib.khp_debug_bsdf_sample(
            self.ptr, n, self.KINDS_ALL if kinds_mask is None else kinds_mask, ip(ob), ip(mt), N.fptr(ri), N.fptr(nn),
            N.fptr(sm), N.fptr(hu), ip(fl), N.fptr(r["out"]), N.fptr(r["pdf"]), N.fptr(r["f"]), N.fptr(r["sample"]),
            ip(r["flags"]), ip(r["valid"])), "khp_debug_bsdf_sample")
        return r

    def debug_hair_sample(self, lobes, obj, mat, ray_in, normal, hair, lobe_u, flags_in):
        """khp_debug_hair_sample (ABI 16) on n items of Marschner materials: the three-call
        TT / TRT state machine with the lobe set `lobes` (not the context's setting)."""
        ob = np.ascontiguousarray(obj, np.int32).reshape(-1)
        n = len(ob)
        mt = np.ascontiguousarray(mat, np.int32).reshape(-1)
        ri = np.ascontiguousarray(ray_in, np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        hu = np.ascontiguousarray(hair, np.float32).reshape(-1, 2)
        lu = np.ascontiguousarray(lobe_u, np.float32).reshape(-1)
        fl = np.ascontiguousarray(flags_in, np.int32).reshape(-1)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        r = {"out": np.empty((n, 3), np.float32), "pdf": np.empty(n, np.float32), "f": np.empty((n, 3), np.float32),
             "sample": np.empty((n, 2), np.float32), "flags": np.empty(n, np.int32), "valid": np.empty(n, np.int32)}
        N.check(self.lib, self.lib.khp_debug_hair_sample(
            self.ptr, n, int(lobes), ip(ob), ip(mt), N.fptr(ri), N.fptr(nn), N.fptr(hu), N.fptr(lu), ip(fl),
            N.fptr(r["out"]), N.fptr(r["pdf"]), N.fptr(r["f"]), N.fptr(r["sample"]), ip(r["flags"]), ip(r["valid"])),
            "khp_debug_hair_sample")
        return r

    def debug_bsdf_eval(self, obj, mat, ray_in, normal, out):
        """khp_debug_bsdf_eval on n items -> f (n, 3)."""
        ob = np.ascontiguousarray(obj, np.int32).reshape(-1)
        n = len(ob)
        mt = np.ascontiguousarray(mat, np.int32).reshape(-1)
        ri = np.ascontiguousarray(ray_in, np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        oo = np.ascontiguousarray(out, np.float32).reshape(-1, 3)
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        f = np.empty((n, 3), np.float32)
        N.check(self.lib, self.lib.khp_debug_bsdf_eval(self.ptr, n, ip(ob), ip(mt), N.fptr(ri), N.fptr(nn), N.fptr(oo),
                                                       N.fptr(f)), "khp_debug_bsdf_eval")
        return f

    def debug_light_dir(self, light, point, draws):
        """khp_debug_light_dir on n items -> shadow ray origin, direction, attenuation."""
        li = np.ascontiguousarray(light, np.int32).reshape(-1)
        n = len(li)
        p = np.ascontiguousarray(point, np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(draws, np.float32).reshape(-1, 2)
        r = {"o": np.empty((n, 3), np.float32), "d": np.empty((n, 3), np.float32), "att": np.empty(n, np.float32)}
        N.check(self.lib, self.lib.khp_debug_light_dir(self.ptr, n, li.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                       N.fptr(p), N.fptr(u), N.fptr(r["o"]), N.fptr(r["d"]),
                                                       N.fptr(r["att"])), "khp_debug_light_dir")
        return r

    def debug_light_isect(self, light, orig, direction):
        """khp_debug_light_isect on n items -> hit, t, emitted colour."""
        li = np.ascontiguousarray(light, np.int32).reshape(-1)
        n = len(li)
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        r = {"hit": np.empty(n, np.uint8), "t": np.empty(n, np.float32), "emit": np.empty((n, 3), np.float32)}
        N.check(self.lib, self.lib.khp_debug_light_isect(self.ptr, n, li.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                         N.fptr(o), N.fptr(d),
                                                         r["hit"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                         N.fptr(r["t"]), N.fptr(r["emit"])), "khp_debug_light_isect")
        return r

    # ---- ABI 17 queries of the light-path variant (test hooks) ----
    def debug_light_paths(self, k, seed=0x4B49524B):
        """khp_debug_light_paths: the subpaths of sample index k as the renderer's own kernel
        traces them -> [light_paths, n_lights, vertices, 10] (valid, pos, din, hit colour)."""
        prm = N.BdptParams()
        N.check(self.lib, self.lib.khp_get_bdpt(self.ptr, ctypes.byref(prm)), "khp_get_bdpt")
        nl = len(self._scene.lights) if self._scene is not None else 0
        shape = (int(prm.light_paths), nl, int(prm.vertices), 10)
        out = np.zeros(max(1, int(np.prod(shape))), np.float32)
        N.check(self.lib, self.lib.khp_debug_light_paths(self.ptr, int(seed), int(k), N.fptr(out)),
                "khp_debug_light_paths")
        return out[:int(np.prod(shape))].reshape(shape)

    def debug_bdpt_connect(self, orig, direction, bounce, light, j, vertex):
        """khp_debug_bdpt_connect on n items -> hit, accepted, connection ray (o, d), tmax, cj."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        n = len(o)
        b = np.ascontiguousarray(bounce, np.uint32).reshape(-1)
        li = np.ascontiguousarray(light, np.int32).reshape(-1)
        jj = np.ascontiguousarray(j, np.uint32).reshape(-1)
        v = np.ascontiguousarray(vertex, np.float32).reshape(-1, 10)
        up = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        r = {"hit": np.empty(n, np.uint8), "accepted": np.empty(n, np.uint8), "o": np.empty((n, 3), np.float32),
             "d": np.empty((n, 3), np.float32), "tmax": np.empty(n, np.float32), "cj": np.empty((n, 3), np.float32)}
        N.check(self.lib, self.lib.khp_debug_bdpt_connect(
            self.ptr, n, N.fptr(o), N.fptr(d), up(b), li.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), up(jj),
            N.fptr(v), bp(r["hit"]), bp(r["accepted"]), N.fptr(r["o"]), N.fptr(r["d"]), N.fptr(r["tmax"]),
            N.fptr(r["cj"])), "khp_debug_bdpt_connect")
        return r

    def debug_img_connect(self, width, height, sensor, j, prev, cur):
        """khp_debug_img_connect on n items of a width x height frame -> accepted, d, t, cj."""
        s = np.ascontiguousarray(sensor, np.float32).reshape(-1, 3)
        n = len(s)
        jj = np.ascontiguousarray(j, np.uint32).reshape(-1)
        pv = np.ascontiguousarray(prev, np.float32).reshape(-1, 10)
        cv = np.ascontiguousarray(cur, np.float32).reshape(-1, 10)
        r = {"accepted": np.empty(n, np.uint8), "d": np.empty((n, 3), np.float32), "t": np.empty(n, np.float32),
             "cj": np.empty((n, 3), np.float32)}
        N.check(self.lib, self.lib.khp_debug_img_connect(
            self.ptr, int(width), int(height), n, N.fptr(s), jj.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            N.fptr(pv), N.fptr(cv), r["accepted"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), N.fptr(r["d"]),
            N.fptr(r["t"]), N.fptr(r["cj"])), "khp_debug_img_connect")
        return r

    # ---- queries of the texture lookups (test hooks) ----
    def debug_tex_color(self, tex, xy):
        """khp_debug_tex_color on n (texture, x, y) items -> rgba (n, 4)."""
        ti = np.ascontiguousarray(tex, np.int32).reshape(-1)
        n = len(ti)
        c = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty((n, 4), np.float32)
        N.check(self.lib, self.lib.khp_debug_tex_color(self.ptr, n, ti.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                       N.fptr(c), N.fptr(out)), "khp_debug_tex_color")
        return out

    def debug_env_color(self, direction):
        """khp_debug_env_color on n directions -> rgb (n, 3)."""
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        out = np.empty((len(d), 3), np.float32)
        N.check(self.lib, self.lib.khp_debug_env_color(self.ptr, len(d), N.fptr(d), N.fptr(out)), "khp_debug_env_color")
        return out

    def debug_material(self, orig, direction):
        """khp_debug_material: closest hit, its barycentrics and texcoord, and the resolved material, per ray."""
        o = np.ascontiguousarray(orig, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
        n = len(o)
        r = {"t": np.empty(n, np.float32), "obj": np.empty(n, np.int32), "bary": np.empty((n, 2), np.float32),
             "tc": np.empty((n, 2), np.float32), "diffuse": np.empty((n, 3), np.float32),
             "specular": np.empty((n, 3), np.float32), "volume": np.empty((n, 3), np.float32),
             "emission": np.empty((n, 3), np.float32), "roughness": np.empty(n, np.float32)}
        N.check(self.lib, self.lib.khp_debug_material(
            self.ptr, n, N.fptr(o), N.fptr(d), N.fptr(r["t"]), r["obj"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            N.fptr(r["bary"]), N.fptr(r["tc"]), N.fptr(r["diffuse"]), N.fptr(r["specular"]), N.fptr(r["volume"]),
            N.fptr(r["emission"]), N.fptr(r["roughness"])), "khp_debug_material")
        return r

    def debug_queues(self):
        """The extension rays and the shadow rays (o, d, t_max) of bounce
        khp_ctx_params.dump_bounce of the last synchronous render."""
        n = ctypes.c_uint32()
        N.check(self.lib, self.lib.khp_debug_queue(self.ptr, ctypes.byref(n), None, None), "khp_debug_queue")
        o, d = np.empty((n.value, 3), np.float32), np.empty((n.value, 3), np.float32)
        N.check(self.lib, self.lib.khp_debug_queue(self.ptr, ctypes.byref(n), N.fptr(o), N.fptr(d)), "khp_debug_queue")
        m = ctypes.c_uint32()
        N.check(self.lib, self.lib.khp_debug_shadow_queue(self.ptr, ctypes.byref(m), None, None, None),
                "khp_debug_shadow_queue")
        so, sd, st = np.empty((m.value, 3), np.float32), np.empty((m.value, 3), np.float32), np.empty(m.value, np.float32)
        N.check(self.lib, self.lib.khp_debug_shadow_queue(self.ptr, ctypes.byref(m), N.fptr(so), N.fptr(sd), N.fptr(st)),
                "khp_debug_shadow_queue")
        return (o, d), (so, sd, st)

    def stats(self) -> dict:
        s = N.Stats()
        N.check(self.lib, self.lib.khp_get_stats(self.ptr, ctypes.byref(s)), "khp_get_stats")
        return s.as_dict()

    # --- multi-GPU --------------------------------------------------------------
    def comm_init(self, nranks: int, rank: int, uid: bytes, timeout_ms: int | None = None):
        """khp_comm_init; timeout_ms (khp_comm_set_timeout, ABI 11) bounds the init and
        every later wait of this context while the communicator exists."""
        if timeout_ms is not None:
            self.comm_set_timeout(timeout_ms)
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        N.check(self.lib, self.lib.khp_comm_init(self.ptr, nranks, rank, buf), "khp_comm_init")

    def comm_set_timeout(self, timeout_ms: int):
        N.check(self.lib, self.lib.khp_comm_set_timeout(self.ptr, int(timeout_ms)), "khp_comm_set_timeout")

    def gather_framebuffer(self, width, height, spp, depth, tile_size, nranks, rank, root=0):
        p = N.RenderParams(width, height, spp, depth, 0, 0, tile_size, rank, nranks, 0)
        N.check(self.lib, self.lib.khp_gather_framebuffer(self.ptr, ctypes.byref(p), root), "khp_gather_framebuffer")


def _ray_items(pixels, samples):
    """The (pixel, sample) pairs of a camera-ray query as two uint32 arrays of one length."""
    px = np.ascontiguousarray(pixels, np.uint32).reshape(-1)
    sm = np.ascontiguousarray(samples, np.uint32).reshape(-1)
    if len(sm) == 1 and len(px) > 1:
        sm = np.full(len(px), sm[0], np.uint32)
    if len(px) != len(sm):
        raise ValueError("pixels and samples must have one length")
    return px, sm


def lens_from_kirk(focal_length: float, f_stop: float, focus_distance: float) -> dict:
    """khp_lens_from_kirk: KIRK's Camera members as set_lens arguments: radius = (focal_length /
    f_stop) * 3 (m_aperture, times the factor of transformToDof's diskRand), focus KIRK."""
    lib = N.load_library()
    prm = N.Lens()
    N.check(lib, lib.khp_lens_from_kirk(float(focal_length), float(f_stop), float(focus_distance), ctypes.byref(prm)),
            "khp_lens_from_kirk")
    return prm.as_dict()


def camera_rays_host(camera: "N.Camera", width: int, pixels, samples, lens: dict | None = None,
                     seed: int = 0x4B49524B):
    """khp_camera_rays_host: the camera rays (origins, directions) khp_render traces for the
    (pixel, sample) pairs, as a plain host loop over the kernels' own function; lens: a dict of
    radius, focus_distance and focus (lens() / lens_from_kirk()), None for the pinhole."""
    lib = N.load_library()
    px, sm = _ray_items(pixels, samples)
    o, d = np.empty((len(px), 3), np.float32), np.empty((len(px), 3), np.float32)
    prm = None
    if lens is not None:
        prm = ctypes.byref(N.Lens(float(lens["radius"]), float(lens.get("focus_distance", 11.0)),
                                  int(lens.get("focus", N.LENS_FOCUS_KIRK)), 0))
    N.check(lib, lib.khp_camera_rays_host(ctypes.byref(camera), prm, int(width), int(seed), len(px), N.uptr(px),
                                          N.uptr(sm), N.fptr(o), N.fptr(d)), "khp_camera_rays_host")
    return o, d


def _hair_items(materials, n):
    mats = list(materials) if not isinstance(materials, N.Material) else [materials]
    if len(mats) == 1 and n > 1:
        mats = mats * n
    if len(mats) != n:
        raise ValueError("one material, or one per item, is needed")
    return (N.Material * n)(*mats)


def hair_eval_host(materials, uvw, normal, wo, wi):
    """khp_hair_eval_host: f(w_o, w_i) of ChiangHairBSDF materials (one, or one per item) in the hair
    frames uvw (n, 3, 3), as a plain host loop over the kernels' own function -> f (n, 3)."""
    lib = N.load_library()
    fr = np.ascontiguousarray(uvw, np.float32).reshape(-1, 9)
    n = len(fr)
    nn, o, i = (np.ascontiguousarray(a, np.float32).reshape(n, 3) for a in (normal, wo, wi))
    f = np.empty((n, 3), np.float32)
    N.check(lib, lib.khp_hair_eval_host(n, _hair_items(materials, n), N.fptr(fr), N.fptr(nn), N.fptr(o), N.fptr(i),
                                        N.fptr(f)), "khp_hair_eval_host")
    return f


def hair_sample_host(materials, uvw, normal, wo, draws):
    """khp_hair_sample_host: one sample per item from the draws (n, 4) = u_l, u_n, u_0, u_1 -> a dict of
    out (n, 3), pdf (n), f (n, 3) and valid (n)."""
    lib = N.load_library()
    fr = np.ascontiguousarray(uvw, np.float32).reshape(-1, 9)
    n = len(fr)
    nn, o = (np.ascontiguousarray(a, np.float32).reshape(n, 3) for a in (normal, wo))
    u = np.ascontiguousarray(draws, np.float32).reshape(n, 4)
    r = {"out": np.empty((n, 3), np.float32), "pdf": np.empty(n, np.float32), "f": np.empty((n, 3), np.float32),
         "valid": np.empty(n, np.int32)}
    N.check(lib, lib.khp_hair_sample_host(n, _hair_items(materials, n), N.fptr(fr), N.fptr(nn), N.fptr(o), N.fptr(u),
                                          N.fptr(r["out"]), N.fptr(r["pdf"]), N.fptr(r["f"]),
                                          r["valid"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
            "khp_hair_sample_host")
    return r


def _u64ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _kmath_op(op) -> int:
    return N.KMATH_OP[op] if isinstance(op, str) else int(op)


def _kmath_items(items):
    w = np.ascontiguousarray(items, np.uint64)
    if w.ndim != 2 or w.shape[1] != 3:
        raise ValueError("items must have the shape (n, 3)")
    return w, np.empty_like(w)


def kmath_host(op, items) -> np.ndarray:
    """khp_kmath_host: one op of csrc/kmath_ops.h (a name of native.KMATH_OPS or its number) over items
    (n, 3) of raw uint64 words, as the host compiler builds kmath.h (no device, no context); returns the
    (n, 3) output words.  Nothing is converted: a float32 argument is the low half of its word."""
    w, o = _kmath_items(items)
    lib = N.load_library()
    N.check(lib, lib.khp_kmath_host(_kmath_op(op), len(w), _u64ptr(w), _u64ptr(o)), "khp_kmath_host")
    return o


def _env_light_arg(rgb, scale=1.0, rotation=0.0, nee=True, select=0.5):
    """A khp_env_light over a host map (height, width, 3), and the array it points into."""
    a = np.ascontiguousarray(rgb, np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("rgb must have the shape (height, width, 3)")
    prm = N.EnvLight(a.shape[1], a.shape[0], 0, int(bool(nee)), float(scale), float(rotation), float(select), 0,
                     a.ctypes.data)
    return prm, a


def _env_tables(width, height):
    return {"weight": np.empty((height, width), np.uint32), "row_cdf": np.empty((height, width + 1), np.uint32),
            "marginal": np.empty(height + 1, np.uint64)}


def env_light_tables_host(rgb, **params) -> dict:
    """khp_env_light_tables_host: the sampling table of the map rgb (height, width, 3) as plain host loops
    -> a dict of weight (H, W) uint32, row_cdf (H, W + 1) uint32 and marginal (H + 1) uint64."""
    lib = N.load_library()
    prm, a = _env_light_arg(rgb, **params)
    t = _env_tables(a.shape[1], a.shape[0])
    N.check(lib, lib.khp_env_light_tables_host(ctypes.byref(prm), N.uptr(t["weight"]), N.uptr(t["row_cdf"]),
                                               _u64ptr(t["marginal"])), "khp_env_light_tables_host")
    return t


def env_light_sample_host(rgb, draws, **params) -> dict:
    """khp_env_light_sample_host: one direction per item from the draws (n, 2), as a plain host loop over
    the kernels' own function -> a dict of dir (n, 3), pdf (n), radiance (n, 3) and valid (n)."""
    lib = N.load_library()
    prm, _a = _env_light_arg(rgb, **params)
    u = np.ascontiguousarray(draws, np.float32).reshape(-1, 2)
    n = len(u)
    r = {"dir": np.empty((n, 3), np.float32), "pdf": np.empty(n, np.float32),
         "radiance": np.empty((n, 3), np.float32), "valid": np.empty(n, np.int32)}
    N.check(lib, lib.khp_env_light_sample_host(ctypes.byref(prm), n, N.fptr(u), N.fptr(r["dir"]), N.fptr(r["pdf"]),
                                               N.fptr(r["radiance"]),
                                               r["valid"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
            "khp_env_light_sample_host")
    return r


def env_light_eval_host(rgb, dir, **params) -> dict:
    """khp_env_light_eval_host: the map's radiance and the sampler's density in the directions dir (n, 3),
    any length -> a dict of radiance (n, 3) and pdf (n)."""
    lib = N.load_library()
    prm, _a = _env_light_arg(rgb, **params)
    d = np.ascontiguousarray(dir, np.float32).reshape(-1, 3)
    n = len(d)
    r = {"radiance": np.empty((n, 3), np.float32), "pdf": np.empty(n, np.float32)}
    N.check(lib, lib.khp_env_light_eval_host(ctypes.byref(prm), n, N.fptr(d), N.fptr(r["radiance"]), N.fptr(r["pdf"])),
            "khp_env_light_eval_host")
    return r


def _frame_check(name, a, width, height):
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != (height, width, 3) or \
            not a.flags.c_contiguous:
        raise ValueError(f"{name}: a C-contiguous float32 array of shape {(height, width, 3)} is needed")


def _denoise_args(width, height, guides, device, params):
    """khp_denoise_params and khp_aov_buffers of a denoise call, the planes checked first (dtype,
    shape, or DeviceBuffer size) as render_aov checks its arrays."""
    params = dict(params)
    flags = int(params.pop("flags", 0)) | (N.DENOISE_DEMODULATE if params.pop("demodulate", False) else 0) | \
        (N.DENOISE_DEVICE if device else 0)
    for k in params:
        if k not in dict(N.DenoiseParams._fields_) or k in ("reserved", "width", "height"):
            raise ValueError(f"khp_denoise_params has no field {k!r} to set")
    buf, keep = N.AovBuffers(), []
    for ch, a in guides.items():
        if ch == "light_ended":     # the restatement's bookkeeping, not a plane
            continue
        if ch not in N.AOV_CHANNELS:
            raise ValueError(f"guides: no channel {ch!r} (one of {', '.join(N.AOV_CHANNELS)})")
        if a is None or ch == "object":   # the object plane is ignored by the filter
            continue
        tail, dtype = N.AOV_CHANNELS[ch]
        if device:
            need = int(np.prod((height, width) + tail)) * 4
            if not isinstance(a, DeviceBuffer) or a.nbytes < need:
                raise ValueError(f"channel {ch}: a DeviceBuffer of {need} bytes is needed with device=True")
            ptr = a.ptr
        else:
            if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != (height, width) + tail or \
                    not a.flags.c_contiguous:
                raise ValueError(f"channel {ch}: a C-contiguous {np.dtype(dtype).name} array of shape "
                                 f"{(height, width) + tail} is needed")
            ptr = a.ctypes.data
        setattr(buf, ch, ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)))
        keep.append(a)
    p = N.DenoiseParams.defaults(width=width, height=height, flags=flags, **params)
    return p, buf, keep


def denoise_host(width, height, guides: dict, colour: np.ndarray, out: np.ndarray | None = None, **params) -> np.ndarray:
    """khp_denoise_host: HipContext.denoise's filter as a plain host loop over the same per-pixel
    functions -- no device, no context, the same bits.  numpy arrays only; returns out."""
    p, buf, keep = _denoise_args(width, height, guides, False, params)
    _frame_check("colour", colour, width, height)
    if out is None:
        out = np.zeros((height, width, 3), np.float32)
    _frame_check("out", out, width, height)
    lib = N.load_library()
    N.check(lib, lib.khp_denoise_host(ctypes.byref(p), colour.ctypes.data_as(ctypes.c_void_p), ctypes.byref(buf),
                                      out.ctypes.data_as(ctypes.c_void_p)), "khp_denoise_host")
    del keep
    return out


def _noise_args(ctx, width, height, variance, moments, out_variance, device, params, has_context):
    """khp_denoise_noise of a denoise_var call, its planes checked first (dtype, shape, or DeviceBuffer
    size) as _denoise_args checks the guides; `prefilter` and `floor` are taken out of `params`.
    Returns (the struct, the out_variance array or None, keep-alives)."""
    kw = {k: params.pop(k) for k in ("prefilter", "floor") if k in params}
    if variance is not None and moments is not None:
        raise ValueError("variance= and moments= are two sources of the noise: give one")
    z, keep = N.DenoiseNoise.defaults(**kw), []

    def plane(name, a, tail, dtype):
        shape = (height, width) + tail
        if device:
            need = int(np.prod(shape)) * 4
            if not isinstance(a, DeviceBuffer) or a.nbytes < need:
                raise ValueError(f"{name}: a DeviceBuffer of {need} bytes is needed with device=True")
            ptr = a.ptr
        else:
            if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError(f"{name}: a C-contiguous {np.dtype(dtype).name} array of shape {shape} is needed")
            ptr = a.ctypes.data
        keep.append(a)
        return ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float if dtype == np.float32 else ctypes.c_uint32))

    if variance is not None:
        z.source = N.NOISE_PLANE
        z.variance = plane("variance", variance, (), np.float32)
    elif moments is not None:
        z.source = N.NOISE_MOMENTS
        z.m2 = plane("moments['m2']", moments["m2"], (3,), np.float32)
        z.count = plane("moments['count']", moments["count"], (), np.uint32)
    elif has_context:
        z.source = N.NOISE_CONTEXT
    else:
        raise ValueError("variance= or moments= is needed: there is no context whose moments to read")
    ov = None
    if out_variance is not None and out_variance is not False:
        if out_variance is True:
            ov = DeviceBuffer(ctx, 4 * width * height) if device else np.zeros((height, width), np.float32)
        else:
            ov = out_variance
        z.out_variance = plane("out_variance", ov, (), np.float32)
    return z, ov, keep


def denoise_var_host(width, height, guides: dict, colour: np.ndarray, variance=None, moments=None,
                     out: np.ndarray | None = None, out_variance=False, **params):
    """khp_denoise_var_host: HipContext.denoise_var's filter as a plain host loop over the same
    per-pixel functions -- no device, no context, the same bits.  numpy arrays only, and the noise is
    `variance` or `moments`.  Returns out, or (out, out_variance) when that was asked for."""
    params = dict(params)
    z, ov, keep_z = _noise_args(None, width, height, variance, moments, out_variance, False, params, False)
    p, buf, keep = _denoise_args(width, height, guides, False, params)
    _frame_check("colour", colour, width, height)
    if out is None:
        out = np.zeros((height, width, 3), np.float32)
    _frame_check("out", out, width, height)
    lib = N.load_library()
    N.check(lib, lib.khp_denoise_var_host(ctypes.byref(p), colour.ctypes.data_as(ctypes.c_void_p), ctypes.byref(buf),
                                          ctypes.byref(z), out.ctypes.data_as(ctypes.c_void_p)), "khp_denoise_var_host")
    del keep, keep_z
    return out if ov is None else (out, ov)


REPROJECT_OUTPUTS = {"colour": (3,), "length": (), "variance": (), "motion": (2,)}   # khp_reproject_out, in struct order


def _reproject_args(ctx, width, height, cur, hist, out, device, params):
    """khp_reproject_params, the two khp_reproject_frame and khp_reproject_out of a reproject call, every
    array checked first (dtype, shape, or DeviceBuffer size) as _denoise_args checks the guides.
    Returns (params, cur frame, hist frame or None, out struct, the outputs as a dict, keep-alives)."""
    params = dict(params)
    flags = int(params.pop("flags", 0)) | (N.REPROJECT_MATCH_OBJECT if params.pop("match_object", False) else 0) | \
        (N.REPROJECT_DEVICE if device else 0)
    for k in params:
        if k not in dict(N.ReprojectParams._fields_) or k in ("reserved", "width", "height"):
            raise ValueError(f"khp_reproject_params has no field {k!r} to set")
    keep = []

    def plane(name, a, tail, dtype=np.float32):
        shape = (height, width) + tail
        if device:
            need = int(np.prod(shape)) * 4
            if not isinstance(a, DeviceBuffer) or a.nbytes < need:
                raise ValueError(f"{name}: a DeviceBuffer of {need} bytes is needed with device=True")
            ptr = a.ptr
        else:
            if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError(f"{name}: a C-contiguous {np.dtype(dtype).name} array of shape {shape} is needed")
            ptr = a.ctypes.data
        keep.append(a)
        return ctypes.cast(ptr, ctypes.POINTER(ctypes.c_int32 if dtype == np.int32 else ctypes.c_float))

    def frame(which, f):
        for k in f:
            if k not in ("camera", "colour", "variance", "length", "aov", "motion"):
                raise ValueError(f"{which}: a frame has no entry {k!r}")
        if not isinstance(f.get("camera"), N.Camera):
            raise ValueError(f"{which}['camera']: an N.Camera is needed (scenes.camera makes one)")
        s = N.ReprojectFrame(camera=f["camera"])
        if f.get("colour") is None:
            raise ValueError(f"{which}['colour'] is needed")
        s.colour = plane(f"{which}['colour']", f["colour"], (3,))
        for k in ("variance", "length"):
            if f.get(k) is not None:
                setattr(s, k, plane(f"{which}[{k!r}]", f[k], ()))
        for ch, a in (f.get("aov") or {}).items():
            if ch == "light_ended":     # the restatement's bookkeeping, not a plane
                continue
            if ch not in N.AOV_CHANNELS:
                raise ValueError(f"{which}['aov']: no channel {ch!r} (one of {', '.join(N.AOV_CHANNELS)})")
            if a is None or ch == "albedo":   # the albedo plane is never read
                continue
            tail, dtype = N.AOV_CHANNELS[ch]
            setattr(s.aov, ch, plane(f"{which}['aov'][{ch!r}]", a, tail, dtype))
        return s

    cf = frame("cur", cur)
    hf = frame("hist", hist) if hist is not None else None
    o, res = N.ReprojectOut(), {}
    for name, tail in REPROJECT_OUTPUTS.items():
        if out is not None and name in out:
            a = out[name]
            if a is None:
                continue
        elif device:
            a = DeviceBuffer(ctx, int(np.prod((height, width) + tail)) * 4)
        else:
            a = np.zeros((height, width) + tail, np.float32)
        setattr(o, name, plane(f"out[{name!r}]", a, tail))
        res[name] = a
    if out is not None:
        for k in out:
            if k not in REPROJECT_OUTPUTS:
                raise ValueError(f"out: no output {k!r} (one of {', '.join(REPROJECT_OUTPUTS)})")
    p = N.ReprojectParams.defaults(width=width, height=height, flags=flags, **params)
    return p, cf, hf, o, res, keep


def reproject_host(width, height, cur: dict, hist: dict | None = None, out: dict | None = None, **params) -> dict:
    """khp_reproject_host: HipContext.reproject as a plain host loop over the same per-pixel function --
    no device, no context, the same bits.  numpy arrays only; returns the dict of outputs."""
    p, cf, hf, o, res, keep = _reproject_args(None, width, height, cur, hist, out, False, params)
    lib = N.load_library()
    N.check(lib, lib.khp_reproject_host(ctypes.byref(p), ctypes.byref(cf), ctypes.byref(hf) if hf is not None else None,
                                        ctypes.byref(o)), "khp_reproject_host")
    del keep
    return res


class TemporalAccumulator:
    """The ping-pong a viewer does around khp_reproject: it owns the history -- the blended
    colour, its length and variance, and the camera and AOV planes they belong to -- and each push()
    blends a new frame into it.  With a context the frames are DeviceBuffers of that context and the
    kernel runs; without one they are numpy arrays and the host entry runs.  The same bits either way.

        acc = TemporalAccumulator(w, h, ctx)           # **params: khp_reproject_params fields
        shown = acc.push(cam, aov, colour)["colour"]   # every frame, moved camera or not
        acc.reset()                                    # after set_scene: the history is of another scene
                                                       # (after update_geometry too: reset(), or keep it
                                                       #  and let the object / depth tests reject what moved;
                                                       #  either way render the next frame from first_sample = 0)

    The outputs alternate between two sets of buffers: what push() returns stays as it is until the
    push after the next.  The aov planes (and nothing else) are kept by reference as the next history's:
    hand over planes that will not be written to before the next push."""

    def __init__(self, width: int, height: int, ctx: "HipContext | None" = None, **params):
        self.width, self.height, self.ctx, self.params = int(width), int(height), ctx, dict(params)
        for k in params:
            if k not in dict(N.ReprojectParams._fields_) and k != "match_object" or k in ("reserved", "width", "height", "samples"):
                raise ValueError(f"khp_reproject_params has no field {k!r} to set here (samples goes to push())")
        self._sets, self._turn, self._hist = [None, None], 0, None

    def reset(self):
        """Drop the history: the next push() starts one.  HipContext.update_geometry does not do this, nor
        restart the context's running mean, sample counts and moments: render with first_sample = 0."""
        self._hist = None

    @property
    def history(self) -> "dict | None":
        """The frame the next push() blends into (camera, colour, length, variance, aov), or None."""
        return self._hist

    def _outputs(self):
        if self._sets[self._turn] is None:
            shape = lambda tail: (self.height, self.width) + tail
            if self.ctx is not None:
                make = lambda tail: DeviceBuffer(self.ctx, int(np.prod(shape(tail))) * 4)
            else:
                make = lambda tail: np.zeros(shape(tail), np.float32)
            self._sets[self._turn] = {name: make(tail) for name, tail in REPROJECT_OUTPUTS.items()}
        return self._sets[self._turn]

    def push(self, camera: "N.Camera", aov: dict, colour, variance=None, samples: float = 1.0) -> dict:
        """Blend the frame (camera, aov, colour, variance) of weight `samples` (its samples per pixel) into
        the history and keep the result as the next history.  Returns the dict of khp_reproject's outputs:
        "colour" (the frame to show, or to hand to denoise_var with "variance"), "length", "variance", "motion"."""
        cur = {"camera": camera, "colour": colour, "variance": variance, "aov": aov}
        out = self._outputs()
        kw = dict(self.params, samples=samples)
        if self.ctx is not None:
            res = self.ctx.reproject(self.width, self.height, cur, self._hist, out=out, device=True, **kw)
        else:
            res = reproject_host(self.width, self.height, cur, self._hist, out=out, **kw)
        self._turn ^= 1
        self._hist = {"camera": camera, "colour": res["colour"], "length": res["length"], "variance": res["variance"],
                      "aov": {ch: a for ch, a in aov.items() if ch in N.AOV_CHANNELS and ch != "albedo"}}
        return res


def moments_fold_host(samples: np.ndarray, first_sample: int = 0, state: dict | None = None) -> dict:
    """khp_moments_fold_host: the fold of HipContext's sample moments as a plain host loop over the
    same functions the kernels compile -- no device, no context, the same bits.  `samples` is
    (K, ..., 3) float32, sample s having global index first_sample + s; `state` is a dict of mean,
    m2, count and bad to continue from (left as it is), or None for a zeroed one.  Returns the new
    state with rel_error, the planes shaped like one sample."""
    s = np.ascontiguousarray(samples, np.float32)
    if s.ndim < 2 or s.shape[-1] != 3:
        raise ValueError("samples: a float32 array of shape (K, ..., 3) is needed")
    shape = s.shape[1:-1]
    n_pix = int(np.prod(shape, dtype=np.int64))
    res, buf = {}, N.MomentsBuffers()
    for ch, (tail, dtype) in N.MOMENTS_PLANES.items():
        if state is not None and ch != "rel_error":
            a = np.array(state[ch], dtype, order="C")
            if a.shape != shape + tail:
                raise ValueError(f"state[{ch!r}]: shape {shape + tail} is needed")
        else:
            a = np.zeros(shape + tail, dtype)
        setattr(buf, ch, ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_float if dtype == np.float32 else ctypes.c_uint32)))
        res[ch] = a
    lib = N.load_library()
    N.check(lib, lib.khp_moments_fold_host(n_pix, int(first_sample), s.shape[0], s.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(buf)), "khp_moments_fold_host")
    return res


def _adaptive_params(threshold=None, min_samples=None, max_samples=None) -> "N.AdaptiveParams":
    given = {"threshold": threshold, "min_samples": min_samples, "max_samples": max_samples}
    return N.AdaptiveParams.defaults(**{k: v for k, v in given.items() if v is not None})


def _select_args(state: dict, owned):
    """(khp_moments_buffers over the state's planes flattened by pixel, the owned list, the pixel count, keep-alives)."""
    buf, keep = N.MomentsBuffers(), []
    n_pix = int(np.asarray(state["count"]).size)
    for ch, (tail, dtype) in N.MOMENTS_PLANES.items():
        if ch == "rel_error":
            continue
        a = np.ascontiguousarray(state[ch], dtype).reshape((n_pix,) + tail)
        setattr(buf, ch, ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_float if dtype == np.float32 else ctypes.c_uint32)))
        keep.append(a)
    own = np.ascontiguousarray(owned, np.uint32).reshape(-1)
    if own.size and int(own.max()) >= n_pix:
        raise ValueError(f"owned: a pixel index is not below the state's {n_pix} pixels")
    keep.append(own)
    return buf, own, n_pix, keep


def adaptive_select_host(state: dict, owned, first_sample: int, **params) -> np.ndarray:
    """khp_adaptive_select_host: the pixels of `owned` an adaptive pass starting at first_sample
    traces, in owned order, as a plain host loop over the rule the selection kernel compiles -- no
    device, no context.  `state`: mean, m2, count and bad by image pixel (read_moments or
    moments_fold_host).  **params: threshold, min_samples, max_samples over khp_adaptive_defaults."""
    a = _adaptive_params(**params)
    buf, own, _n_pix, keep = _select_args(state, owned)
    act = np.empty(max(1, own.size), np.uint32)
    n = ctypes.c_uint32()
    lib = N.load_library()
    N.check(lib, lib.khp_adaptive_select_host(ctypes.byref(a), int(first_sample), ctypes.byref(buf), own.size,
                                              N.uptr(own), N.uptr(act), ctypes.byref(n)), "khp_adaptive_select_host")
    del keep
    return act[:n.value].copy()


def moments_variance(state: dict) -> np.ndarray:
    """The unbiased sample variance m2 / (n - 1) per channel of a moments state (read_moments or
    moments_fold_host), NaN where n < 2.  numpy, a convenience only."""
    n = np.asarray(state["count"]).astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n >= 2, np.asarray(state["m2"], np.float64) / (n - 1), np.nan).astype(np.float32)


def comm_init_local(ctxs) -> None:
    """khp_comm_init_local: contexts of this process as the ranks of one gather group
    (rank = position), the framebuffer gather moving over device copies, not RCCL."""
    lib = N.load_library()
    arr = (ctypes.c_void_p * len(ctxs))(*[c.ptr.value for c in ctxs])
    N.check(lib, lib.khp_comm_init_local(arr, len(ctxs)), "khp_comm_init_local")


def comm_unique_id() -> bytes:
    lib = N.load_library()
    buf = (ctypes.c_uint8 * 128)()
    N.check(lib, lib.khp_comm_unique_id(buf), "khp_comm_unique_id")
    return bytes(buf)


class BVH:
    """CPU_DataStructure-shaped batched queries on the GPU BVH."""

    def __init__(self, ctx: HipContext):
        self.ctx = ctx

    def closest_intersection(self, orig, direction):
        return self.ctx.trace_closest(orig, direction)

    def is_intersection(self, orig, direction, tmax):
        return self.ctx.trace_any(orig, direction, tmax)


class PathTracer:
    """KIRK::CPU::PathTracer on the HIP core (progressive, seeded)."""

    def __init__(self, scene: SceneData | None = None, depth: int = 8, device: int = 0, width: int = 256,
                 height: int = 256, seed: int = 0x4B49524B):
        self.ctx = HipContext(device)
        self.m_depth = depth                # CPU_Raytracer.h:73-75 default 8
        self.m_samples_per_pixel = 1        # PathTracer() default
        self.c_sample = 0
        self.width, self.height = width, height
        self.seed = seed
        self.m_use_tonemapping = False      # CPU_PathTracer.h:152
        self.m_tonemapper = N.Tonemap.defaults()  # CPU_PathTracer.h:38, Tonemapping.h:23-33
        if scene is not None:
            self.init(scene)

    def init(self, scene: SceneData):
        self.ctx.set_scene(scene)
        self.ctx.build_accel()
        self.reset()

    def set_depth(self, depth: int):
        self.m_depth = int(depth)

    def set_sample_count(self, samples: int):
        self.m_samples_per_pixel = int(samples)

    def get_current_sample_count(self) -> int:
        return self.c_sample

    def reset(self):
        self.c_sample = 0

    def render(self, n: int = 1):
        """Add up to `n` samples (KIRK's render() adds one sample per full pass)."""
        n = min(n, self.m_samples_per_pixel - self.c_sample)
        if n <= 0:
            return
        self.ctx.render(self.width, self.height, n, self.m_depth, self.seed, first_sample=self.c_sample,
                        readback=False)
        self.c_sample += n

    def render_to_texture(self) -> np.ndarray:
        """Render every remaining sample; returns the float RGB framebuffer (H, W, 3), row 0 = bottom."""
        self.render(self.m_samples_per_pixel - self.c_sample)
        return self.ctx.read_framebuffer(self.width, self.height)

    def texture_rgba8(self) -> np.ndarray:
        """The 8-bit render texture after the current samples, on the device:
        drawTexture's setPixel, or applyToneMapping when m_use_tonemapping
        (CPU_PathTracer.cpp:43-47, 61-104).  (H, W, 4) uint8, row 0 = bottom."""
        tm = self.m_tonemapper if self.m_use_tonemapping else None
        return self.ctx.read_rgba8(self.width, self.height, tm)

    @staticmethod
    def to_rgba8(fb: np.ndarray) -> np.ndarray:
        """Texture::setPixel's 8-bit clamp (Texture.cpp:222-241), top row first."""
        rgb = np.clip(fb, 0.0, 1.0) * 255.0
        rgba = np.concatenate([rgb, np.full(fb.shape[:2] + (1,), 255.0, np.float32)], axis=-1)
        return rgba.astype(np.uint8)[::-1]
