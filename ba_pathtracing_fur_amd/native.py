"""ctypes view of the C-ABI in include/kirk_hip.h.

The product path is libkirk_hip.so (HIP kernels for gfx950).  There is no CPU
fallback: if the library is missing or no GPU is present, the calls fail
loudly (RuntimeError), they never route anywhere else.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_uint8, c_uint32, c_uint64, c_double, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libkirk_hip.so")

# enums (kirk_hip.h)
KHP_OK, KHP_EINVAL, KHP_ENOMEM, KHP_EDEVICE, KHP_ENOTREADY, KHP_EUNSUPPORTED = range(6)
STATUS_NAMES = {0: "KHP_OK", 1: "KHP_EINVAL", 2: "KHP_ENOMEM", 3: "KHP_EDEVICE", 4: "KHP_ENOTREADY",
                5: "KHP_EUNSUPPORTED"}

BSDF_NAMES = ["LambertianReflectionBSDF", "SpecularReflectionBSDF", "SpecularTransmissionBSDF", "GlossyBSDF",
              "GlassBSDF", "MilkGlassBSDF", "LambertianTransmissionBSDF", "EmissionBSDF", "TransparentBSDF",
              "MarschnerHairBSDF", "DEonHairBSDF", "ChiangHairBSDF"]
SHADER_NAMES = ["SimpleShader", "MarschnerHairShader"]
LIGHT_POINT, LIGHT_QUAD, LIGHT_SPOT, LIGHT_SUN = 0, 1, 2, 3

RENDER_OUT_DEVICE = 1 << 0
RENDER_NO_READBACK = 1 << 1
RENDER_STATS = 1 << 2
RENDER_ASYNC = 1 << 3
CTX_STATS = 1 << 0
CTX_HOST_BUILD = 1 << 1

F3 = c_float * 3


class Material(ctypes.Structure):
    _fields_ = [("bsdf", c_int32), ("shader", c_int32), ("diffuse", F3), ("specular", F3), ("volume", F3),
                ("emission", F3), ("ior", c_float), ("roughness", c_float)]


class Light(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("color", F3), ("position", F3), ("direction", F3), ("size", c_float * 2),
                ("radius", c_float), ("att_const", c_float), ("att_lin", c_float), ("att_quad", c_float),
                ("inner_angle", c_float), ("outer_angle", c_float)]


class Environment(ctypes.Structure):
    _fields_ = [("color", F3), ("ambient", F3)]


class Camera(ctypes.Structure):
    _fields_ = [("position", F3), ("bottom_left", F3), ("axis_x", F3), ("axis_y", F3), ("pixel_size", c_float)]


TEX_WRAP_CLAMP, TEX_WRAP_TILE = 0, 1
ENV_COLOR, ENV_CUBE_MAP, ENV_SPHERE_MAP = 0, 1, 2


class Texture(ctypes.Structure):
    """khp_texture (ABI 6): KIRK::Texture's 8-bit texels."""
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("channels", c_uint32), ("wrap_mode", c_uint32),
                ("data", POINTER(c_uint8))]


class MaterialTextures(ctypes.Structure):
    """khp_material_textures (ABI 6): texture index per parameter, -1 = the material value."""
    _fields_ = [("diffuse", c_int32), ("specular", c_int32), ("volume", c_int32), ("emission", c_int32),
                ("roughness", c_int32)]


class EnvMap(ctypes.Structure):
    """khp_env_map (ABI 6): Environment::m_type and its textures."""
    _fields_ = [("type", c_int32), ("tex", c_int32 * 6)]


class SceneDesc(ctypes.Structure):
    _fields_ = [("n_tris", c_uint32), ("tri_v", POINTER(c_float)), ("tri_n", POINTER(c_float)),
                ("tri_mat", POINTER(c_uint32)), ("n_cones", c_uint32), ("cone_base_r0", POINTER(c_float)),
                ("cone_apex_r1", POINTER(c_float)), ("cone_mat", POINTER(c_uint32)), ("n_materials", c_uint32),
                ("materials", POINTER(Material)), ("n_lights", c_uint32), ("lights", POINTER(Light)),
                ("env", Environment), ("camera", Camera), ("tri_frame", POINTER(c_float)),
                ("n_cone_models", c_uint32), ("cone_models", POINTER(c_float)), ("cone_model", POINTER(c_uint32)),
                ("n_textures", c_uint32), ("textures", POINTER(Texture)),
                ("material_textures", POINTER(MaterialTextures)), ("tri_uv", POINTER(c_float)), ("env_map", EnvMap)]


class RenderParams(ctypes.Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("spp", c_uint32), ("depth", c_uint32),
                ("seed", c_uint32), ("first_sample", c_uint32), ("tile_size", c_uint32), ("tile_rank", c_uint32),
                ("tile_nranks", c_uint32), ("flags", c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("n_objects", c_uint64), ("n_nodes", c_uint64), ("n_leaves", c_uint64), ("bvh_depth", c_uint32),
                ("max_leaf_size", c_uint32), ("device_bytes", c_uint64), ("build_ms", c_double),
                ("upload_ms", c_double), ("render_ms", c_double), ("extend_ms", c_double), ("shade_ms", c_double),
                ("shadow_ms", c_double), ("other_ms", c_double), ("extend_rays", c_uint64),
                ("shadow_rays", c_uint64), ("extend_launches", c_uint64), ("node_visits", c_uint64),
                ("prim_tests", c_uint64), ("shadow_node_visits", c_uint64), ("shadow_prim_tests", c_uint64),
                ("stack_spills", c_uint64), ("bounce_rays", c_uint64 * 16), ("bounce_nodes", c_uint64 * 16),
                ("bounce_prims", c_uint64 * 16), ("bounce_shadow_rays", c_uint64 * 16),
                ("bounce_shadow_nodes", c_uint64 * 16), ("bounce_shadow_prims", c_uint64 * 16),
                ("bounce_extend_ms", c_double * 16), ("bounce_shadow_ms", c_double * 16),
                ("bounce_wave_iters", c_uint64 * 16), ("bounce_lanes_busy", c_uint64 * 16),
                ("bounce_shadow_wave_iters", c_uint64 * 16), ("bounce_shadow_lanes_busy", c_uint64 * 16),
                ("step_cycles", c_uint64 * 4), ("bvh_on_device", c_uint32), ("subframes", c_uint32),
                ("flatten_ms", c_double), ("bvh_ms", c_double), ("bvh_kernel_ms", c_double), ("layout_ms", c_double),
                ("flatten_kernel_ms", c_double), ("layout_kernel_ms", c_double),
                ("extend_pruned_pops", c_uint64), ("shadow_pruned_pops", c_uint64), ("frames", c_uint64),
                ("extend_busy_ms", c_double), ("shadow_finish_ms", c_double), ("shadow_launches", c_uint64),
                ("ahead_finished", c_uint64), ("ahead_resumed", c_uint64)]

    def as_dict(self) -> dict:
        return {k: (list(getattr(self, k)) if not isinstance(getattr(self, k), (int, float)) else getattr(self, k))
                for k, _ in self._fields_}


class CtxParams(ctypes.Structure):
    """khp_ctx_params (ABI 13 layout, 64 bytes; path_order since ABI 9, wide_from since
    ABI 10, path_kernel since ABI 11, ray_sort_from and lds_nodes since ABI 12, render_ahead since
    ABI 13): scheduling knobs of a context; no value changes any result."""
    _fields_ = [("fuse_frames", c_uint32), ("frames_in_flight", c_uint32), ("chunk_paths", c_uint64),
                ("heavy_iters", c_uint32), ("dump_bounce", c_int32), ("trace_kernels", c_uint32),
                ("shade_order", c_uint32), ("serial_stages", c_uint32), ("path_order", c_uint32),
                ("wide_from", c_uint32), ("path_kernel", c_uint32), ("ray_sort_from", c_uint32),
                ("lds_nodes", c_uint32), ("render_ahead", c_uint32), ("path_from", c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class BdptParams(ctypes.Structure):
    """khp_bdpt_params (ABI 7): the light-path (bidirectional) variant, SURVEY §8(f)4."""
    _fields_ = [("enabled", c_uint32), ("light_paths", c_uint32), ("vertices", c_uint32), ("bias", c_float),
                ("bounce_bias", c_float), ("min_pdf", c_float), ("image_plane", c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


HAIR_LOBE_R, HAIR_LOBE_TT, HAIR_LOBE_TRT = 1, 2, 4


class HairLobes(ctypes.Structure):
    """khp_hair_lobes (ABI 16, 8 bytes): the enabled lobes of Marschner's fibre model."""
    _fields_ = [("lobes", c_uint32), ("reserved", c_uint32)]


LENS_FOCUS_KIRK, LENS_FOCUS_PLANE = 0, 1


class Lens(ctypes.Structure):
    """khp_lens (16 bytes): the thin-lens camera; radius 0 is the pinhole."""
    _fields_ = [("radius", c_float), ("focus_distance", c_float), ("focus", c_uint32), ("reserved", c_uint32)]

    def as_dict(self) -> dict:
        return {"radius": float(self.radius), "focus_distance": float(self.focus_distance), "focus": int(self.focus)}


ENV_LIGHT_DEVICE = 1


class EnvLight(ctypes.Structure):
    """khp_env_light (40 bytes): a latitude-longitude map of float32 radiance as a light; 0 x 0 is off."""
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("flags", c_uint32), ("nee", c_uint32), ("scale", c_float),
                ("rotation", c_float), ("select", c_float), ("reserved", c_uint32), ("rgb", c_void_p)]

    def as_dict(self) -> dict:
        return {"width": int(self.width), "height": int(self.height), "nee": bool(self.nee), "scale": float(self.scale),
                "rotation": float(self.rotation), "select": float(self.select)}


class AovBuffers(ctypes.Structure):
    """khp_aov_buffers (48 bytes): the planes khp_render_aov writes; a null plane is not computed."""
    _fields_ = [("normal", POINTER(c_float)), ("albedo", POINTER(c_float)), ("tangent", POINTER(c_float)),
                ("depth", POINTER(c_float)), ("coverage", POINTER(c_float)), ("object", POINTER(c_int32))]


# khp_aov_buffers' planes in struct order: name -> (trailing shape, dtype)
AOV_CHANNELS = {"normal": ((3,), np.float32), "albedo": ((3,), np.float32), "tangent": ((3,), np.float32),
                "depth": ((), np.float32), "coverage": ((), np.float32), "object": ((), np.int32)}


DENOISE_DEVICE = 1 << 0
DENOISE_DEMODULATE = 1 << 1


class DenoiseParams(ctypes.Structure):
    """khp_denoise_params (48 bytes): the guided a-trous filter's size, iterations, flags, sigmas and clamp."""
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("iterations", c_uint32), ("flags", c_uint32),
                ("sigma_color", c_float), ("sigma_normal", c_float), ("sigma_tangent", c_float),
                ("sigma_depth", c_float), ("sigma_coverage", c_float), ("clamp", c_float),
                ("reserved", c_uint32 * 2)]

    @classmethod
    def defaults(cls, **kw) -> "DenoiseParams":
        """khp_denoise_params_defaults (5 iterations, sigmas 4 / 0.35 / 0.35 / 0.05 / 0.25, no clamp) with fields changed."""
        p = cls()
        load_library().khp_denoise_params_defaults(ctypes.byref(p))
        for k, v in kw.items():
            if k not in dict(cls._fields_) or k == "reserved":
                raise AttributeError(f"khp_denoise_params has no field {k}")
            setattr(p, k, v)
        return p


NOISE_PLANE, NOISE_MOMENTS, NOISE_CONTEXT = 0, 1, 2


class DenoiseNoise(ctypes.Structure):
    """khp_denoise_noise (48 bytes): where khp_denoise_var takes each pixel's measured variance from,
    the prefilter, the floor and the optional filtered-variance output."""
    _fields_ = [("source", c_uint32), ("prefilter", c_uint32), ("floor", c_float), ("reserved", c_uint32),
                ("variance", POINTER(c_float)), ("m2", POINTER(c_float)), ("count", POINTER(c_uint32)),
                ("out_variance", POINTER(c_float))]

    @classmethod
    def defaults(cls, **kw) -> "DenoiseNoise":
        """khp_denoise_noise_defaults (KHP_NOISE_PLANE, the trimmed prefilter, floor 1e-6, no planes) with fields changed."""
        p = cls()
        load_library().khp_denoise_noise_defaults(ctypes.byref(p))
        for k, v in kw.items():
            if k not in dict(cls._fields_) or k == "reserved":
                raise AttributeError(f"khp_denoise_noise has no field {k}")
            setattr(p, k, v)
        return p


REPROJECT_DEVICE = 1 << 0
REPROJECT_MATCH_OBJECT = 1 << 1


class ReprojectParams(ctypes.Structure):
    """khp_reproject_params (48 bytes): the frame size, flags, the current frame's weight, the history cap and
    the four tolerances of the tap tests."""
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("flags", c_uint32), ("samples", c_float),
                ("max_history", c_float), ("depth_tol", c_float), ("normal_tol", c_float), ("tangent_tol", c_float),
                ("coverage_tol", c_float), ("reserved", c_uint32 * 3)]

    @classmethod
    def defaults(cls, **kw) -> "ReprojectParams":
        """khp_reproject_params_defaults (samples 1, max_history 32, tolerances 0.05 / off / 0.25 / 0.5: starting
        values, not a measured optimum) with fields changed."""
        p = cls()
        load_library().khp_reproject_params_defaults(ctypes.byref(p))
        for k, v in kw.items():
            if k not in dict(cls._fields_) or k == "reserved":
                raise AttributeError(f"khp_reproject_params has no field {k}")
            setattr(p, k, v)
        return p


class ReprojectFrame(ctypes.Structure):
    """khp_reproject_frame (128 bytes): a frame's camera, colour, variance or NULL, length (the history only)
    and the planes khp_render_aov wrote with that camera."""
    _fields_ = [("camera", Camera), ("reserved", c_uint32), ("colour", POINTER(c_float)), ("variance", POINTER(c_float)),
                ("length", POINTER(c_float)), ("aov", AovBuffers)]


class ReprojectOut(ctypes.Structure):
    """khp_reproject_out (32 bytes): the blended colour, the new length, the propagated variance (+inf where
    unknown) and the motion vectors (H, W, 2); a null plane is not written."""
    _fields_ = [("colour", POINTER(c_float)), ("length", POINTER(c_float)), ("variance", POINTER(c_float)),
                ("motion", POINTER(c_float))]


MOMENTS_DEVICE = 1 << 0


class Moments(ctypes.Structure):
    """khp_moments (16 bytes): the per-pixel sample moments' switch, off by default."""
    _fields_ = [("enabled", c_uint32), ("reserved", c_uint32 * 3)]


class MomentsBuffers(ctypes.Structure):
    """khp_moments_buffers (40 bytes): the planes khp_read_moments writes; a null plane is skipped."""
    _fields_ = [("mean", POINTER(c_float)), ("m2", POINTER(c_float)), ("count", POINTER(c_uint32)),
                ("bad", POINTER(c_uint32)), ("rel_error", POINTER(c_float))]


# khp_moments_buffers' planes in struct order: name -> (trailing shape, dtype)
MOMENTS_PLANES = {"mean": ((3,), np.float32), "m2": ((3,), np.float32), "count": ((), np.uint32),
                  "bad": ((), np.uint32), "rel_error": ((), np.float32)}


class AdaptiveParams(ctypes.Structure):
    """khp_adaptive_params (16 bytes): an adaptive pass's convergence bound and sample limits."""
    _fields_ = [("threshold", c_float), ("min_samples", c_uint32), ("max_samples", c_uint32), ("reserved", c_uint32)]

    @classmethod
    def defaults(cls, **kw) -> "AdaptiveParams":
        """khp_adaptive_defaults (threshold 0.05, min_samples 8, no cap) with fields changed."""
        p = cls()
        load_library().khp_adaptive_defaults(ctypes.byref(p))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(f"khp_adaptive_params has no field {k}")
            setattr(p, k, v)
        return p


class AdaptiveResult(ctypes.Structure):
    """khp_adaptive_result (32 bytes): the rank's pixel count and the pass's active pixels."""
    _fields_ = [("owned", c_uint64), ("active", c_uint64), ("reserved", c_uint64 * 2)]


class Tonemap(ctypes.Structure):
    """khp_tonemap: KIRK::Tonemapper's parameters (Utils/Tonemapping.h:22-33)."""
    _fields_ = [("exposure", c_float), ("bias", c_float), ("gamma", c_float), ("contrast", c_float),
                ("white", c_float), ("black", c_float), ("rec_gamma", c_int32), ("center_weight", c_int32),
                ("kernel_multiplier", c_float), ("center_x", c_int32), ("center_y", c_int32)]

    @classmethod
    def defaults(cls, **kw) -> "Tonemap":
        t = cls(exposure=0.0, bias=0.85, gamma=1.0, contrast=0.0, white=1.0, black=0.0, rec_gamma=0,
                center_weight=0, kernel_multiplier=0.125, center_x=-1, center_y=-1)
        for k, v in kw.items():
            if not hasattr(t, k):
                raise AttributeError(f"khp_tonemap has no field {k}")
            setattr(t, k, v)
        return t


FUR_FRAME_KIRK, FUR_FRAME_NORMAL = 0, 1


class FurParams(ctypes.Structure):
    """khp_fur_params (ABI 14, 44 bytes): Mesh::addFurToFaces' arguments and the seeded extensions."""
    _fields_ = [("fibers_per_face", c_uint32), ("density", c_float), ("verts", c_uint32), ("root_radius", c_float),
                ("scale", c_float), ("frame", c_uint32), ("comb", F3), ("seed", c_uint32), ("reserved", c_uint32)]

    @classmethod
    def defaults(cls, **kw) -> "FurParams":
        """khp_fur_params_defaults (the Demo's addFurFibersToAllMeshes(5, 10, 0.004)) with fields changed."""
        p = cls()
        load_library().khp_fur_params_defaults(ctypes.byref(p))
        for k, v in kw.items():
            if k not in dict(cls._fields_):
                raise AttributeError(f"khp_fur_params has no field {k}")
            if k == "comb":
                p.comb[:] = [float(x) for x in v]
            else:
                setattr(p, k, v)
        return p


class RefitInfo(ctypes.Structure):
    """khp_refit_info (khp_update_geometry)."""
    _fields_ = [("refit_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double), ("sah_cost", ctypes.c_double),
                ("sah_cost_built", ctypes.c_double), ("n_updates", c_uint32), ("reserved", c_uint32),
                ("root_box", c_float * 6)]

    def as_dict(self) -> dict:
        return {"refit_ms": self.refit_ms, "kernel_ms": self.kernel_ms, "sah_cost": self.sah_cost,
                "sah_cost_built": self.sah_cost_built, "n_updates": int(self.n_updates),
                "root_box": np.array(self.root_box[:], np.float32)}


class VariantFacts(ctypes.Structure):
    """khp_variant_facts: what a render kernel's compile-time instance is chosen from (flags, but bounce)."""
    _fields_ = [(k, c_uint32) for k in ("textured", "fur_only", "lobes_on", "hair", "env", "lens_on", "bd", "bounce",
                                        "cam0", "stats", "cam", "wide", "top", "has_top", "ahead", "queue_start")]


# khp_kernel_family (include/kirk_hip.h), in enum order: the kernel, and its template arguments in declaration order
KERNEL_FAMILIES = (("k_path", ("tex", "wide", "kinds", "ra", "qs", "lens", "env")),
                   ("k_shade", ("tex", "bd", "kinds", "lens", "env")),
                   ("k_extend", ("stats", "cam", "wide", "top", "lens")),
                   ("k_shadow", ("stats", "wide", "top")),
                   ("k_aov_trace", ("tex", "lens")),
                   ("k_generate", ("lens",)),
                   ("k_shadow_finish", ("bd",)))

# every symbol the header declares (checked by tests/test_abi.py)
EXPORTED = ["khp_create", "khp_destroy", "khp_last_error", "khp_abi_version", "khp_set_scene", "khp_build_accel",
            "khp_render", "khp_read_framebuffer", "khp_trace_closest", "khp_trace_any", "khp_get_stats",
            "khp_comm_unique_id", "khp_comm_init", "khp_gather_framebuffer", "khp_bsdf_kind_from_name",
            "khp_bsdf_name", "khp_shader_kind_from_name", "khp_camera_setup", "khp_fibers_to_cones",
            "khp_gen_hairball", "khp_gen_icosphere", "khp_gen_torus", "khp_host_build", "khp_debug_queue",
            "khp_read_rgba8", "khp_tonemap_defaults", "khp_read_bvh",
            "khp_read_layout", "khp_set_scene_device", "khp_gen_hairball_device", "khp_device_alloc",
            "khp_device_free", "khp_device_copy", "khp_fibers_to_triangles", "khp_gen_hairball_tris_device",
            "khp_sync", "khp_ctx_params_defaults", "khp_set_params", "khp_get_params", "khp_debug_shadow_queue",
            "khp_bdpt_params_defaults", "khp_set_bdpt", "khp_get_bdpt", "khp_gather_plan",
            "khp_read_rgba8_async", "khp_snapshot_wait", "khp_comm_init_local", "khp_comm_set_timeout",
            "khp_tonemap_log_sum", "khp_set_camera", "khp_debug_comm_wait", "khp_fur_params_defaults",
            "khp_fur_count", "khp_gen_fur", "khp_gen_fur_device", "khp_debug_surface", "khp_debug_bsdf_sample",
            "khp_debug_bsdf_eval", "khp_debug_light_dir", "khp_debug_light_isect", "khp_hair_lobes_defaults",
            "khp_set_hair_lobes", "khp_get_hair_lobes", "khp_debug_hair_sample", "khp_render_aov",
            "khp_debug_light_paths", "khp_debug_bdpt_connect", "khp_debug_img_connect", "khp_denoise_params_defaults",
            "khp_denoise", "khp_denoise_host", "khp_moments_defaults", "khp_set_moments", "khp_get_moments",
            "khp_read_moments", "khp_moments_fold_host", "khp_adaptive_defaults", "khp_render_adaptive",
            "khp_adaptive_select_host", "khp_debug_adaptive_select", "khp_debug_adaptive_list",
            "khp_denoise_noise_defaults", "khp_denoise_var", "khp_denoise_var_host",
            "khp_reproject_params_defaults", "khp_reproject", "khp_reproject_host", "khp_debug_tex_color",
            "khp_debug_env_color", "khp_debug_material", "khp_lens_defaults", "khp_lens_from_kirk", "khp_set_lens",
            "khp_get_lens", "khp_camera_rays_host", "khp_debug_camera_rays", "khp_hair_material",
            "khp_hair_eval_host", "khp_hair_sample_host", "khp_env_light_defaults", "khp_set_env_light",
            "khp_get_env_light", "khp_env_light_tables_host", "khp_env_light_sample_host", "khp_env_light_eval_host",
            "khp_debug_env_light_tables", "khp_debug_env_light", "khp_kmath_host", "khp_debug_kmath",
            "khp_update_geometry", "khp_update_geometry_device", "khp_get_refit_info", "khp_refit_host",
            "khp_kernel_variant_host", "khp_kernel_variant_table"]

# khp_kmath_op (include/kirk_hip.h): the ops of khp_kmath_host / khp_debug_kmath, in enum order
KMATH_OPS = ("mul", "add", "div", "sqrt", "rsqrt", "muladd", "floor", "f2i", "f2u", "i2f", "u2f", "u642f", "d2i2d",
             "dmul", "dadd", "ddiv", "umulhi", "ldexpf", "sinf", "cosf", "atanf", "atan2f", "asinf", "acosf", "expf",
             "sinhf", "hypotf", "logf_d", "powf_d", "j0", "log_d", "exp_d", "pow_d", "lowbias32", "path_key",
             "draw_u32", "draw_u01", "dot", "cross", "normalize", "reflect", "refract", "rotate_rowvec", "angle",
             "faceforward", "gmin", "gmax", "gclamp")
KMATH_OP = {name: i for i, name in enumerate(KMATH_OPS)}

# the include/kirk_hip.h this module mirrors (load_library refuses another)
ABI_VERSION = 17

_lib = None


def fptr(a: np.ndarray):
    return a.ctypes.data_as(POINTER(c_float))


def uptr(a: np.ndarray):
    return a.ctypes.data_as(POINTER(c_uint32))


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load libkirk_hip.so; raises RuntimeError if it was not built.

    `path`, or the KHP_LIB environment variable, selects another build of the
    same ABI (tools/build_variant.sh + tools/gpu_variants.sh A/B runs); the
    library itself reads no environment."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("KHP_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"HIP core not built: {p} missing (run __graft_entry__.build())")
    lib = ctypes.CDLL(p)
    P = POINTER
    sig = {
        "khp_create": (c_int, [P(c_void_p), c_int, c_uint32]),
        "khp_destroy": (None, [c_void_p]),
        "khp_last_error": (c_char_p, []),
        "khp_abi_version": (c_int, []),
        "khp_set_scene": (c_int, [c_void_p, P(SceneDesc)]),
        "khp_build_accel": (c_int, [c_void_p]),
        "khp_render": (c_int, [c_void_p, P(RenderParams), c_void_p]),
        "khp_render_aov": (c_int, [c_void_p, P(RenderParams), P(AovBuffers)]),
        "khp_denoise_params_defaults": (None, [P(DenoiseParams)]),
        "khp_denoise": (c_int, [c_void_p, P(DenoiseParams), c_void_p, P(AovBuffers), c_void_p]),
        "khp_denoise_host": (c_int, [P(DenoiseParams), c_void_p, P(AovBuffers), c_void_p]),
        "khp_denoise_noise_defaults": (None, [P(DenoiseNoise)]),
        "khp_denoise_var": (c_int, [c_void_p, P(DenoiseParams), c_void_p, P(AovBuffers), P(DenoiseNoise), c_void_p]),
        "khp_denoise_var_host": (c_int, [P(DenoiseParams), c_void_p, P(AovBuffers), P(DenoiseNoise), c_void_p]),
        "khp_reproject_params_defaults": (None, [P(ReprojectParams)]),
        "khp_reproject": (c_int, [c_void_p, P(ReprojectParams), P(ReprojectFrame), P(ReprojectFrame), P(ReprojectOut)]),
        "khp_reproject_host": (c_int, [P(ReprojectParams), P(ReprojectFrame), P(ReprojectFrame), P(ReprojectOut)]),
        "khp_moments_defaults": (None, [P(Moments)]),
        "khp_set_moments": (c_int, [c_void_p, P(Moments)]),
        "khp_get_moments": (c_int, [c_void_p, P(Moments)]),
        "khp_read_moments": (c_int, [c_void_p, c_uint32, P(MomentsBuffers)]),
        "khp_moments_fold_host": (c_int, [c_uint32, c_uint32, c_uint32, c_void_p, P(MomentsBuffers)]),
        "khp_adaptive_defaults": (None, [P(AdaptiveParams)]),
        "khp_render_adaptive": (c_int, [c_void_p, P(RenderParams), P(AdaptiveParams), P(AdaptiveResult), c_void_p]),
        "khp_adaptive_select_host": (c_int, [P(AdaptiveParams), c_uint32, P(MomentsBuffers), c_uint32, P(c_uint32),
                                             P(c_uint32), P(c_uint32)]),
        "khp_debug_adaptive_select": (c_int, [c_void_p, P(AdaptiveParams), c_uint32, c_uint32, P(MomentsBuffers),
                                              c_uint32, P(c_uint32), P(c_uint32), P(c_uint32)]),
        "khp_debug_adaptive_list": (c_int, [c_void_p, P(c_uint32), P(c_uint32), P(c_double)]),
        "khp_sync": (c_int, [c_void_p]),
        "khp_ctx_params_defaults": (None, [P(CtxParams)]),
        "khp_set_params": (c_int, [c_void_p, P(CtxParams)]),
        "khp_get_params": (c_int, [c_void_p, P(CtxParams)]),
        "khp_bdpt_params_defaults": (None, [P(BdptParams)]),
        "khp_set_bdpt": (c_int, [c_void_p, P(BdptParams)]),
        "khp_set_camera": (c_int, [c_void_p, P(Camera)]),
        "khp_debug_comm_wait": (c_int, [c_void_p, c_int, c_uint32, c_uint32, P(c_double)]),
        "khp_get_bdpt": (c_int, [c_void_p, P(BdptParams)]),
        "khp_read_framebuffer": (c_int, [c_void_p, P(c_float)]),
        "khp_read_rgba8": (c_int, [c_void_p, P(Tonemap), P(c_uint8)]),
        "khp_tonemap_defaults": (None, [P(Tonemap)]),
        "khp_read_rgba8_async": (c_int, [c_void_p, P(c_uint8), P(c_uint64)]),
        "khp_snapshot_wait": (c_int, [c_void_p, c_uint64, c_int]),
        "khp_set_scene_device": (c_int, [c_void_p, P(SceneDesc)]),
        "khp_gen_hairball_device": (c_int, [c_void_p, c_uint32, c_uint32, P(c_float), c_float, c_float, c_uint32,
                                            c_void_p, c_void_p]),
        "khp_fibers_to_triangles": (c_int, [c_uint32, c_uint32, P(c_float), P(c_float), c_uint32, P(c_float),
                                            P(c_float), P(c_float)]),
        "khp_gen_hairball_tris_device": (c_int, [c_void_p, c_uint32, c_uint32, P(c_float), c_float, c_float,
                                                 c_uint32, c_uint32, c_void_p, c_void_p, c_void_p]),
        "khp_device_alloc": (c_int, [c_void_p, ctypes.c_size_t, P(c_void_p)]),
        "khp_device_free": (c_int, [c_void_p, c_void_p]),
        "khp_device_copy": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_int]),
        "khp_read_layout": (c_int, [c_void_p, P(c_uint32), P(c_uint32), c_void_p, P(c_float), P(c_uint32)]),
        "khp_read_bvh": (c_int, [c_void_p, P(c_uint32), P(c_uint32), P(c_float), P(c_int32), P(c_int32), P(c_int32)]),
        "khp_trace_closest": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float), P(c_float), P(c_int32),
                                      P(c_float)]),
        "khp_trace_any": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float), P(c_float), P(c_uint8)]),
        "khp_get_stats": (c_int, [c_void_p, P(Stats)]),
        "khp_comm_unique_id": (c_int, [P(c_uint8)]),
        "khp_comm_init": (c_int, [c_void_p, c_int, c_int, P(c_uint8)]),
        "khp_comm_set_timeout": (c_int, [c_void_p, c_uint32]),
        "khp_tonemap_log_sum": (c_int, [P(ctypes.c_double), ctypes.c_uint64, c_float, P(c_float)]),
        "khp_gather_framebuffer": (c_int, [c_void_p, P(RenderParams), c_int]),
        "khp_comm_init_local": (c_int, [P(c_void_p), c_int]),
        "khp_gather_plan": (c_int, [c_uint32, c_uint32, c_uint32, c_int, c_int, c_int, P(c_uint64), P(c_uint32),
                                    P(c_uint64)]),
        "khp_bsdf_kind_from_name": (c_int, [c_char_p]),
        "khp_bsdf_name": (c_char_p, [c_int]),
        "khp_shader_kind_from_name": (c_int, [c_char_p]),
        "khp_camera_setup": (c_int, [P(c_float), P(c_float), P(c_float), c_float, c_float, c_float, c_uint32,
                                     c_uint32, P(Camera)]),
        "khp_fibers_to_cones": (c_int, [c_uint32, c_uint32, P(c_float), P(c_float), P(c_float), P(c_float)]),
        "khp_gen_hairball": (c_int, [c_uint32, c_uint32, P(c_float), c_float, c_float, c_uint32, P(c_float),
                                     P(c_float)]),
        "khp_fur_params_defaults": (None, [P(FurParams)]),
        "khp_fur_count": (c_int, [P(FurParams), c_uint32, P(c_float), P(c_uint64), P(c_uint32)]),
        "khp_gen_fur": (c_int, [P(FurParams), c_uint32, P(c_float), P(c_float), P(c_float), P(c_float)]),
        "khp_gen_fur_device": (c_int, [c_void_p, P(FurParams), c_uint32, c_void_p, c_void_p, c_uint64, c_void_p,
                                       c_void_p, P(c_uint64)]),
        "khp_gen_icosphere": (c_int, [c_uint32, P(c_float), c_float, P(c_float), P(c_float)]),
        "khp_gen_torus": (c_int, [c_uint32, c_uint32, P(c_float), c_float, c_float, P(c_float), P(c_float)]),
        "khp_debug_queue": (c_int, [c_void_p, P(c_uint32), P(c_float), P(c_float)]),
        "khp_debug_shadow_queue": (c_int, [c_void_p, P(c_uint32), P(c_float), P(c_float), P(c_float)]),
        "khp_debug_surface": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float), P(c_float), P(c_int32), P(c_float),
                                      P(c_float), P(c_int32)]),
        "khp_debug_bsdf_sample": (c_int, [c_void_p, c_uint32, c_uint32, P(c_int32), P(c_int32), P(c_float), P(c_float),
                                          P(c_float), P(c_float), P(c_int32), P(c_float), P(c_float), P(c_float),
                                          P(c_float), P(c_int32), P(c_int32)]),
        "khp_debug_bsdf_eval": (c_int, [c_void_p, c_uint32, P(c_int32), P(c_int32), P(c_float), P(c_float),
                                        P(c_float), P(c_float)]),
        "khp_hair_lobes_defaults": (None, [P(HairLobes)]),
        "khp_set_hair_lobes": (c_int, [c_void_p, P(HairLobes)]),
        "khp_get_hair_lobes": (c_int, [c_void_p, P(HairLobes)]),
        "khp_lens_defaults": (None, [P(Lens)]),
        "khp_lens_from_kirk": (c_int, [c_float, c_float, c_float, P(Lens)]),
        "khp_set_lens": (c_int, [c_void_p, P(Lens)]),
        "khp_get_lens": (c_int, [c_void_p, P(Lens)]),
        "khp_hair_material": (c_int, [P(c_float), c_float, c_float, c_float, c_float, P(Material)]),
        "khp_hair_eval_host": (c_int, [c_uint32, P(Material), P(c_float), P(c_float), P(c_float), P(c_float),
                                       P(c_float)]),
        "khp_hair_sample_host": (c_int, [c_uint32, P(Material), P(c_float), P(c_float), P(c_float), P(c_float),
                                         P(c_float), P(c_float), P(c_float), P(c_int32)]),
        "khp_camera_rays_host": (c_int, [P(Camera), P(Lens), c_uint32, c_uint32, c_uint32, P(c_uint32), P(c_uint32),
                                         P(c_float), P(c_float)]),
        "khp_debug_camera_rays": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, P(c_uint32), P(c_uint32), P(c_float),
                                          P(c_float)]),
        "khp_env_light_defaults": (None, [P(EnvLight)]),
        "khp_set_env_light": (c_int, [c_void_p, P(EnvLight)]),
        "khp_get_env_light": (c_int, [c_void_p, P(EnvLight)]),
        "khp_env_light_tables_host": (c_int, [P(EnvLight), P(c_uint32), P(c_uint32), P(ctypes.c_uint64)]),
        "khp_env_light_sample_host": (c_int, [P(EnvLight), c_uint32, P(c_float), P(c_float), P(c_float), P(c_float),
                                              P(c_int32)]),
        "khp_env_light_eval_host": (c_int, [P(EnvLight), c_uint32, P(c_float), P(c_float), P(c_float)]),
        "khp_debug_env_light_tables": (c_int, [c_void_p, P(c_uint32), P(c_uint32), P(ctypes.c_uint64)]),
        "khp_debug_env_light": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float), P(c_float), P(c_float), P(c_float),
                                        P(c_int32), P(c_float), P(c_float)]),
        "khp_kmath_host": (c_int, [c_uint32, c_uint32, P(ctypes.c_uint64), P(ctypes.c_uint64)]),
        "khp_debug_kmath": (c_int, [c_void_p, c_uint32, c_uint32, P(ctypes.c_uint64), P(ctypes.c_uint64)]),
        "khp_debug_hair_sample": (c_int, [c_void_p, c_uint32, c_uint32, P(c_int32), P(c_int32), P(c_float), P(c_float),
                                          P(c_float), P(c_float), P(c_int32), P(c_float), P(c_float), P(c_float),
                                          P(c_float), P(c_int32), P(c_int32)]),
        "khp_debug_light_dir": (c_int, [c_void_p, c_uint32, P(c_int32), P(c_float), P(c_float), P(c_float),
                                        P(c_float), P(c_float)]),
        "khp_debug_light_isect": (c_int, [c_void_p, c_uint32, P(c_int32), P(c_float), P(c_float), P(c_uint8),
                                          P(c_float), P(c_float)]),
        "khp_debug_light_paths": (c_int, [c_void_p, c_uint32, c_uint32, P(c_float)]),
        "khp_debug_bdpt_connect": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float), P(c_uint32), P(c_int32),
                                           P(c_uint32), P(c_float), P(c_uint8), P(c_uint8), P(c_float), P(c_float),
                                           P(c_float), P(c_float)]),
        "khp_debug_img_connect": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, P(c_float), P(c_uint32), P(c_float),
                                          P(c_float), P(c_uint8), P(c_float), P(c_float), P(c_float)]),
        "khp_debug_tex_color": (c_int, [c_void_p, c_uint32, P(c_int32), P(c_float), P(c_float)]),
        "khp_debug_env_color": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float)]),
        "khp_debug_material": (c_int, [c_void_p, c_uint32, P(c_float), P(c_float), P(c_float), P(c_int32), P(c_float),
                                       P(c_float), P(c_float), P(c_float), P(c_float), P(c_float), P(c_float)]),
        "khp_host_build": (c_int, [P(SceneDesc), P(c_uint32), P(c_uint32), P(c_float), P(c_int32), P(c_int32),
                                   P(c_int32), P(c_float), P(c_float)]),
        "khp_update_geometry": (c_int, [c_void_p, P(SceneDesc), P(RefitInfo)]),
        "khp_update_geometry_device": (c_int, [c_void_p, P(SceneDesc), P(RefitInfo)]),
        "khp_get_refit_info": (c_int, [c_void_p, P(RefitInfo)]),
        "khp_refit_host": (c_int, [P(SceneDesc), c_uint32, P(c_int32), P(c_int32), P(c_int32), P(c_float),
                                   P(c_float), P(c_float), P(ctypes.c_double)]),
        "khp_kernel_variant_host": (c_int, [c_uint32, P(VariantFacts), P(c_uint32), P(c_uint32), P(c_uint32)]),
        "khp_kernel_variant_table": (c_int, [c_uint32, c_uint32, P(c_uint32), P(c_uint32)]),
    }
    lib.khp_abi_version.restype = c_int
    lib.khp_abi_version.argtypes = []
    abi = lib.khp_abi_version()
    if abi != ABI_VERSION:   # the structs above would be read with the wrong layout
        raise RuntimeError(f"{p}: ABI {abi}, this package needs ABI {ABI_VERSION} (rebuild: __graft_entry__.build())")
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:   # a library of this ABI built before the symbol was added
            raise RuntimeError(f"{p}: no symbol {name}, this package needs it (rebuild: __graft_entry__.build())") from None
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class KhpError(RuntimeError):
    def __init__(self, status: int, where: str, msg: str):
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


def check(lib, status: int, where: str):
    if status != KHP_OK:
        raise KhpError(status, where, (lib.khp_last_error() or b"").decode())


def tonemap_log_sum(terms: np.ndarray, start: float = 0.0) -> np.float32:
    """khp_tonemap_log_sum (host only): KIRK's float running sum of double terms, in order."""
    lib = load_library()
    t = np.ascontiguousarray(terms, dtype=np.float64)
    out = c_float(0.0)
    check(lib, lib.khp_tonemap_log_sum(t.ctypes.data_as(POINTER(ctypes.c_double)), t.size, float(start),
                                       ctypes.byref(out)), "khp_tonemap_log_sum")
    return np.float32(out.value)


def kernel_variant(family: int, **facts) -> tuple:
    """khp_kernel_variant_host (host only): (the instance's template arguments, grid_kind) for the
    khp_variant_facts fields given (the others 0)."""
    lib = load_library()
    args, n, gk = (c_uint32 * 7)(), c_uint32(), c_uint32()
    f = VariantFacts(**{k: int(v) for k, v in facts.items()})
    check(lib, lib.khp_kernel_variant_host(family, ctypes.byref(f), args, ctypes.byref(n), ctypes.byref(gk)),
          "khp_kernel_variant_host")
    return tuple(args[:n.value]), gk.value


def kernel_variant_table(family: int) -> list:
    """khp_kernel_variant_table (host only): every compiled instance of the family, in table order."""
    lib = load_library()
    args, n, rows = (c_uint32 * 7)(), c_uint32(), []
    while lib.khp_kernel_variant_table(family, len(rows), args, ctypes.byref(n)) == KHP_OK:
        rows.append(tuple(args[:n.value]))
    return rows


def host_build(scene) -> dict:
    """Flatten + BVH build of the product, run on the host (no GPU): khp_host_build."""
    lib = load_library()
    d = scene.desc()
    nn, dep = c_uint32(), c_uint32()
    ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
    check(lib, lib.khp_host_build(ctypes.byref(d), ctypes.byref(nn), ctypes.byref(dep), None, None, None, None, None,
                                  None), "khp_host_build")
    n, m = nn.value, scene.n_objects
    boxes = np.empty((n, 6), np.float32)
    first = np.empty(n, np.int32)
    count = np.empty(n, np.int32)
    ids = np.empty(m, np.int32)
    bounds = np.empty((m, 9), np.float32)
    rec = np.empty((m, 16), np.float32)
    check(lib, lib.khp_host_build(ctypes.byref(d), ctypes.byref(nn), ctypes.byref(dep), fptr(boxes), ip(first),
                                  ip(count), ip(ids), fptr(bounds), fptr(rec)), "khp_host_build")
    return {"boxes": boxes, "first": first, "count": count, "ids": ids, "bounds": bounds, "records": rec,
            "depth": dep.value}


def refit_host(scene, bvh: dict) -> dict:
    """khp_refit_host (host only): the topology of `bvh` (host_build's or read_bvh's dict: first,
    count, ids) refitted to the moved `scene`: boxes, per-object bounds and records, sah_cost."""
    lib = load_library()
    d = scene.desc()
    ip = lambda a: a.ctypes.data_as(POINTER(c_int32))
    first = np.ascontiguousarray(bvh["first"], np.int32)
    count = np.ascontiguousarray(bvh["count"], np.int32)
    ids = np.ascontiguousarray(bvh["ids"], np.int32)
    n, m = first.size, scene.n_objects
    if count.size != n or ids.size != m:
        raise ValueError("refit_host: first / count / ids do not fit the scene")
    boxes = np.empty((n, 6), np.float32)
    bounds = np.empty((m, 9), np.float32)
    rec = np.empty((m, 16), np.float32)
    cost = ctypes.c_double(0.0)
    check(lib, lib.khp_refit_host(ctypes.byref(d), n, ip(first), ip(count), ip(ids), fptr(boxes), fptr(bounds),
                                  fptr(rec), ctypes.byref(cost)), "khp_refit_host")
    return {"boxes": boxes, "first": first, "count": count, "ids": ids, "bounds": bounds, "records": rec,
            "sah_cost": cost.value}


def gather_plan(width: int, height: int, tile: int, nranks: int, rank: int, root: int = 0):
    """khp_gather_plan (host only): (counts[nranks], pixel indices) that
    khp_gather_framebuffer moves, as seen from `rank`."""
    lib = load_library()
    n = c_uint64()
    check(lib, lib.khp_gather_plan(width, height, tile, nranks, rank, root, None, None, ctypes.byref(n)),
          "khp_gather_plan")
    counts = np.zeros(nranks, np.uint64)
    pix = np.zeros(max(1, n.value), np.uint32)
    check(lib, lib.khp_gather_plan(width, height, tile, nranks, rank, root, counts.ctypes.data_as(POINTER(c_uint64)),
                                   uptr(pix), ctypes.byref(n)), "khp_gather_plan")
    return counts, pix[:n.value]
