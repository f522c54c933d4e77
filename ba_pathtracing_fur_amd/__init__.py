"""MI355X-native fur path-tracing core (the hot path of lucashilbig/BA_Pathtracing_Fur).

The product is libkirk_hip.so (HIP kernels for gfx950 behind the C-ABI in
include/kirk_hip.h).  This package holds its ctypes binding, the seeded scene
inputs, and a KIRK-shaped host interface.  No pixel is computed in Python and
there is no CPU fallback.
"""
import os as _os


def set_hw_queues(n: int = 8) -> None:
    """Set GPU_MAX_HW_QUEUES (hardware queues per process; HIP's default is 4)
    for this process.  HIP reads it once, when the runtime initialises, so this
    must run before the first khp_create (or any other HIP call) in the process.
    The default context (one batch in flight) uses three streams, which fit in
    the default four queues; with khp_ctx_params.frames_in_flight = 2 or 3 the
    extra streams share queues unless this is raised.  Never
    called implicitly: the host program decides."""
    _os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))


from . import native  # noqa: E402,F401
from .native import (AOV_CHANNELS, DENOISE_DEMODULATE, DENOISE_DEVICE, HAIR_LOBE_R, HAIR_LOBE_TRT,  # noqa: E402
                     HAIR_LOBE_TT, LENS_FOCUS_KIRK, LENS_FOCUS_PLANE, MOMENTS_DEVICE, MOMENTS_PLANES, NOISE_CONTEXT,
                     NOISE_MOMENTS, NOISE_PLANE, REPROJECT_DEVICE, REPROJECT_MATCH_OBJECT, AdaptiveParams, AovBuffers,
                     DenoiseNoise, DenoiseParams, ReprojectFrame, ReprojectOut, ReprojectParams)
from .pathtracer import (BVH, BsdfFactory, HipContext, PathTracer, ShaderFactory, TemporalAccumulator,  # noqa: E402
                         adaptive_select_host, camera_rays_host, comm_unique_id, denoise_host, denoise_var_host,
                         env_light_eval_host, env_light_sample_host, env_light_tables_host, hair_eval_host, kmath_host,
                         hair_sample_host, lens_from_kirk, moments_fold_host, moments_variance, reproject_host)
from .native import refit_host  # noqa: E402
from .scenes import SceneData, build_config  # noqa: E402

__all__ = ["set_hw_queues", "native", "BVH", "BsdfFactory", "HipContext", "PathTracer", "ShaderFactory", "SceneData",
           "build_config", "comm_unique_id", "HAIR_LOBE_R", "HAIR_LOBE_TT", "HAIR_LOBE_TRT", "AovBuffers",
           "AOV_CHANNELS", "DenoiseParams", "DENOISE_DEVICE", "DENOISE_DEMODULATE", "denoise_host", "MOMENTS_DEVICE",
           "MOMENTS_PLANES", "moments_fold_host", "moments_variance", "AdaptiveParams", "adaptive_select_host", "DenoiseNoise",
           "NOISE_PLANE", "NOISE_MOMENTS", "NOISE_CONTEXT", "denoise_var_host", "ReprojectParams", "ReprojectFrame",
           "ReprojectOut", "REPROJECT_DEVICE", "REPROJECT_MATCH_OBJECT", "reproject_host", "TemporalAccumulator",
           "LENS_FOCUS_KIRK", "LENS_FOCUS_PLANE", "lens_from_kirk", "camera_rays_host", "hair_eval_host", "hair_sample_host",
           "env_light_tables_host", "env_light_sample_host", "env_light_eval_host", "kmath_host", "refit_host"]
