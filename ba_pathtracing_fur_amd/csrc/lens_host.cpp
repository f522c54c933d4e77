// lens_host.cpp -- khp_lens_defaults, khp_lens_from_kirk and khp_camera_rays_host: the
// host side of the thin-lens camera.  The ray function is lens.h's, the one the gfx950
// kernels compile too; this is the plain loop over it, a reference that needs no device
// and no context.
#include "lens.h"
#include "scene.h"

extern "C" void khp_lens_defaults(khp_lens* out) {
    if (!out) return;
    *out = khp_lens{};
    out->radius = 0.0f;             // off: KIRK's path tracer never calls transformToDof
    out->focus_distance = 11.0f;    // Camera::m_focus_distance (Camera.h:116)
    out->focus = KHP_LENS_FOCUS_KIRK;
}

static bool finite_positive(float x) { return x > 0.0f && x != khp::k_inf(); }

extern "C" khp_status khp_lens_from_kirk(float focal_length, float f_stop, float focus_distance, khp_lens* out) {
    using namespace khp;
    if (!out) return fail(KHP_EINVAL, "khp_lens_from_kirk: null argument");
    if (!finite_positive(focal_length)) return fail(KHP_EINVAL, "khp_lens_from_kirk: focal_length must be finite and > 0");
    if (!finite_positive(f_stop)) return fail(KHP_EINVAL, "khp_lens_from_kirk: f_stop must be finite and > 0");
    if (!finite_positive(focus_distance))
        return fail(KHP_EINVAL, "khp_lens_from_kirk: focus_distance must be finite and > 0");
    const float aperture = focal_length / f_stop;   // Camera::m_aperture
    const float radius = aperture * 3.0f;           // glm::diskRand(m_aperture * 3) (Camera.cpp:43)
    if (radius == k_inf()) return fail(KHP_EINVAL, "khp_lens_from_kirk: radius must be finite and >= 0");
    khp_lens l{};
    l.radius = radius;
    l.focus_distance = focus_distance;
    l.focus = KHP_LENS_FOCUS_KIRK;
    *out = l;
    return KHP_OK;
}

namespace khp {
// The checks khp_camera_rays_host and khp_debug_camera_rays share; null: the call is fine.
const char* camera_rays_error(const khp_lens* lens, uint32_t width, uint32_t n, const void* pixels,
                              const void* samples, const void* orig, const void* dir) {
    if (!pixels || !samples || !orig || !dir) return "null argument";
    if (width == 0u) return "width must be > 0";
    if (n == 0u || n > (1u << 20)) return "n must be in [1, 2^20]";
    if (lens) return lens_error(lens);
    return nullptr;
}
}  // namespace khp

extern "C" khp_status khp_camera_rays_host(const khp_camera* cam, const khp_lens* lens, uint32_t width, uint32_t seed,
                                           uint32_t n, const uint32_t* pixels, const uint32_t* samples, float* orig,
                                           float* dir) {
    using namespace khp;
    if (!cam) return fail(KHP_EINVAL, "khp_camera_rays_host: null argument");
    if (const char* why = camera_rays_error(lens, width, n, pixels, samples, orig, dir))
        return fail(KHP_EINVAL, std::string("khp_camera_rays_host: ") + why);
    khp_lens off;
    khp_lens_defaults(&off);
    const khp_lens& l = lens ? *lens : off;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t pixel = pixels[i];
        const uint32_t key = path_key(seed, pixel, samples[i]);
        v3 o, d;
        camera_ray(*cam, l, pixel % width, pixel / width, key, o, d);
        orig[3 * (size_t)i] = o.x; orig[3 * (size_t)i + 1] = o.y; orig[3 * (size_t)i + 2] = o.z;
        dir[3 * (size_t)i] = d.x; dir[3 * (size_t)i + 1] = d.y; dir[3 * (size_t)i + 2] = d.z;
    }
    return KHP_OK;
}
