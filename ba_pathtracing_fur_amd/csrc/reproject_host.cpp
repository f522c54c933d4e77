// reproject_host.cpp -- khp_reproject_host and khp_reproject_params_defaults: the host
// side of the temporal reprojection.  The per-pixel function is reproject.h's, the one
// the gfx950 kernel compiles too; this is the plain loop over it, a reference that
// needs no device and no context.
#include "reproject.h"
#include "scene.h"

extern "C" void khp_reproject_params_defaults(khp_reproject_params* out) {
    if (!out) return;
    *out = khp_reproject_params{};
    out->samples = 1.0f;          // a 1-spp pass per frame, the GUI loop's
    out->max_history = 32.0f;     // starting values, not a measured optimum
    out->depth_tol = 0.05f;
    out->normal_tol = 0.0f;       // off: a fibre's normal turns across its sub-pixel width
    out->tangent_tol = 0.25f;     // 1 - cos, about 41 degrees between fibre directions
    out->coverage_tol = 0.5f;
}

extern "C" khp_status khp_reproject_host(const khp_reproject_params* p, const khp_reproject_frame* cur,
                                         const khp_reproject_frame* hist, const khp_reproject_out* out) {
    using namespace khp;
    RpParams P{};
    RpFrame C{}, Hs{};
    RpOut O{};
    if (const char* why = rp_check(p, cur, hist, out, true, P, C, Hs, O)) return fail(KHP_EINVAL, why);
    for (uint32_t y = 0; y < P.H; ++y)
        for (uint32_t x = 0; x < P.W; ++x) rp_pixel(P, C, Hs, O, x, y);
    return KHP_OK;
}
