// denoise_host.cpp -- khp_denoise_host and khp_denoise_params_defaults: the host
// side of the guided a-trous filter.  The per-pixel functions are denoise.h's,
// the ones the gfx950 kernels compile too; this is the plain loop over them, a
// reference that needs no device and no context.
#include <new>
#include <utility>
#include <vector>

#include "denoise.h"
#include "scene.h"

extern "C" void khp_denoise_params_defaults(khp_denoise_params* out) {
    if (!out) return;
    *out = khp_denoise_params{};
    out->iterations = 5;
    out->sigma_color = 4.0f;      // radiance units (the sweep behind these)
    out->sigma_normal = 0.35f;
    out->sigma_tangent = 0.35f;
    out->sigma_depth = 0.05f;
    out->sigma_coverage = 0.25f;
}

extern "C" khp_status khp_denoise_host(const khp_denoise_params* p, const float* colour, const khp_aov_buffers* guides,
                                       float* out) {
    using namespace khp;
    DnParams P{};
    DnPlanes G{};
    if (const char* why = dn_check(p, colour, guides, out, true, P, G)) return fail(KHP_EINVAL, why);
    const size_t npix = (size_t)P.W * P.H;
    std::vector<DnRec> g0, g1, mod, a, b;
    try {
        for (auto* v : {&g0, &g1, &mod, &a, &b}) v->resize(npix);
    } catch (const std::bad_alloc&) {
        return fail(KHP_ENOMEM, "khp_denoise_host: no memory for 80 bytes per pixel");
    }
    for (size_t i = 0; i < npix; ++i) dn_prepare(P, G, i, g0[i], g1[i], a[i], mod[i]);
    for (uint32_t it = 0; it < p->iterations; ++it) {
        const int s = 1 << it;
        for (uint32_t y = 0; y < P.H; ++y)
            for (uint32_t x = 0; x < P.W; ++x)
                b[(size_t)y * P.W + x] = dn_filter(P, (int)x, (int)y, s, g0.data(), g1.data(), a.data());
        std::swap(a, b);
    }
    for (size_t i = 0; i < npix; ++i) dn_finish(P, a[i], mod[i], out + 3 * i);
    return KHP_OK;
}
