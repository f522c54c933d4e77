// denoise_var_host.cpp -- khp_denoise_var_host and khp_denoise_noise_defaults: the host side
// of the a-trous filter guided by measured variance.  The per-pixel functions are
// denoise_var.h's, the ones the gfx950 kernels compile too; this is the plain loop over
// them, a reference that needs no device and no context.
#include <new>
#include <utility>
#include <vector>

#include "denoise_var.h"
#include "scene.h"

extern "C" void khp_denoise_noise_defaults(khp_denoise_noise* out) {
    if (!out) return;
    *out = khp_denoise_noise{};
    out->source = KHP_NOISE_PLANE;
    out->prefilter = 1;       // the trimmed 3 x 3 (the findings behind it)
    out->floor = 1e-6f;
}

extern "C" khp_status khp_denoise_var_host(const khp_denoise_params* p, const float* colour, const khp_aov_buffers* guides,
                                           const khp_denoise_noise* noise, float* out) {
    using namespace khp;
    DnParams P{};
    DnPlanes G{};
    DnvNoise Z{};
    khp_status st;
    if (const char* why = dnv_check(p, colour, guides, noise, out, true, P, G, Z, st)) return fail(st, why);
    const size_t npix = (size_t)P.W * P.H;
    std::vector<DnRec> g0, g1, a, b;
    std::vector<DnVar> va, vb;
    try {
        for (auto* v : {&g0, &g1, &a, &b}) v->resize(npix);
        va.resize(npix);
        vb.resize(npix);
    } catch (const std::bad_alloc&) {
        return fail(KHP_ENOMEM, "khp_denoise_var_host: no memory for 80 bytes per pixel");
    }
    for (size_t i = 0; i < npix; ++i) dnv_prepare(P, G, Z, i, g0[i], g1[i], a[i], va[i]);
    for (uint32_t it = 0; it < p->iterations; ++it) {
        const int s = 1 << it;
        for (uint32_t y = 0; y < P.H; ++y)
            for (uint32_t x = 0; x < P.W; ++x) {
                const size_t i = (size_t)y * P.W + x;
                b[i] = Z.prefilter ? dnv_filter<true>(P, Z.floor, (int)x, (int)y, s, g0.data(), g1.data(), a.data(), va.data(), vb[i])
                                   : dnv_filter<false>(P, Z.floor, (int)x, (int)y, s, g0.data(), g1.data(), a.data(), va.data(), vb[i]);
            }
        std::swap(a, b);
        std::swap(va, vb);
    }
    for (size_t i = 0; i < npix; ++i) {
        out[3 * i] = a[i].x;
        out[3 * i + 1] = a[i].y;
        out[3 * i + 2] = a[i].z;
        if (Z.out_variance) Z.out_variance[i] = dnv_finish_variance(va[i]);
    }
    return KHP_OK;
}
