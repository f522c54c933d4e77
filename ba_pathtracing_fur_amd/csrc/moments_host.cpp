// moments_host.cpp -- khp_moments_defaults and khp_moments_fold_host: the host side
// of the per-pixel sample moments.  The fold and the error plane are moments.h's,
// the ones the gfx950 kernels compile too; this is the plain loop over them, a
// reference that needs no device and no context.
#include "moments.h"
#include "scene.h"

extern "C" void khp_moments_defaults(khp_moments* out) {
    if (!out) return;
    *out = khp_moments{};   // off
}

extern "C" khp_status khp_moments_fold_host(uint32_t n_pixels, uint32_t first_sample, uint32_t n_samples,
                                            const float* samples, const khp_moments_buffers* state) {
    using namespace khp;
    if (!state || !samples) return fail(KHP_EINVAL, "khp_moments_fold_host: null argument");
    if (!state->mean || !state->m2 || !state->count || !state->bad)
        return fail(KHP_EINVAL, "khp_moments_fold_host: a null state plane (mean, m2, count and bad are needed)");
    if (n_pixels == 0) return fail(KHP_EINVAL, "khp_moments_fold_host: n_pixels must be > 0");
    if ((uint64_t)first_sample + n_samples > 0xFFFFFFFFull)
        return fail(KHP_EINVAL, "khp_moments_fold_host: first_sample + n_samples overflows");
    for (size_t p = 0; p < n_pixels; ++p) {
        MomRec a = {state->mean[3 * p], state->mean[3 * p + 1], state->mean[3 * p + 2], state->count[p]};
        MomRec b = {state->m2[3 * p], state->m2[3 * p + 1], state->m2[3 * p + 2], state->bad[p]};
        for (uint32_t s = 0; s < n_samples; ++s) {
            const float* x = samples + 3 * ((size_t)s * n_pixels + p);
            mom_fold(a, b, x[0], x[1], x[2], first_sample + s);
        }
        state->mean[3 * p] = a.x; state->mean[3 * p + 1] = a.y; state->mean[3 * p + 2] = a.z;
        state->m2[3 * p] = b.x; state->m2[3 * p + 1] = b.y; state->m2[3 * p + 2] = b.z;
        state->count[p] = a.w;
        state->bad[p] = b.w;
        if (state->rel_error) state->rel_error[p] = mom_rel_error(a, b);
    }
    return KHP_OK;
}
