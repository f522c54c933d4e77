// adaptive_host.cpp -- khp_adaptive_defaults and khp_adaptive_select_host: the host side of
// the adaptive passes.  The rule is adaptive.h's, the one the gfx950 selection kernel
// compiles too; this is the plain loop over it, a reference that needs no device and no
// context.
#include "adaptive.h"
#include "scene.h"

extern "C" void khp_adaptive_defaults(khp_adaptive_params* out) {
    if (!out) return;
    *out = khp_adaptive_params{};
    out->threshold = 0.05f;
    out->min_samples = 8u;
}

extern "C" khp_status khp_adaptive_select_host(const khp_adaptive_params* prm, uint32_t first_sample,
                                               const khp_moments_buffers* state, uint32_t n_owned,
                                               const uint32_t* owned, uint32_t* active, uint32_t* n_active) {
    using namespace khp;
    if (!prm || !state || !n_active) return fail(KHP_EINVAL, "khp_adaptive_select_host: null argument");
    if (const char* why = adapt_params_error(prm)) return fail(KHP_EINVAL, std::string("khp_adaptive_select_host: ") + why);
    if (!state->mean || !state->m2 || !state->count || !state->bad)
        return fail(KHP_EINVAL, "khp_adaptive_select_host: a null state plane (mean, m2, count and bad are needed)");
    if (n_owned != 0u && (!owned || !active)) return fail(KHP_EINVAL, "khp_adaptive_select_host: null pixel list");
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_owned; ++i) {
        const size_t p = owned[i];
        const MomRec a = {state->mean[3 * p], state->mean[3 * p + 1], state->mean[3 * p + 2], state->count[p]};
        const MomRec b = {state->m2[3 * p], state->m2[3 * p + 1], state->m2[3 * p + 2], state->bad[p]};
        if (adapt_active(*prm, first_sample, a, b)) active[n++] = owned[i];
    }
    *n_active = n;
    return KHP_OK;
}
