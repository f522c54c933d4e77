// adaptive.h -- the definition of an adaptive pass's pixel selection (kirk_hip.h,
// DESIGN.md §15): which owned pixels khp_render_adaptive traces, read off the moments
// state of moments.h.
//
// The rule is one KHD function, compiled into the host entry (adaptive_host.cpp, g++) and
// into the gfx950 selection kernel (k_adapt_flag of adaptive_dev.h).  The value it compares
// is mom_rel_error of moments.h, the error plane's own function, so both sides decide on
// the same bits; tests/_adaptiveref.py restates the rule in numpy.
#pragma once

#include "moments.h"

namespace khp {

// NULL when the parameters are usable, else what is wrong with them.
inline const char* adapt_params_error(const khp_adaptive_params* a) {
    if (!a) return "null argument";
    if (!(a->threshold >= 0.0f)) return "threshold must be >= 0 and not NaN";
    if (a->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// Whether the pixel with records a = (mean, n), b = (m2, bad) is traced by a pass that starts at first_sample.
KHD bool adapt_active(const khp_adaptive_params& prm, uint32_t first_sample, const MomRec& a, const MomRec& b) {
    if (first_sample == 0u) return true;                       // a restart: mom_fold's k == 0 rule zeroes the state
    const uint64_t t = (uint64_t)a.w + (uint64_t)b.w;          // samples taken, finite or not
    if (t < prm.min_samples) return true;
    if (prm.max_samples != 0u && t >= prm.max_samples) return false;
    // negated: a NaN error (an overflowed m2) stays active.  Below two samples the error is +inf by
    // definition and the pixel stays active at every threshold, +inf included (+inf <= +inf holds, so
    // the comparison alone would call it converged there).
    return a.w < 2u || !(mom_rel_error(a, b) <= prm.threshold);
}

}  // namespace khp
