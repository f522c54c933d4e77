// moments.h -- the definition of the per-pixel sample moments (kirk_hip.h,
// DESIGN.md §14): beside the framebuffer's running mean, per pixel the count of
// finite samples, their mean, their sum of squared deviations M2 (Welford) and
// the count of rejected samples.
//
// Everything that computes a value is a KHD function in this header, compiled
// into the host entry (moments_host.cpp, g++) and into the gfx950 kernels
// (k_accumulate_m, k_accumulate_all_m and k_moments_read of render.hip /
// moments_dev.h).  Every operation is one float32 operation in the order
// written; both sides build with -ffp-contract=off, so the two give the same
// bits, and tests/_momentsref.py restates the same sequence in numpy.
//
// The state of a pixel is two 16-byte records, the integers carried as bits:
//   a = (mean.r, mean.g, mean.b, n)      b = (m2.r, m2.g, m2.b, bad)
// all zero when made.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kirk_hip.h"
#include "kmath.h"

namespace khp {

// One 16-byte record; every load or store of one is a single aligned 128-bit access.
struct alignas(16) MomRec {
    float x, y, z;
    uint32_t w;
};

KHD bool mom_finite(float x) { return (bits_from_f(x) & 0x7f800000u) != 0x7f800000u; }

KHD void mom_channel(float x, float nf, float& mean, float& m2) {
    const float d = x - mean;
    mean = mean + d / nf;
    const float e = x - mean;
    m2 = m2 + d * e;
}

// Fold the sample colour (xr, xg, xb) whose global sample index is k.
KHD void mom_fold(MomRec& a, MomRec& b, float xr, float xg, float xb, uint32_t k) {
    if (k == 0) {   // the framebuffer's own restart rule
        a.x = a.y = a.z = 0.0f;
        b.x = b.y = b.z = 0.0f;
        a.w = b.w = 0u;
    }
    if (!(mom_finite(xr) && mom_finite(xg) && mom_finite(xb))) {
        b.w += 1u;
        return;
    }
    a.w += 1u;
    if (a.w == 1u) {   // an assignment: -0 survives, as in the framebuffer's k == 0 case
        a.x = xr; a.y = xg; a.z = xb;
        b.x = b.y = b.z = 0.0f;
        return;
    }
    const float nf = (float)a.w;   // exact up to 2^24 samples, the cap on spp
    mom_channel(xr, nf, a.x, b.x);
    mom_channel(xg, nf, a.y, b.y);
    mom_channel(xb, nf, a.z, b.z);
}

// The relative standard error of the pixel's mean, channels summed; +inf below two samples.
KHD float mom_rel_error(const MomRec& a, const MomRec& b) {
    const float s = (b.x + b.y) + b.z;
    const float mu = (a.x + a.y) + a.z;
    if (a.w < 2u) return k_inf();
    const float nf = (float)a.w;
    return sqrtf(s / (nf * (nf - 1.0f))) / (fabsf(mu) + 1e-3f);
}

}  // namespace khp
