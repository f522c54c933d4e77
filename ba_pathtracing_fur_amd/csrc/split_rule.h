// split_rule.h -- where KIRK's BVH recursion is undefined, and what the builders
// do there.  One definition for the host builder (scene.cpp)
// and both phases of the device builder (bvh_build.hip); the oracle and
// tests/_bvhref.py restate it.
//
// BVHNode::partition computes, per axis, cbdiff = cbmax - cbmin and
// k = (16 * 0.9f) / cbdiff, and indexes bin_bounds[16] with
// (int)(k * (c - cbmin)) (CPU_BVH.cpp:378-403).  For finite input that is in
// range exactly when cbdiff and k are finite:
//   * cbdiff overflows to +inf for centroids more than FLT_MAX apart; k is 0
//     and 0 * inf is NaN;
//   * k overflows to +inf for 0 < cbdiff < 14.4 / FLT_MAX (about 4.2e-38); the
//     products are +inf, or NaN at c == cbmin.
// The float -> int conversion of such a value is undefined in C++ (x86 gives
// INT_MIN, the GPU saturates) and KIRK writes outside its bins.  Likewise,
// when no plane's cost is below FLT_MAX (areas that overflow), KIRK partitions
// by plane 0 of axis 0 with uninitialised child centroid boxes.
//
// The rule: a node whose split is undefined is a leaf.  Wherever KIRK's
// behaviour is defined, nothing changes: worth(cb) implies cbdiff > 0, and a
// finite k keeps k * (c - cbmin) within [0, 14.4 (1 + 2^-22)].
#pragma once

#include "kmath.h"

namespace khp {

// Beside worthSplitting(): the centroid box (mn, mx) gives a finite extent and a finite k on every axis.
KHD bool split_defined(const float* mn, const float* mx) {
    for (int a = 0; a < 3; ++a) {
        const float cbdiff = mx[a] - mn[a];
        const float k = (16.0f * (1.0f - 0.1f)) / cbdiff;
        // x - x is 0 for finite x and NaN for an infinity or a NaN
        if (cbdiff - cbdiff != 0.0f || k - k != 0.0f) return false;
    }
    return true;
}

// The SAH sweep found a plane: some cost was below its initial best, FLT_MAX.
KHD bool cost_defined(float best) { return best < 3.402823466e+38f; }

}  // namespace khp
