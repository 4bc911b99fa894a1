// The absolute term of the node tests of the walks whose particle test is the authority (csrc/sphere.hip, knn.hip,
// pair_counts.hip).  Free of HIP so that a plain host program can call it (tools/knn_rules_check.cpp does, under the
// sanitizers).
#pragma once

#include <cmath>

#include "cstone_hip.h"

namespace cship
{

/*! factor * eps * L in T, with eps the machine epsilon of T and L the largest of |lo_a|, |hi_a| and len_a over the axes
 *  of the box.  The factor is the caller's and comes with a derivation: 64 where a point meets a node's box (at
 *  sphereProfilesKernel in sphere.hip; knn.hip takes it over), 256 where a box of targets does (at pairCountsKernel in
 *  pair_counts.hip). */
template<class T>
inline T nodeAbsMargin(const cstone_box& b, double factor)
{
    double L = 0;
    for (int a = 0; a < 3; ++a)
        L = std::fmax(L, std::fmax(std::fmax(std::fabs(b.lim[2 * a]), std::fabs(b.lim[2 * a + 1])), b.lim[2 * a + 1] - b.lim[2 * a]));
    const double eps = sizeof(T) == 4 ? 1.1920928955078125e-07 : 2.220446049250313e-16;
    return T(factor * eps * L);
}

} // namespace cship
