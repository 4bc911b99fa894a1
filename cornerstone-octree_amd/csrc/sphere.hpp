// Sphere queries on the octree (csrc/sphere.hip): what the rest of the library needs of them.  The rule is stated in
// include/cstone_hip.h, cstone_hip_sphere_profiles.
#pragma once

#include <cstddef>
#include <cstdint>

#include "ctx.hpp"

namespace cship
{

//! are edges[0 .. numBins] what the rule asks for: 1 <= numBins <= CSTONE_SPHERE_MAX_BINS, finite, edges[0] >= 0,
//! strictly ascending?  (host; decided before anything is launched, and before any collective on several ranks)
bool sphereEdgesOk(const double* edges, int numBins);

/*! the operand of the all-reduce of cstone_hip_domain_mr_sphere_profiles: buf[k] = double(counts[k]), buf[n + k] =
 *  sums[k] for k < n (sums == nullptr: only the first half is written).  Counts below 2^53 travel exactly. */
void spherePackRows(cstone_hip_ctx* ctx, const uint64_t* counts, const double* sums, size_t n, double* buf);
//! and back: counts[k] = uint64(buf[k]), sums[k] = buf[n + k] (sums nullable)
void sphereUnpackRows(cstone_hip_ctx* ctx, const double* buf, size_t n, uint64_t* counts, double* sums);

} // namespace cship
