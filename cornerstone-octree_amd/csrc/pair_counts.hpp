// Pair counts in radial bins (csrc/pair_counts.hip): what the rest of the library needs of them.  The rule is stated in
// include/cstone_hip.h, cstone_hip_pair_counts.
#pragma once

#include "ctx.hpp"

namespace cship
{

/*! why a call with these arguments is refused, or nullptr: bad real_bits, bad w_bits with a w, numBins outside
 *  1 .. CSTONE_PAIR_MAX_BINS, edges not finite, negative or not strictly ascending, no box, an outer edge that is not
 *  below half of every periodic edge.  Host only and the same on every rank that passes the same arguments: the domains
 *  ask before any collective. */
const char* pairCountsRefusal(int realBits, int wBits, bool wGiven, const cstone_box* box, const double* edges, int numBins);

} // namespace cship
