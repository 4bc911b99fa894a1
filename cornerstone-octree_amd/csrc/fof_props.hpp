// Device steps of the friends-of-friends group catalogue (fof_props.hip): the segmented reduction over the members of a
// catalogue, and what cstone_hip_domain_mr_fof_catalog (domain_mr.hip) needs around it -- runs of equal 64-bit labels, the
// partial of a rank about its local reference, the owner's combine and the finish.  The rule is stated in
// include/cstone_hip.h, cstone_hip_fof_group_properties.  Every call is asynchronous on the context's stream unless it
// says otherwise.
#pragma once

#include "ctx.hpp"

namespace cship
{

/*! what travels to the owner of a label: one record per distinct label of the sender's assigned particles.  sums = {M, Sx,
 *  Sy, Sz, Q, Px, Py, Pz} about ref, the position (exact in a double) of the sender's first member in (label, index) order */
struct FofPartial
{
    uint64_t label, count;
    double sums[8];
    double ref[3];
    uint32_t wide, pad;
};
static_assert(sizeof(FofPartial) == 112);

//! the outputs of the finish: rows of the coordinate type T, any of velocity, radius, flags, labels, sizes may be null
struct FofGroupOut
{
    void *mass, *center, *velocity, *radius;
    uint32_t* flags;
    uint64_t *labels, *sizes;
};

/*! the segmented reduction over members[0 .. group_offsets[num_groups]) (all device): finished rows into out, or, with
 *  partials != nullptr, one FofPartial per group (label: sortedLabels at the group's first member).  vx == nullptr: no
 *  velocities.  Uses the arena for the carries. */
int fofPropsReduce(cstone_hip_ctx* ctx, int realBits, int massBits, const void* x, const void* y, const void* z, const void* m,
                   const void* vx, const void* vy, const void* vz, const cstone_box& box, const uint32_t* groupOffsets,
                   const uint32_t* members, uint32_t numGroups, const FofGroupOut& out, FofPartial* partials,
                   const uint64_t* sortedLabels);

/*! runs of equal keys in keys[0 .. n) (sorted): runStart[r] (numRuns + 1 entries), runLabels[r] (nullable);
 *  host[0] = numRuns, host[1] = number of keys >= limit.  work: 2 n + 64 words.  Synchronises the stream; uses the arena. */
int fofRunsU64(cstone_hip_ctx* ctx, const uint64_t* keys, uint32_t n, uint64_t limit, uint32_t* work, uint32_t* runStart,
               uint64_t* runLabels, uint32_t host[2]);

//! keys[i] = records[i].label
void fofPartialLabels(cstone_hip_ctx* ctx, const FofPartial* records, uint32_t n, uint64_t* keys);

/*! the owner: run r of the sorted (label, record index) pairs is combined in that order about the position of the own
 *  particle first + (label - firstId) into combined[r] (label, count, sums, wide; ref = that position); keep[r] = count >=
 *  minMembers.  A label outside [firstId, firstId + numOwn) ORs 32 into the sticky error word and keeps nothing. */
int fofCombinePartials(cstone_hip_ctx* ctx, int realBits, const void* x, const void* y, const void* z, const cstone_box& box,
                       const FofPartial* records, const uint32_t* order, const uint32_t* runStart, uint32_t numRuns,
                       uint64_t firstId, uint32_t first, uint32_t numOwn, uint64_t minMembers, FofPartial* combined,
                       uint32_t* keep);

//! row pos[r] of out = the finished values of combined[r] for every r < numRuns with keep[r]
int fofFinishCombined(cstone_hip_ctx* ctx, int realBits, bool velocities, const cstone_box& box, const FofPartial* combined,
                      const uint32_t* keep, const uint32_t* pos, uint32_t numRuns, const FofGroupOut& out);

} // namespace cship
