// Device steps of friends-of-friends across ranks (cstone_hip_domain_mr_fof, domain_mr.hip) beside the public lowering
// step cstone_hip_fof_lower_labels: the cover condition's smallest halo radius, the count of the groups a rank owns, and
// the three ends of the group-size protocol.  The kernels are in fof.hip; every call is asynchronous on the context's
// stream unless it says otherwise.
#pragma once

#include "ctx.hpp"

namespace cship
{

//! what travels to the owner of a label: the label and the assigned members one local component of the sender has
struct FofPair
{
    uint64_t label, count;
};

//! *outBits = min(*outBits, bit pattern of radii[leaf]) over the leaves of [first, last) with counts[leaf] > 0; the
//! caller presets the word (the bits of +inf, 0x7f800000)
void fofMinRadius(cstone_hip_ctx* ctx, const float* radii, const uint32_t* counts, int first, int last, uint32_t* outBits);

//! *word = *word ? 1 : 0
void fofClampFlag(cstone_hip_ctx* ctx, uint32_t* word);

//! *numOwn += the k < n with labels[k] == firstId + k
void fofCountOwn(cstone_hip_ctx* ctx, const uint64_t* labels, uint32_t n, uint64_t firstId, uint32_t* numOwn);

/*! count[c] (n words) = the members k in [first, last) of component c; one pair per c with count[c] > 0, in ascending c:
 *  keys[i] = labels[c], values[i] = c.  *numPairsHost: their number (synchronises the stream).  Uses the arena. */
int fofComponentPairs(cstone_hip_ctx* ctx, const uint32_t* component, uint32_t n, uint32_t first, uint32_t last,
                      const uint64_t* labels, uint32_t* count, uint64_t* keys, uint32_t* values, uint32_t* numPairsHost);

//! pairs[i] = {keys[i], count[values[i]]}
void fofPackPairs(cstone_hip_ctx* ctx, const uint64_t* keys, const uint32_t* values, const uint32_t* count,
                  uint32_t numPairs, FofPair* pairs);

//! the owner: totals[label - firstId] (numOwn words, zeroed here) += count over the pairs, answers[i] = the total of
//! pairs[i]'s label
int fofOwnerTotals(cstone_hip_ctx* ctx, const FofPair* pairs, uint32_t numPairs, uint64_t firstId, uint32_t numOwn,
                   uint64_t* totals, uint64_t* answers);

//! componentTotals[values[i]] = answers[i], then sizes[k] = componentTotals[component[k]] for k in [first, last)
void fofSizesFromAnswers(cstone_hip_ctx* ctx, const uint32_t* values, const uint64_t* answers, uint32_t numPairs,
                         const uint32_t* component, uint32_t first, uint32_t last, uint64_t* componentTotals,
                         uint64_t* sizes);

} // namespace cship
