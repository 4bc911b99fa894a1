// k nearest neighbours on the octree (csrc/knn.hip): the host rules of cstone_hip_knn, kept free of HIP so that a plain
// host program can call them (tools/knn_rules_check.cpp does, under the sanitizers).  The rule of the call is stated in
// include/cstone_hip.h, cstone_hip_knn.
#pragma once

#include <cstddef>
#include <cstdint>

#include "cstone_hip.h"
#include "node_margin.hpp" // the absolute term of the node test: nodeAbsMargin(box, 64)

namespace cship
{

/*! why a cstone_hip_knn call is refused with CSTONE_E_ARG, or nullptr if it is taken.  requiredPointers: are all the
 *  pointers the call needs non-null?  (they are looked at only while there are queries) */
inline const char* knnRefusal(int realBits, uint32_t k, uint32_t first, uint32_t last, uint32_t numQueries, bool requiredPointers)
{
    if (realBits != 32 && realBits != 64) return "real_bits unsupported";
    if (k < 1 || k > CSTONE_KNN_MAX_K) return "k outside 1 .. CSTONE_KNN_MAX_K";
    if (last < first) return "last < first";
    if (numQueries > 0 && !requiredPointers) return "null pointer";
    return nullptr;
}

//! list registers per lane for k: ceil(k / 64) rounded up to an instantiated count (1, 2, 4)
inline int knnListRegisters(uint32_t k) { return k <= 64 ? 1 : k <= 128 ? 2 : 4; }

/*! How many queries one all_gather of cstone_hip_domain_mr_knn carries: every rank sends 16 k bytes per query and receives
 *  numRanks times that, so  floor(capBytes / (16 k numRanks))  queries keep the receive buffer under capBytes; at least 1
 *  (a single query whose records exceed the cap still travels, alone), at most numQueries.  It follows from Q, k, P and
 *  the cap alone, so every rank cuts the same chunks.  0 for no queries. */
inline uint32_t knnChunkQueries(uint32_t numQueries, uint32_t k, int numRanks, uint64_t capBytes)
{
    if (numQueries == 0 || k == 0 || numRanks < 1) return 0;
    const uint64_t perQuery = uint64_t(16) * k * uint64_t(numRanks);
    const uint64_t fit      = capBytes / perQuery;
    return uint32_t(fit < 1 ? 1 : fit > numQueries ? numQueries : fit);
}

//! one slot of a rank's answer as it travels: the bits of d2 (f32: zero-extended) and the global id; all ones: unfilled
struct KnnRecord
{
    uint64_t d2, id;
};

/*! the local search of cstone_hip_domain_mr_knn (csrc/knn.hip): cstone_hip_knn without query_self, writing
 *  records[q][0 .. k) with the ids idBase + (j - first).  An empty range touches neither the particles nor the tree. */
int knnLocalRecords(cstone_hip_ctx* ctx, int realBits, const void* x, const void* y, const void* z, uint32_t first,
                    uint32_t last, const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf,
                    const uint32_t* layout, const void* centers, const void* sizes, const void* queryCenters,
                    const void* queryRmax, uint32_t numQueries, uint32_t k, uint64_t idBase, KnnRecord* records);
/*! the merge: rows[p][q][0 .. k) of numRanks ranks, whose id ranges ascend with p, into ids, dist2 (nullable) and counts
 *  (nullable) of numQueries queries */
int knnMergeRecords(cstone_hip_ctx* ctx, int realBits, const KnnRecord* rows, int numRanks, const void* queryRmax,
                    uint32_t numQueries, uint32_t k, uint64_t* ids, void* dist2, uint32_t* counts);

} // namespace cship
