// Host-side pieces shared by the single-rank and the multi-rank Domain orchestration (domain.hip, domain_mr.hip).
// host_rules.hpp (no HIP): the box rule, the start pass of a partial sort, the acceptance of a re-sort, the sort switches
// and the update step of the small GLOBAL tree restated for the host.  Here, on top of a context and device buffers: the
// growth of a tree's capacity, a pinned block for the read-backs of a sync, and the host's copy of the global tree.
#pragma once

#include <cstdint>
#include <vector>

#include "ctx.hpp"
#include "devbuf.hpp"
#include "device_keys.hpp"
#include "host_rules.hpp"

namespace cship
{

static_assert(hostMaxLevel<uint32_t>() == maxLevel<uint32_t>() && hostMaxLevel<uint64_t>() == maxLevel<uint64_t>());

//! room for `need` leaves in a leaf array and its counts (contents kept), grown by half at least
template<class K>
int ensureTree(cstone_hip_ctx* ctx, DevBuf& tree, DevBuf& counts, int& cap, int need)
{
    if (need <= cap) return CSTONE_OK;
    int newCap = std::max(need, int(cap * 1.5));
    CS_TRY(tree.ensure(ctx, size_t(newCap + 1) * sizeof(K), true));
    CS_TRY(counts.ensure(ctx, size_t(newCap) * sizeof(uint32_t), true));
    cap = newCap;
    return CSTONE_OK;
}

//! pinned host block for the read-backs of a sync: an asynchronous copy into PAGEABLE memory makes the host wait for it,
//! which would turn every one of the copies that are meant to travel behind one synchronisation into a round trip
struct PinnedBlock
{
    char* p      = nullptr;
    size_t bytes = 0, used = 0;
    ~PinnedBlock()
    {
        if (p) (void)hipHostFree(p);
    }
    //! room for `need` more bytes (64-byte aligned); grows only while nothing is handed out (used == 0)
    void* take(size_t need)
    {
        const size_t at = (used + 63) & ~size_t(63);
        if (at + need > bytes) return nullptr;
        used = at + need;
        return p + at;
    }
    int reserve(cstone_hip_ctx* ctx, size_t total)
    {
        used = 0;
        if (total <= bytes) return CSTONE_OK;
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (p) CS_HIP(ctx, hipHostFree(p));
        p = nullptr, bytes = 0;
        const size_t want = total + total / 2 + 4096;
        CS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault));
        bytes = want;
        return CSTONE_OK;
    }
};

//! one cstone_hip_update_octree step (rebalance with the counts at hand, then recount) of a tree that grows as needed
template<class K>
int updateOctreeGrowing(cstone_hip_ctx* ctx, const void* keys, size_t n, uint32_t bucket, DevBuf& tree, DevBuf& counts,
                        int& cap, int& numLeaves, int* converged)
{
    while (true)
    {
        int leaves = numLeaves;
        int rc = cstone_hip_update_octree(ctx, 8 * sizeof(K), keys, n, bucket, tree.p, counts.as<uint32_t>(), &leaves, cap,
                                          0xFFFFFFFFu, converged);
        if (rc == CSTONE_OK) numLeaves = leaves;
        if (rc != CSTONE_E_CAPACITY) return rc;
        CS_TRY(ensureTree<K>(ctx, tree, counts, cap, leaves + 1));
    }
}

//! cstone_hip_compute_octree (from the root until converged) into a tree with room for `need` leaves that grows until
//! the result fits
template<class K>
int computeOctreeGrowing(cstone_hip_ctx* ctx, const void* keys, size_t n, uint32_t bucket, DevBuf& tree, DevBuf& counts,
                         int& cap, int need, int& numLeaves)
{
    while (true)
    {
        CS_TRY(ensureTree<K>(ctx, tree, counts, cap, need));
        int leaves = 0, iters = 0;
        int rc = cstone_hip_compute_octree(ctx, 8 * sizeof(K), keys, n, bucket, tree.p, counts.as<uint32_t>(), &leaves, cap,
                                           0xFFFFFFFFu, &iters);
        if (rc == CSTONE_OK) numLeaves = leaves;
        if (rc != CSTONE_E_CAPACITY) return rc;
        need = leaves + 1;
    }
}

/*! The host's copy of the GLOBAL tree -- leaves and (all-reduced) counts as the last sync read them back -- next to the
 *  device arrays `tree` / `counts` of capacity `cap` with `numLeaves` leaves, which stay with the Domain object. */
template<class K>
struct GlobalTreeHost
{
    std::vector<K> leaves;
    std::vector<uint32_t> counts;
    PinnedBlock pin; // where the read-backs of a sync arrive (the owner may take more room behind queueReadBack)

    //! the copies are those of a tree of numLeaves leaves: the host can make the update step
    bool matches(int numLeaves) const { return int(leaves.size()) == numLeaves + 1 && int(counts.size()) == numLeaves; }

    /*! globalTreeStepHost on the copies; a changed leaf array replaces `leaves`, is uploaded to `tree` (grown as needed)
     *  and sets numLeaves.  The counts of the new tree are the caller's to make.  *same: every node op was "keep". */
    int stepOnHost(cstone_hip_ctx* ctx, uint32_t bucket, DevBuf& tree, DevBuf& devCounts, int& cap, int& numLeaves,
                   bool* same)
    {
        std::vector<K> fresh;
        *same = globalTreeStepHost<K>(leaves, counts, bucket, fresh);
        if (*same) return CSTONE_OK;
        const int newLeaves = int(fresh.size()) - 1;
        CS_TRY(ensureTree<K>(ctx, tree, devCounts, cap, newLeaves + 1));
        leaves.swap(fresh);
        CS_TRY(cstone_hip_upload(ctx, tree.p, leaves.data(), leaves.size() * sizeof(K)));
        numLeaves = newLeaves;
        return CSTONE_OK;
    }

    //! the device's counts (and, when the device made it, the leaf array) on their way to the pinned block; not waited
    //! for.  extraPinnedBytes: room the caller takes from `pin` for read-backs of its own
    int queueReadBack(cstone_hip_ctx* ctx, const DevBuf& tree, const DevBuf& devCounts, int numLeaves, bool withLeaves,
                      size_t extraPinnedBytes)
    {
        CS_TRY(pin.reserve(ctx, size_t(numLeaves) * 4 + size_t(numLeaves + 1) * sizeof(K) + extraPinnedBytes));
        pinCounts_ = static_cast<uint32_t*>(pin.take(size_t(numLeaves) * 4));
        CS_TRY(copyToPinned(ctx, pinCounts_, devCounts.p, size_t(numLeaves) * 4));
        pinLeaves_ = nullptr;
        if (withLeaves)
        {
            pinLeaves_ = static_cast<K*>(pin.take(size_t(numLeaves + 1) * sizeof(K)));
            CS_TRY(copyToPinned(ctx, pinLeaves_, tree.p, size_t(numLeaves + 1) * sizeof(K)));
        }
        pinLeafCount_ = numLeaves;
        return CSTONE_OK;
    }
    //! behind a synchronisation of the stream: what was queued becomes the host's copy (nothing queued: nothing happens)
    void takeReadBack()
    {
        if (!pinCounts_) return;
        counts.assign(pinCounts_, pinCounts_ + pinLeafCount_);
        if (pinLeaves_) leaves.assign(pinLeaves_, pinLeaves_ + pinLeafCount_ + 1);
        pinCounts_ = nullptr, pinLeaves_ = nullptr;
    }

private:
    uint32_t* pinCounts_ = nullptr;
    K* pinLeaves_        = nullptr;
    int pinLeafCount_    = 0;
};

} // namespace cship
