// Device-resident orchestration of cstone::Domain::sync for ONE rank (R/domain/domain.hpp:196-243 and the pieces
// it drives: GlobalAssignment R/domain/assignment.hpp:39-205, FocusedOctree R/focus/octree_focus_mpi.hpp,
// CombinedUpdate::updateFocus R/focus/octree_focus.hpp:83-137, Halos R/halos/halos.hpp:128-222, layout
// R/domain/layout.hpp:150-165).  Everything stays in HBM; per sync the host reads back the bounding box (6 scalars),
// the number of valid particles and, per tree rebalance step, {changed flag, new leaf count}.
//
// Multi-rank operation (peers, MAC-driven focus resolution, treelet / particle / halo exchange over RCCL) is the next
// row to build; the object refuses num_ranks > 1 instead of silently running something else.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ctx.hpp"
#include "devbuf.hpp"
#include "device_keys.hpp"
#include "host_tree.hpp"
#include "resort.hpp"
#include "scan.hpp"

namespace cship
{

namespace
{

// ---- focus-tree rebalance decisions for all nodes (leaves and internal), R/focus/rebalance.hpp:50-88.
//      Single rank: the focus is the whole key range, so MAC flags never decide anything (inFringe / inFocus are
//      always true) and the decision reduces to counts.
template<class K>
__global__ __launch_bounds__(256) void focusOpsKernel(const K* __restrict__ prefixes,
                                                      const NodeIdx* __restrict__ childOffsets,
                                                      const NodeIdx* __restrict__ parents,
                                                      const uint32_t* __restrict__ counts, NodeIdx numNodes,
                                                      uint32_t bucket, NodeIdx* __restrict__ ops)
{
    NodeIdx i = blockIdx.x * 256 + threadIdx.x;
    if (i >= numNodes) return;
    int op = 1;
    if (i > 0 && counts[parents[(i - 1) / 8]] <= bucket) { op = 0; }
    else
    {
        unsigned level = prefixBits(prefixes[i]) / 3;
        if (childOffsets[i] == 0 && level < maxLevel<K>() && counts[i] > bucket) op = 8;
    }
    ops[i] = op;
}

// ---- R/focus/rebalance.hpp:113-184: a merged node inherits the op of its closest kept ancestor iff both start at
//      the same key; reads the ORIGINAL ops and writes a second array (the reference rewrites in place, race-free in
//      outcome).  changed |= 1 if any op != 1.
template<class K>
__global__ __launch_bounds__(256) void protectAncestorsKernel(const K* __restrict__ prefixes,
                                                              const NodeIdx* __restrict__ parents,
                                                              const NodeIdx* __restrict__ opsIn, NodeIdx numNodes,
                                                              NodeIdx* __restrict__ opsOut, int* __restrict__ changed)
{
    NodeIdx i = blockIdx.x * 256 + threadIdx.x;
    int op    = 1;
    if (i < numNodes)
    {
        if (i == 0) { op = opsIn[0]; }
        else
        {
            NodeIdx a = i;
            while (opsIn[a] == 0)
                a = parents[(a - 1) / 8];
            op = (fromPrefix(prefixes[i]) == fromPrefix(prefixes[a])) ? opsIn[a] : 0;
        }
        opsOut[i] = op;
    }
    // (set once: updates of tens of thousands of waves to one address serialise in the L2, reads of it do not)
    if (__any(op != 1) && (threadIdx.x & 63) == 0 && *reinterpret_cast<volatile int*>(changed) == 0) atomicOr(changed, 1);
}

//! leafOps[i] = ops[leafToInternal[numInternal + i]] for i < numLeaves, leafOps[numLeaves] = 0
__global__ __launch_bounds__(256) void leafOpsKernel(const NodeIdx* __restrict__ ops,
                                                     const NodeIdx* __restrict__ leafToInternal, NodeIdx numInternal,
                                                     NodeIdx numLeaves, uint32_t* __restrict__ leafOps)
{
    NodeIdx i = blockIdx.x * 256 + threadIdx.x;
    if (i < numLeaves) leafOps[i] = uint32_t(ops[leafToInternal[numInternal + i]]);
    else if (i == numLeaves) leafOps[i] = 0;
}

//! counts[leafToInternal[numInternal + i]] = leafCounts[i]
__global__ __launch_bounds__(256) void scatterLeafCountsKernel(const uint32_t* __restrict__ leafCounts,
                                                               const NodeIdx* __restrict__ leafToInternal,
                                                               NodeIdx numInternal, NodeIdx numLeaves,
                                                               uint32_t* __restrict__ counts)
{
    NodeIdx i = blockIdx.x * 256 + threadIdx.x;
    if (i < numLeaves) counts[leafToInternal[numInternal + i]] = leafCounts[i];
}

template<class K>
__global__ void countValidKernel(const K* __restrict__ keys, size_t n, int* __restrict__ out)
{
    // number of keys below the end of the curve = index of the first remove marker (keys are sorted)
    size_t lo = 0, len = n;
    while (len > 0)
    {
        size_t half = len >> 1;
        bool right  = keys[lo + half] < endKey<K>();
        lo          = right ? lo + half + 1 : lo;
        len         = right ? len - half - 1 : half;
    }
    out[0] = int(lo);
}

template<class K>
__global__ void initTreeKernel(K* tree, uint32_t* counts, uint32_t c0)
{
    tree[0]   = 0;
    tree[1]   = endKey<K>();
    counts[0] = c0;
}

} // namespace

struct DomainBase
{
    virtual ~DomainBase() = default;
    virtual int sync(void** keys, void** x, void** y, void** z, void** h, size_t n, void** scratch, int numScratch,
                     void** props, const int* propBytes, int numProps) = 0;
    virtual int view(cstone_hip_domain_view* out)        = 0;
    virtual void setHaloFactor(float factor)             = 0;
    virtual void setSortMode(int mode)                   = 0;
    virtual void setSpeculativeBox(bool on)              = 0;
    virtual int reapplySync(const void* in, size_t n, int elemBytes, void* out) = 0;
    virtual int updateExpansionCenters(const void* x, const void* y, const void* z, const void* m, int massBits) = 0;
    virtual int computeGravity(const void* x, const void* y, const void* z, const void* m, const void* h, int massBits,
                               int order, double G, double eps2, void* ax, void* ay, void* az, void* phi) = 0;
    virtual int adaptH(const void* x, const void* y, const void* z, void* h, uint32_t ng0, uint32_t tol, uint32_t maxIter,
                       float growLimit, uint32_t* counts, uint32_t* status) = 0;
    virtual int fof(const void* x, const void* y, const void* z, double linkingLength, uint32_t* labels,
                    uint32_t* groupSizes, uint32_t* numGroups) = 0;
    virtual int fofProperties(const void* x, const void* y, const void* z, const void* m, int massBits, const void* vx,
                              const void* vy, const void* vz, const uint32_t* groupOffsets, const uint32_t* members,
                              uint32_t numGroups, void* mass, void* center, void* velocity, void* radius,
                              uint32_t* flags) = 0;
    virtual int sphereProfiles(const void* x, const void* y, const void* z, const void* w, int massBits, const void* queryCenters,
                               const void* queryScale, uint32_t numQueries, const double* edgesHost, int numBins,
                               uint64_t* counts, double* sums, uint32_t* flags) = 0;
    virtual int knn(const void* x, const void* y, const void* z, const void* queryCenters, const void* queryRmax,
                    const uint32_t* querySelf, uint32_t numQueries, uint32_t k, uint32_t* neighbors, void* dist2,
                    uint32_t* counts) = 0;
    virtual int pairCounts(const void* x, const void* y, const void* z, const void* w, int wBits, const double* edgesHost,
                           int numBins, uint64_t* counts, double* sums, uint64_t* statsHost) = 0;
    virtual int pairCountsCross(const void* x, const void* y, const void* z, const void* w, int wBits, const void* queryCenters,
                                const void* queryW, uint32_t numQueries, const double* edgesHost, int numBins,
                                uint64_t* counts, double* sums, uint64_t* statsHost) = 0;
    virtual void stats(cstone_hip_domain_stats* out)     = 0;
};

template<class K, class T>
class DomainImpl final : public DomainBase
{
public:
    DomainImpl(cstone_hip_ctx* ctx, int curve, uint32_t bucket, uint32_t bucketFocus, float theta, const cstone_box& box)
        : ctx_(ctx)
        , curve_(curve)
        , bucket_(bucket)
        , bucketFocus_(bucketFocus)
        , theta_(theta)
        , box_(box)
    {
    }
    ~DomainImpl() override
    {
        if (pinnedLevels_) (void)hipHostFree(pinnedLevels_);
    }

    int sync(void** keysPP, void** xPP, void** yPP, void** zPP, void** hPP, size_t n, void** scratchAll, int numScratch,
             void** props, const int* propBytes, int numProps) override
    {
        if (n == 0) return fail(ctx_, CSTONE_E_ARG, "domain_sync: no particles");
        if (!firstCall_ && n != bufSize_)
            return fail(ctx_, CSTONE_E_ARG, "Domain sync: input array sizes are inconsistent (%zu != %u)", n, bufSize_);
        SyncState s{xPP, yPP, zPP, hPP, static_cast<K*>(*keysPP), n, scratchAll, numScratch, props, propBytes, numProps};
        const int rc = runStages(s);
        // a sync that failed behind a fork onto the tree stream joins it: nothing of this sync is in flight afterwards
        if (rc != CSTONE_OK && treeInFlight_)
        {
            (void)hipStreamSynchronize(ctx_->tree);
            treeInFlight_ = false;
        }
        // ... and one that failed between focusRebuild and the end of focusCounts (all particles removed, found at the
        // read-back of the re-sort; any CS_TRY of tryResort's tail, stepGlobalTree, joinTreeStream or focusCounts) holds
        // the new tree with the counts and the layout of the old one: the next sync starts both trees from the root, as
        // the first did
        if (rc != CSTONE_OK && s.rebuilt && !s.converged && !s.treeDone)
        {
            firstCall_    = true;
            layoutLeaves_ = -1;
            deepestBound_ = int(maxLevel<K>());
            levelRangeHost_.clear();
        }
        if (rc != CSTONE_OK) ctx_->sideBusy &= ~SIDE_TREE;
        return rc;
    }

private:
    struct SyncState;
    int runStages(SyncState& s)
    {
        CS_TRY(takeLevelRanges());
        // ---- GlobalAssignment::assign (assignment.hpp:57-103): box, keys, sort, one global-tree step
        CS_TRY(measureBoxFirst(s));
        CS_TRY(reserveSortBuffers(s));
        // The gather of x, y, z has no consumer inside a sync: with three or more scratch arrays it runs on the context's
        // second stream, next to the tree updates (chains of small, latency-bound kernels with two read-backs in between)
        // and the gather of h, and is joined before the call returns.
        s.noOverlap    = std::getenv("CSTONE_NO_GATHER_OVERLAP") != nullptr; // tuning / tests
        // (tuning / tests: the order on one stream.  A tree that the last sync left as it was is expected to stay: then
        //  there is nothing to hoist but the node ops, and those cost the encode more than they save -- the gather of
        //  x, y, z bounds such a sync, not the tree: extras.zero_motion)
        s.noHoist      = std::getenv("CSTONE_NO_TREE_HOIST") != nullptr || !treeChanged_;
        ctx_->sideBusy = 0; // (a sync that failed behind a fork may have left a bit set)
        CS_TRY(tryResort(s));
        resortedThisSync_ = s.sorted;
        CS_TRY(encodeSortCheckBox(s));
        CS_TRY(stepGlobalTree(s));
        CS_TRY(forkXyzGather(s, s.numAssigned)); // (radix path: the ordering is final from here on)
        // ---- GlobalAssignment::distribute on one rank: nothing to exchange; the second sort (assignment.hpp:156) of an
        //      already sorted range is the identity and is skipped.
        // ---- h goes into SFC order for the halo radii (domain.hpp:213-215): gathered further down, in the pass that
        //      takes the maximum per leaf
        CS_TRY(updateFocusTree(s));
        s.treeDone = true;
        CS_TRY(layoutAndHalos(s));
        CS_TRY(gatherFields(s));
        return finishSync(s); // (its synchronisation brings the global counts: a hoisted sync has none before it)
    }

public:
    void setHaloFactor(float factor) override { haloSearchExt_ = factor; }
    void setSortMode(int mode) override { sortMode_ = mode; }
    void setSpeculativeBox(bool on) override { speculativeBox_ = on; }
    // what the client chose (cstone_hip_domain_set_speculative_box); the environment variable of the experiments overrides
    // it.  Read at every sync (the multi-rank path reads it once, in its constructor)
    bool maySpeculate() const { return speculativeBox_ && std::getenv("CSTONE_NO_SPECULATIVE_BOX") == nullptr; }

    int view(cstone_hip_domain_view* v) override
    {
        v->start_index           = startIndex_;
        v->end_index             = endIndex_;
        v->num_particles_with_halos = bufSize_;
        v->box                   = box_;
        v->num_global_leaves     = gLeaves_;
        v->global_leaves         = gTree_.p;
        v->global_counts         = gCounts_.as<uint32_t>();
        v->num_focus_leaves      = fLeaves_;
        v->num_focus_nodes       = fLeaves_ + (fLeaves_ - 1) / 7;
        v->focus_leaves          = fTree_.p;
        v->focus_leaf_counts     = fLeafCounts_.as<uint32_t>();
        v->prefixes              = fPrefixes_.p;
        v->child_offsets         = fChild_.as<int32_t>();
        v->parents               = fParents_.as<int32_t>();
        v->level_range           = fLevelRange_.as<int32_t>();
        v->internal_to_leaf      = fItl_.as<int32_t>();
        v->leaf_to_internal      = fLti_.as<int32_t>();
        v->layout                = layout_.as<uint32_t>();
        v->centers               = fCenters_.p;
        v->sizes                 = fSizes_.p;
        v->halo_flags            = flags_.as<int32_t>();
        v->sfc_order             = order_.as<uint32_t>();
        v->halo_radii            = radii_.as<float>();
        v->expansion_centers     = haveExpansion_ ? fExpansion_.p : nullptr;
        return CSTONE_OK;
    }

    /*! cstone_hip_adapt_smoothing_lengths for [start_index, end_index) of the last sync on the focus tree of the view.
     *  On one rank every particle is here, so h may grow without limit: growLimit == 0 means INFINITY */
    int adaptH(const void* x, const void* y, const void* z, void* h, uint32_t ng0, uint32_t tol, uint32_t maxIter,
               float growLimit, uint32_t* counts, uint32_t* status) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_adapt_h: no sync yet");
        if (growLimit == 0.0f) growLimit = INFINITY;
        return cstone_hip_adapt_smoothing_lengths(ctx_, rb, x, y, z, h, startIndex_, endIndex_, &box_,
                                                  fChild_.as<int32_t>(), fItl_.as<int32_t>(), layout_.as<uint32_t>(),
                                                  fCenters_.p, fSizes_.p, ng0, tol, maxIter, growLimit, 0, nullptr, counts,
                                                  status);
    }

    //! cstone_hip_friends_of_friends for [start_index, end_index) of the last sync on the focus tree of the view
    int fof(const void* x, const void* y, const void* z, double linkingLength, uint32_t* labels, uint32_t* groupSizes,
            uint32_t* numGroups) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_fof: no sync yet");
        return cstone_hip_friends_of_friends(ctx_, rb, x, y, z, startIndex_, endIndex_, &box_, fChild_.as<int32_t>(),
                                             fItl_.as<int32_t>(), layout_.as<uint32_t>(), fCenters_.p, fSizes_.p,
                                             linkingLength, labels, groupSizes, numGroups);
    }

    //! cstone_hip_fof_group_properties with the box of the last sync
    int fofProperties(const void* x, const void* y, const void* z, const void* m, int massBits, const void* vx, const void* vy,
                      const void* vz, const uint32_t* groupOffsets, const uint32_t* members, uint32_t numGroups, void* mass,
                      void* center, void* velocity, void* radius, uint32_t* flags) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_fof_properties: no sync yet");
        return cstone_hip_fof_group_properties(ctx_, rb, massBits, x, y, z, m, vx, vy, vz, &box_, groupOffsets, members,
                                               numGroups, mass, center, velocity, radius, flags);
    }

    //! cstone_hip_sphere_profiles on the octree, the box and [start_index, end_index) of the last sync
    int sphereProfiles(const void* x, const void* y, const void* z, const void* w, int massBits, const void* queryCenters,
                       const void* queryScale, uint32_t numQueries, const double* edgesHost, int numBins, uint64_t* counts,
                       double* sums, uint32_t* flags) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_sphere_profiles: no sync yet");
        return cstone_hip_sphere_profiles(ctx_, rb, massBits, x, y, z, w, startIndex_, endIndex_, &box_, fChild_.as<int32_t>(),
                                          fItl_.as<int32_t>(), layout_.as<uint32_t>(), fCenters_.p, fSizes_.p, queryCenters,
                                          queryScale, numQueries, edgesHost, numBins, counts, sums, flags);
    }

    //! cstone_hip_knn on the octree, the box and [start_index, end_index) of the last sync
    int knn(const void* x, const void* y, const void* z, const void* queryCenters, const void* queryRmax,
            const uint32_t* querySelf, uint32_t numQueries, uint32_t k, uint32_t* neighbors, void* dist2,
            uint32_t* counts) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_knn: no sync yet");
        return cstone_hip_knn(ctx_, rb, x, y, z, startIndex_, endIndex_, &box_, fChild_.as<int32_t>(), fItl_.as<int32_t>(),
                              layout_.as<uint32_t>(), fCenters_.p, fSizes_.p, queryCenters, queryRmax, querySelf, numQueries,
                              k, neighbors, dist2, counts);
    }

    //! cstone_hip_pair_counts on the octree and the box of the last sync: targets [start_index, end_index), sources every
    //! particle on the rank
    int pairCounts(const void* x, const void* y, const void* z, const void* w, int wBits, const double* edgesHost, int numBins,
                   uint64_t* counts, double* sums, uint64_t* statsHost) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_pair_counts: no sync yet");
        return cstone_hip_pair_counts(ctx_, rb, wBits, x, y, z, w, 0, bufSize_, startIndex_, endIndex_, &box_,
                                      fChild_.as<int32_t>(), fItl_.as<int32_t>(), layout_.as<uint32_t>(), fCenters_.p, fSizes_.p,
                                      edgesHost, numBins, counts, sums, statsHost);
    }

    //! cstone_hip_pair_counts_cross on the octree, the box and [start_index, end_index) of the last sync
    int pairCountsCross(const void* x, const void* y, const void* z, const void* w, int wBits, const void* queryCenters,
                        const void* queryW, uint32_t numQueries, const double* edgesHost, int numBins, uint64_t* counts,
                        double* sums, uint64_t* statsHost) override
    {
        if (firstCall_ || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "domain_pair_counts_cross: no sync yet");
        return cstone_hip_pair_counts_cross(ctx_, rb, wBits, x, y, z, w, startIndex_, endIndex_, &box_, fChild_.as<int32_t>(),
                                            fItl_.as<int32_t>(), layout_.as<uint32_t>(), fCenters_.p, fSizes_.p, queryCenters,
                                            queryW, numQueries, edgesHost, numBins, counts, sums, statsHost);
    }

    /*! Domain::updateExpansionCenters (R/domain/domain.hpp:415-421) on one rank = FocusedOctree::updateCenters without its
     *  exchanges (octree_focus_mpi.hpp:369-449: computeLeafSourceCenter, upsweep with CombineSourceCenter) + setMac for
     *  1 / theta: (centre of mass, MAC radius^2) per node of the focus tree.  x, y, z, m: the arrays of the last sync's
     *  results (all of them are assigned on one rank), device */
    int updateExpansionCenters(const void* x, const void* y, const void* z, const void* m, int massBits) override
    {
        if (lastN_ == 0 || fLeaves_ < 1) return fail(ctx_, CSTONE_E_ARG, "update_expansion_centers: no sync yet");
        if ((massBits != 32 && massBits != 64) || !x || !y || !z || !m)
            return fail(ctx_, CSTONE_E_ARG, "update_expansion_centers: bad argument");
        const NodeIdx L = fLeaves_, I = (L - 1) / 7, M = L + I;
        CS_TRY(fExpansion_.ensure(ctx_, size_t(M) * 4 * sizeof(T)));
        CS_TRY(cstone_hip_leaf_source_centers(ctx_, 8 * sizeof(T), massBits, 8 * sizeof(T), x, y, z, m,
                                              fLti_.as<int32_t>() + I, L, layout_.as<uint32_t>(), fExpansion_.p));
        int32_t levels[maxLevel<K>() + 2];
        CS_TRY(copyToHost(ctx_, levels, fLevelRange_.p, sizeof levels)); // (which levels exist: synchronises the stream)
        CS_TRY(cstone_hip_upsweep_centers(ctx_, 8 * sizeof(T), int(maxLevel<K>()), levels, fChild_.as<int32_t>(),
                                          fExpansion_.p));
        CS_TRY(cstone_hip_set_mac(ctx_, curve_, 8 * sizeof(K), 8 * sizeof(T), fPrefixes_.p, M, fExpansion_.p, 1.0f / theta_,
                                  &box_));
        haveExpansion_ = true;
        return cstone_hip_ctx_sync(ctx_);
    }

    /*! Barnes-Hut gravity on the focus tree (csrc/gravity.hip): the multipoles about the current expansion centres, then
     *  the group walk over the end_index particles.  The target groups follow from the sync's tree and are kept until
     *  the next sync.  h: per-particle softening lengths laid out like x, or null.  order 3: the octupoles after the
     *  multipoles, and the walk that takes both. */
    int computeGravity(const void* x, const void* y, const void* z, const void* m, const void* h, int massBits,
                       int order, double G, double eps2, void* ax, void* ay, void* az, void* phi) override
    {
        if (!haveExpansion_)
            return fail(ctx_, CSTONE_E_ARG,
                        "domain_compute_gravity: no expansion centres (sync_grav or update_expansion_centers after the "
                        "last sync)");
        if (box_.bc[0] == 1 || box_.bc[1] == 1 || box_.bc[2] == 1)
            return fail(ctx_, CSTONE_E_ARG, "domain_compute_gravity: periodic boundaries need Ewald summation, which is "
                                            "not provided");
        if ((massBits != 32 && massBits != 64) || !x || !y || !z || !m || !ax || !ay || !az)
            return fail(ctx_, CSTONE_E_ARG, "domain_compute_gravity: bad argument");
        const NodeIdx L = fLeaves_, I = (L - 1) / 7, M = L + I;
        if (groupsSync_ != syncs_)
        {
            CS_TRY(groups_.ensure(ctx_, size_t(endIndex_ + 1) * sizeof(uint32_t)));
            uint32_t numGroups = 0;
            CS_TRY(cstone_hip_compute_group_splits(ctx_, kb, rb, 0, endIndex_, x, y, z, fTree_.p, L,
                                                   layout_.as<uint32_t>(), &box_, 64, CSTONE_GRAVITY_GROUP_TOL,
                                                   groups_.as<uint32_t>(), size_t(endIndex_) + 1, &numGroups));
            numGroups_  = numGroups;
            groupsSync_ = syncs_;
        }
        CS_TRY(fMultipoles_.ensure(ctx_, size_t(M) * 8 * sizeof(T)));
        int32_t levels[maxLevel<K>() + 2];
        CS_TRY(copyToHost(ctx_, levels, fLevelRange_.p, sizeof levels));
        CS_TRY(cstone_hip_upsweep_multipoles(ctx_, rb, massBits, x, y, z, m, fLti_.as<int32_t>() + I, L,
                                             layout_.as<uint32_t>(), int(maxLevel<K>()), levels, fChild_.as<int32_t>(),
                                             M, fExpansion_.p, fMultipoles_.p));
        if (order == 3)
        {
            CS_TRY(fOctupoles_.ensure(ctx_, size_t(M) * 8 * sizeof(T)));
            CS_TRY(cstone_hip_upsweep_octupoles(ctx_, rb, massBits, x, y, z, m, fLti_.as<int32_t>() + I, L,
                                                layout_.as<uint32_t>(), int(maxLevel<K>()), levels,
                                                fChild_.as<int32_t>(), M, fExpansion_.p, fMultipoles_.p, fOctupoles_.p));
            return cstone_hip_compute_gravity_o3(ctx_, rb, massBits, x, y, z, m, h, 0, endIndex_, groups_.as<uint32_t>(),
                                                 numGroups_, &box_, fChild_.as<int32_t>(), fItl_.as<int32_t>(),
                                                 layout_.as<uint32_t>(), fExpansion_.p, fMultipoles_.p, fOctupoles_.p, 0,
                                                 G, eps2, ax, ay, az, phi, nullptr, nullptr, nullptr);
        }
        return cstone_hip_compute_gravity_h(ctx_, rb, massBits, x, y, z, m, h, 0, endIndex_, groups_.as<uint32_t>(),
                                            numGroups_, &box_, fChild_.as<int32_t>(), fItl_.as<int32_t>(),
                                            layout_.as<uint32_t>(), fExpansion_.p, fMultipoles_.p, order, G, eps2, ax,
                                            ay, az, phi, nullptr, nullptr);
    }

    /*! Domain::reapplySync (R/domain/domain.hpp:334-378) without an exchange: the kept particles in SFC order */
    int reapplySync(const void* in, size_t n, int elemBytes, void* out) override
    {
        if (lastN_ == 0) return fail(ctx_, CSTONE_E_ARG, "reapply_sync: no sync yet");
        if (n != lastN_)
            return fail(ctx_, CSTONE_E_ARG, "reapply_sync: array of %zu elements, the last sync took %zu", n, lastN_);
        if (!in || !out || in == out) return fail(ctx_, CSTONE_E_ARG, "reapply_sync: bad array");
        return cstone_hip_gather(ctx_, elemBytes, order_.as<uint32_t>(), endIndex_, in, out);
    }

    void stats(cstone_hip_domain_stats* out) override
    {
        out->syncs               = syncs_;
        out->resorts             = uint32_t(resorts_);
        out->resort_fallbacks    = uint32_t(resortFallbacks_);
        out->box_redos           = uint32_t(boxRedos_);
        out->full_sort_fallbacks = uint32_t(fullSortFallbacks_);
        out->last_movers         = lastMovers_;
    }

    float haloSearchExt_ = 1.0f;

private:
    uint32_t syncs_ = 0, lastMovers_ = 0;
    size_t lastN_ = 0; // input size of the last sync
    int boxRedos_ = 0; // syncs whose speculative keys had to be recomputed because the box changed
    bool measureFirst_ = false; // the last box was not the one before it: measure the extents before encoding
    int sortMode_        = CSTONE_SORT_INCREMENTAL;
    bool speculativeBox_ = true;
    static constexpr int kb = 8 * sizeof(K), rb = 8 * sizeof(T);

    //! What the stages of one sync share: the caller's arrays (they change places with the scratch arrays as the fields
    //! move) and what the stages before have decided.  Made by sync() on its stack.
    struct SyncState
    {
        void **xPP, **yPP, **zPP, **hPP;
        K* keys;
        size_t n;
        void** scratch; // [0]: the buffer the single-scratch rotation works with
        int numScratch;
        void** props;
        const int* propBytes;
        int numProps;
        bool speculate      = false; // the keys are computed with the box of the previous sync, the same pass measures
        bool boxMoved       = false; // measured first and found a new box: every key changes, nothing to re-sort from
        int startPass       = 0;     // low digit passes the radix sort leaves to the fix-up
        size_t sortTmpBytes = 0;
        bool sorted         = false; // the re-sort has put keys and order_ into their final order
        uint32_t resortMarkers = 0;  // particles with the remove marker, as the re-sort counted them
        bool noOverlap      = false; // CSTONE_NO_GATHER_OVERLAP
        bool xyzForked = false, xyzJoined = false; // the gather of x, y, z on the second stream
        bool noHoist        = false; // CSTONE_NO_TREE_HOIST
        // what the host has read of the node ops it queued on the tree stream (takeFocusOps):
        int converged       = 0;     //     every node op is "keep"
        NodeIdx newL        = 0;     //     leaves of the rebalanced tree
        bool treeDone       = false; // the focus tree, its links and its counts are those of this sync
        bool rebuilt        = false; // focusRebuild is done or on its way on the tree stream: focusCounts is what is left
        uint32_t numAssigned = 0;    // particles without the remove marker
    };

    T* extentsDev() const { return reinterpret_cast<T*>(ctx_->devScalars + 16); }
    T* extentsHost() const { return reinterpret_cast<T*>(ctx_->hostScalars + 16); }

    //! the level ranges of the linked octree the last sync (re)built travelled to a pinned block behind its last
    //! kernels; that sync ended with a synchronisation of the stream, so they are here now
    int takeLevelRanges()
    {
        if (!levelsPending_) return CSTONE_OK;
        CS_HIP(ctx_, hipStreamSynchronize(ctx_->stream)); // (idle unless the last sync failed half way)
        levelRangeHost_.assign(pinnedLevels_, pinnedLevels_ + maxLevel<K>() + 2);
        const int deepest = deepestLevel<K>(levelRangeHost_);
        if (deepest > deepestBound_)
            return fail(ctx_, CSTONE_E_INTERNAL, "domain_sync: the focus tree has level %d, the bound was %d", deepest,
                        deepestBound_);
        deepestBound_  = deepest;
        levelsPending_ = false;
        return CSTONE_OK;
    }

    /*! The box of a sync follows from the extents of x, y, z (makeGlobalBox + limitBoxShrinking).  After the first call
     *  it rarely changes, so the keys are computed SPECULATIVELY with the box of the previous sync while the same pass
     *  over x, y, z measures the extents; the box rule is evaluated afterwards and only a box that really changed costs a
     *  second encode + sort.  Saves the separate 2.4 GB pass over the coordinates per sync at 1e8.
     *  Decides s.speculate; a sync that does not speculate measures here and sets box_, s.boxMoved and measureFirst_. */
    int measureBoxFirst(SyncState& s)
    {
        const bool anyOpen = box_.bc[0] != 1 || box_.bc[1] != 1 || box_.bc[2] != 1;
        // (adaptive: a sync whose speculation failed -- the outermost particles of an open box move -- makes the following
        //  syncs measure first, until one of them finds the box unchanged again)
        s.speculate = anyOpen && !firstCall_ && !measureFirst_ && maySpeculate();
        if (!anyOpen || s.speculate) return CSTONE_OK;
        // extents of the open dimensions in one launch and one read-back (MinMaxGpu x3 in the reference)
        const void* open[3];
        int dims[3], numOpen = 0;
        void* coords[3] = {*s.xPP, *s.yPP, *s.zPP};
        for (int d = 0; d < 3; ++d)
            if (box_.bc[d] != 1) open[numOpen] = coords[d], dims[numOpen++] = d;
        double ext[6], lim[6] = {};
        CS_TRY(minMaxCoordinates(ctx_, rb, open, numOpen, s.n, ext));
        for (int i = 0; i < numOpen; ++i)
            lim[2 * dims[i]] = ext[2 * i], lim[2 * dims[i] + 1] = ext[2 * i + 1];
        const cstone_box before = box_;
        box_                    = limitBoxShrinking<T>(before, lim, firstCall_);
        s.boxMoved              = !sameLimits(box_, before);
        if (!firstCall_) measureFirst_ = s.boxMoved;
        return CSTONE_OK;
    }

    //! buffers of the sort, and which digits need the radix passes (partialSortStartPass); a run that turns out longer
    //! than the fix-up takes (the particles have clustered since) raises the flag stepGlobalTree reads back
    int reserveSortBuffers(SyncState& s)
    {
        CS_TRY(order_.ensure(ctx_, s.n * sizeof(uint32_t)));
        CS_TRY(orderAlt_.ensure(ctx_, s.n * sizeof(uint32_t)));
        CS_TRY(keysAlt_.ensure(ctx_, s.n * sizeof(K)));
        s.sortTmpBytes = cstone_hip_sort_pairs_temp_bytes(kb, s.n);
        CS_TRY(sortTmp_.ensure(ctx_, s.sortTmpBytes));
        // (the deepest level: of the tree the last sync left behind, exact; the multi-rank path takes the same value
        //  from its own pinned block)
        if (!firstCall_ && !levelRangeHost_.empty() && !allDigits(sortMode_))
            s.startPass = partialSortStartPass<K>(deepestLevel<K>(levelRangeHost_), bucketFocus_);
        return CSTONE_OK;
    }

    //! computeSfcKeys + setMapFromCodes (assignment.hpp:81-86) in one call: the sort's digits are counted while the keys
    //! are still in the encode kernel's registers, its first pass produces the positions instead of reading an iota
    int encodeAndSort(SyncState& s, bool measure, bool* measured)
    {
        CS_TRY(sfcKeysAndOrderingHint(ctx_, curve_, kb, rb, *s.xPP, *s.yPP, *s.zPP, s.keys, order_.as<uint32_t>(), s.n,
                                      box_, keysAlt_.p, orderAlt_.as<uint32_t>(), sortTmp_.p, s.sortTmpBytes, s.startPass,
                                      ctx_->devScalars + 3, true, measure ? extentsDev() : nullptr, measured));
        if (s.startPass == 0) CS_HIP(ctx_, hipMemsetAsync(ctx_->devScalars + 3, 0, sizeof(int), ctx_->stream));
        return CSTONE_OK;
    }

    //! x, y, z change places with the first three scratch arrays
    void swapFieldsWithScratch(SyncState& s)
    {
        std::swap(*s.xPP, s.scratch[0]);
        std::swap(*s.yPP, s.scratch[1]);
        std::swap(*s.zPP, s.scratch[2]);
    }

    //! the gather of x, y, z for the first `count` entries of order_ starts on the second stream (once per sync, and only
    //! with three scratch arrays); the caller's pointers name the new arrays from here on
    int forkXyzGather(SyncState& s, size_t count)
    {
        if (s.numScratch < 3 || s.noOverlap || s.xyzForked || count == 0) return CSTONE_OK;
        CS_TRY(ensureAuxStream(ctx_));
        CS_HIP(ctx_, hipEventRecord(ctx_->evFork, ctx_->stream));
        CS_HIP(ctx_, hipStreamWaitEvent(ctx_->aux, ctx_->evFork, 0));
        const void* src[3] = {*s.xPP, *s.yPP, *s.zPP};
        void* dst[3]       = {s.scratch[0], s.scratch[1], s.scratch[2]};
        int rc;
        {
            StreamScope scope(ctx_, ctx_->aux);
            rc = cstone_hip_gather_multi(ctx_, sizeof(T), order_.as<uint32_t>(), count, src, dst, 3);
        }
        CS_TRY(rc);
        CS_HIP(ctx_, hipEventRecord(ctx_->evJoin, ctx_->aux));
        ctx_->sideBusy |= SIDE_AUX;
        swapFieldsWithScratch(s);
        s.xyzForked = true;
        return CSTONE_OK;
    }
    //! the main stream waits for that gather (once)
    int joinXyzGather(SyncState& s)
    {
        if (s.xyzForked && !s.xyzJoined) CS_HIP(ctx_, hipStreamWaitEvent(ctx_->stream, ctx_->evJoin, 0));
        s.xyzJoined = true;
        ctx_->sideBusy &= ~SIDE_AUX;
        return CSTONE_OK;
    }

    /*! The incremental re-sort (resort.hpp): particles that are still inside the leaf their position belonged to at the
     *  previous sync are ordered leaf by leaf, the others are binned into their new leaves.  Same result as the sort of
     *  all keys; a box that changed, too many movers or an overfull leaf take the regular path.
     *  Result: s.sorted (keys and order_ are final; x, y, z are then on their way),
     *  s.resortMarkers, and s.speculate -- switched off when the attempt has read the extents back and failed, with
     *  box_ being the box this sync needs from then on.  One read-back. */
    int tryResort(SyncState& s)
    {
        const int tileLeaves = LeafResort<K>::leavesPerTile(bucketFocus_);
        const bool attempt   = !firstCall_ && tileLeaves > 0 && layoutLeaves_ == fLeaves_ && fLeaves_ > 0 &&
                             resortBackoff_ == 0 && !s.boxMoved && mayResort(sortMode_);
        if (resortBackoff_ > 0) --resortBackoff_;
        if (!attempt) return CSTONE_OK;
        if (!s.noHoist) CS_TRY(ensureTreeStream(ctx_));
        CS_TRY(resort_.prepare(ctx_, fTree_.as<K>(), layout_.as<uint32_t>(), fLeaves_, s.n, keysAlt_.as<K>(), true));
        // (fillCompactLeavesKernel was the last reader of the old tree on this stream: the tree stream starts here)
        if (!s.noHoist) CS_HIP(ctx_, hipEventRecord(ctx_->evTreeFork, ctx_->stream));
        const ResortArgs<K> ra = resort_.args();
        bool done              = false;
        CS_TRY(computeKeysResort(ctx_, curve_, kb, rb, *s.xPP, *s.yPP, *s.zPP, s.keys, s.n, box_, &ra,
                                 s.speculate ? extentsDev() : nullptr, &done));
        if (!done) return CSTONE_OK;
        CS_TRY(resort_.binMovers(ctx_, tileLeaves));
        // one read-back: the extents (slots 16..27) and what the re-sort found (28..31)
        CS_TRY(copyToPinned(ctx_, ctx_->hostScalars + 16, ctx_->devScalars + 16, 16 * sizeof(int)));
        // The device is busy with the encode and the mover bins from here on, and the host has nothing more to queue
        // before it has seen what they found.  The structural half of the focus-tree update follows from the tree and the counts of
        // the previous sync alone, and whatever becomes of the re-sort, this sync needs it: the node ops go to the tree
        // stream now (not before the encode is queued: the idle device would wait for the host), the host takes their result
        // and queues the rebalance and the linked octree behind them -- all of it beside the encode.
        if (!s.noHoist)
        {
            CS_TRY(forkFocusOps());
            CS_TRY(takeFocusOps(s));
            CS_TRY(forkFocusRebuild(s));
        }
        CS_HIP(ctx_, hipStreamSynchronize(ctx_->stream));
        cstone_box next = box_;
        if (s.speculate)
        {
            double ext[6];
            for (int k = 0; k < 6; ++k)
                ext[k] = double(extentsHost()[k]);
            next = limitBoxShrinking<T>(box_, ext, firstCall_);
        }
        const bool boxChanged = !sameLimits(next, box_);
        const int* found      = ctx_->hostScalars + RESORT_SCALARS;
        const uint32_t markers = uint32_t(found[0]), J = uint32_t(found[2]), movers = uint32_t(found[3]);
        const int flags        = found[1];
        s.resortMarkers        = markers;
        if (!boxChanged && resortAccepted(flags, movers, s.n))
        {
            // (stepGlobalTree would find this too, further down: no leaf pass, gather or tree step for nothing.  With
            //  the rebuild on its way already, sync() puts the domain back to its first-call state)
            if (s.rebuilt && markers >= s.n) return fail(ctx_, CSTONE_E_ARG, "domain_sync: all particles removed");
            CS_TRY(resort_.sortLeaves(ctx_, keysAlt_.as<K>(), s.keys, order_.as<uint32_t>(), movers, markers, J,
                                      tileLeaves, (flags & RESORT_LARGE_QUIET_TILES) != 0));
            CS_TRY(forkXyzGather(s, s.n - markers)); // (the ordering is final: x, y, z follow on the second stream)
            CS_HIP(ctx_, hipMemsetAsync(ctx_->devScalars + 3, 0, sizeof(int), ctx_->stream));
            s.sorted    = true;
            lastMovers_ = movers;
            ++resorts_;
            return CSTONE_OK;
        }
        // the caller's key array has not been touched: the regular path starts from scratch, with the box this sync
        // needs (the extents are known by now)
        // (the radix sort is next: it takes its large tiles again once the tree stream is joined -- it finished long ago)
        if (s.rebuilt) CS_TRY(joinTreeStream());
        if (boxChanged) { adoptChangedBox(next); }
        else
        {
            resortBackoff_ = RESORT_BACKOFF_SYNCS;
            ++resortFallbacks_; // (the multi-rank path backs off alike and keeps no such count)
        }
        s.speculate = false;
        return CSTONE_OK;
    }

    //! the speculation failed: `next` is the box of this sync, and the following syncs measure first
    void adoptChangedBox(const cstone_box& next)
    {
        box_ = next;
        ++boxRedos_;
        measureFirst_ = true;
    }

    //! the regular path of a sync that was not re-sorted: encode + radix sort, then the check of a speculated box -- a
    //! box that changed costs a second encode + sort
    int encodeSortCheckBox(SyncState& s)
    {
        if (s.sorted) return CSTONE_OK;
        bool measured = false;
        CS_TRY(encodeAndSort(s, s.speculate, &measured));
        if (!s.speculate) return CSTONE_OK;
        double lim[6];
        if (measured)
        {
            CS_TRY(copyToPinned(ctx_, extentsHost(), extentsDev(), 6 * sizeof(T)));
            CS_HIP(ctx_, hipStreamSynchronize(ctx_->stream));
            for (int k = 0; k < 6; ++k)
                lim[k] = double(extentsHost()[k]);
        }
        else
        {
            // unaligned arrays: the plain encode ran, measure the extents the regular way
            const void* all[3] = {*s.xPP, *s.yPP, *s.zPP};
            CS_TRY(minMaxCoordinates(ctx_, rb, all, 3, s.n, lim));
        }
        const cstone_box next = limitBoxShrinking<T>(box_, lim, firstCall_);
        if (sameLimits(next, box_)) return CSTONE_OK;
        // the particles have left the box (or shrunk away from it by more than 5 %): keys and order again
        adoptChangedBox(next);
        // the key array is sorted by now: put every entry back to its particle first (the remove markers of the
        // caller must meet their own particles again), then encode with the new box
        CS_TRY(cstone_hip_scatter(ctx_, sizeof(K), order_.as<uint32_t>(), s.n, s.keys, keysAlt_.p));
        CS_HIP(ctx_, hipMemcpyAsync(s.keys, keysAlt_.p, s.n * sizeof(K), hipMemcpyDeviceToDevice, ctx_->stream));
        return encodeAndSort(s, false, nullptr);
    }

    //! one update step of the global tree (on the first call: until it converges) and s.numAssigned
    int stepGlobalTree(SyncState& s)
    {
        if (firstCall_)
        {
            // spanning tree of one rank = the root; counts = bucket - 1 (assignment.hpp:48-53)
            CS_TRY(ensureTree<K>(ctx_, gTree_, gCounts_, gCap_, 4096));
            hipLaunchKernelGGL(initTreeKernel<K>, 1, 1, 0, ctx_->stream, gTree_.as<K>(), gCounts_.as<uint32_t>(),
                               bucket_ - 1);
            gLeaves_ = 1;
        }
        // A sync that was re-sorted knows its number of valid particles already, and the host holds the (small) global tree
        // and its counts from the last sync: the update step of the global tree is then made on the HOST
        // (globalTreeStepHost), the device only counts, and the counts travel back with the read-back of the focus-tree
        // update -- one stream synchronisation and a handful of launches fewer than cstone_hip_update_octree.
        if (s.sorted && !firstCall_ && hostGlobalStep_ && gHost_.matches(gLeaves_))
        {
            s.numAssigned = uint32_t(s.n) - s.resortMarkers;
            if (s.numAssigned == 0) return fail(ctx_, CSTONE_E_ARG, "domain_sync: all particles removed");
            bool same;
            CS_TRY(gHost_.stepOnHost(ctx_, bucket_, gTree_, gCounts_, gCap_, gLeaves_, &same));
            CS_TRY(cstone_hip_compute_node_counts(ctx_, kb, gTree_.p, gCounts_.as<uint32_t>(), gLeaves_, s.keys, s.n,
                                                  0xFFFFFFFFu));
            return gHost_.queueReadBack(ctx_, gTree_, gCounts_, gLeaves_, false, 256);
        }
        // particles flagged with the remove marker sort behind the end of the curve and leave the domain: their number
        // is on its way to the host while the global tree is updated (whose own read-back completes the stream)
        hipLaunchKernelGGL(countValidKernel<K>, 1, 1, 0, ctx_->stream, s.keys, s.n, ctx_->devScalars + 2);
        CS_TRY(copyToPinned(ctx_, ctx_->hostScalars + 2, ctx_->devScalars + 2, 2 * sizeof(int)));
        // updateOctreeGlobal on one rank (tree/update_mpi.hpp:71-94): rebalance with the previous counts, then recount
        int converged = 0;
        CS_TRY(updateOctreeGrowing<K>(ctx_, s.keys, s.n, bucket_, gTree_, gCounts_, gCap_, gLeaves_, &converged));
        if (firstCall_)
        {
            // `while (!updateOctreeGlobal(...));` (assignment.hpp:95-98): at least one more step, whatever the first said
            int guard = 0;
            do
            {
                CS_TRY(updateOctreeGrowing<K>(ctx_, s.keys, s.n, bucket_, gTree_, gCounts_, gCap_, gLeaves_, &converged));
                if (++guard > 64) return fail(ctx_, CSTONE_E_INTERNAL, "global tree does not converge");
            } while (!converged);
        }
        // the copy was queued ahead of the update's own read-back (update_octree synchronises for the new leaf count)
        s.numAssigned = uint32_t(ctx_->hostScalars[2]);
        if (s.numAssigned == 0) return fail(ctx_, CSTONE_E_ARG, "domain_sync: all particles removed");
        if (ctx_->hostScalars[3] != 0)
        {
            // a run of equal high digits was too long for the fix-up: sort the rest the regular way.  (The global tree
            // above is not affected: its leaf boundaries cannot fall inside such a run.)
            CS_TRY(cstone_hip_sort_pairs(ctx_, kb, s.keys, order_.as<uint32_t>(), s.n, keysAlt_.p, orderAlt_.as<uint32_t>(),
                                         sortTmp_.p, s.sortTmpBytes));
            ++fullSortFallbacks_;
        }
        // (tree and counts for the host's copy: they arrive behind the next synchronisation of the stream)
        return gHost_.queueReadBack(ctx_, gTree_, gCounts_, gLeaves_, true, 256);
    }

    //! focus tree (octree_focus_mpi.hpp:535-553 on first call, then :225-227)
    int updateFocusTree(SyncState& s)
    {
        int conv = 0;
        if (firstCall_)
        {
            CS_TRY(ensureTree<K>(ctx_, fTree_, fLeafCounts_, fCap_, 4096));
            hipLaunchKernelGGL(initTreeKernel<K>, 1, 1, 0, ctx_->stream, fTree_.as<K>(), fLeafCounts_.as<uint32_t>(),
                               bucketFocus_ + 1);
            fLeaves_ = 1;
            CS_TRY(buildFocusOctree());
            // counts_ of the single root node = bucketFocus + 1 (octree_focus_mpi.hpp:75)
            CS_TRY(fCounts_.ensure(ctx_, sizeof(uint32_t)));
            CS_HIP(ctx_, hipMemcpyAsync(fCounts_.p, fLeafCounts_.p, sizeof(uint32_t), hipMemcpyDeviceToDevice,
                                        ctx_->stream));
            int guard = 0;
            while (!conv)
            {
                CS_TRY(updateFocus(s.keys, s.numAssigned, &conv));
                if (++guard > 64) return fail(ctx_, CSTONE_E_INTERNAL, "focus tree does not converge");
            }
        }
        if (s.rebuilt)
        {
            // the re-sorted sync: the structure is on its way on the tree stream, the counts follow it on this one
            CS_TRY(joinTreeStream());
            return focusCounts(s.keys, s.numAssigned, s.converged);
        }
        return updateFocus(s.keys, s.numAssigned, &conv);
    }

    //! focusOps of this sync on the tree stream, behind the leaf-table prepare of the main stream (evTreeFork stands
    //! behind its fillCompactLeavesKernel, the last reader of the old tree)
    int forkFocusOps()
    {
        CS_HIP(ctx_, hipStreamWaitEvent(ctx_->tree, ctx_->evTreeFork, 0));
        int rc;
        {
            StreamScope scope(ctx_, ctx_->tree, true);
            treeInFlight_ = true;
            rc            = focusOps();
        }
        CS_TRY(rc);
        CS_HIP(ctx_, hipEventRecord(ctx_->evTreeJoin, ctx_->tree));
        return CSTONE_OK;
    }
    //! the host waits for the node ops on the tree stream and reads {changed, new leaf count}
    int takeFocusOps(SyncState& s)
    {
        CS_HIP(ctx_, hipEventSynchronize(ctx_->evTreeJoin));
        treeInFlight_ = false;
        return readFocusOps(&s.converged, &s.newL);
    }
    //! focusRebuild on the tree stream (the host knows the new leaf count), behind the node ops and with them behind the
    //! last reader of the old tree on the main stream.  An unchanged tree has nothing to rebuild
    int forkFocusRebuild(SyncState& s)
    {
        s.rebuilt = true;
        if (s.converged) return CSTONE_OK;
        ctx_->sideBusy |= SIDE_TREE; // (the node-key sort takes its 256-lane tiles beside the encode or the leaf pass)
        int rc;
        {
            StreamScope scope(ctx_, ctx_->tree, true);
            treeInFlight_ = true;
            rc            = focusRebuild(s.converged, s.newL);
        }
        CS_TRY(rc);
        CS_HIP(ctx_, hipEventRecord(ctx_->evTreeJoin, ctx_->tree));
        return CSTONE_OK;
    }
    //! the main stream waits for the tree stream (the pinned level ranges included: they are written there)
    int joinTreeStream()
    {
        if (treeInFlight_) CS_HIP(ctx_, hipStreamWaitEvent(ctx_->stream, ctx_->evTreeJoin, 0));
        treeInFlight_ = false;
        ctx_->sideBusy &= ~SIDE_TREE;
        return CSTONE_OK;
    }

    //! Halos::discover + computeLayout (halos.hpp:128-222) for the assignment [0, L); h goes into SFC order on the way
    int layoutAndHalos(SyncState& s)
    {
        const NodeIdx L = fLeaves_;
        CS_TRY(layout_.ensure(ctx_, size_t(L + 1) * sizeof(uint32_t)));
        CS_TRY(radii_.ensure(ctx_, size_t(L) * sizeof(float)));
        CS_TRY(flags_.ensure(ctx_, size_t(L) * sizeof(int)));
        CS_HIP(ctx_, hipMemsetAsync(layout_.p, 0, sizeof(uint32_t), ctx_->stream));
        CS_TRY(cstone_hip_inclusive_scan_u32(ctx_, fLeafCounts_.as<uint32_t>(), layout_.as<uint32_t>() + 1, size_t(L)));
        layoutLeaves_ = L;
        // gatherArrays(h) + segmentMax + scale in one pass over h (every leaf is assigned on one rank: the leaves' particles
        // are all the assigned particles)
        // where h goes: the first scratch array -- unless x, y, z are still on their way there on the second stream; a
        // fourth scratch array then takes h (no waiting), with three the gather of h waits for them
        void** hDst = s.scratch;
        if (s.xyzForked && s.numScratch >= 4) { hDst = &s.scratch[3]; }
        else { CS_TRY(joinXyzGather(s)); }
        CS_TRY(gatherWithHaloRadii(ctx_, rb, *s.hPP, order_.as<uint32_t>(), *hDst, layout_.as<uint32_t>(), L,
                                   haloSearchExt_, radii_.as<float>()));
        std::swap(*s.hPP, *hDst);
        CS_HIP(ctx_, hipMemsetAsync(flags_.p, 0, size_t(L) * sizeof(int), ctx_->stream));
        // one rank: every leaf is assigned, no halo leaves: layout = exclusive scan of the leaf counts (layout.hpp:150-165),
        // which is the inclusive scan written above shifted by one.
        CS_TRY(cstone_hip_find_halos(ctx_, curve_, kb, rb, fPrefixes_.p, fChild_.as<int32_t>(), fItl_.as<int32_t>(),
                                     fTree_.p, radii_.as<float>(), &box_, 0, L, flags_.as<int32_t>()));
        return CSTONE_OK;
    }

    //! updateLayout (domain.hpp:542-604): keys already sit at offset 0; gather the unordered arrays
    int gatherFields(SyncState& s)
    {
        CS_TRY(joinXyzGather(s)); // (the property gathers below go through the buffers x, y, z were read from)
        if (s.xyzForked) {} // (x, y, z went on the second stream)
        else if (s.numScratch >= 3)
        {
            // three free buffers (the caller's scratch tuple, R/domain/domain.hpp:196-206 has three as well): x, y, z go
            // to their new order in ONE pass that reads the ordering once
            const void* src[3] = {*s.xPP, *s.yPP, *s.zPP};
            void* dst[3]       = {s.scratch[0], s.scratch[1], s.scratch[2]};
            CS_TRY(cstone_hip_gather_multi(ctx_, sizeof(T), order_.as<uint32_t>(), s.numAssigned, src, dst, 3));
            swapFieldsWithScratch(s);
        }
        else
        {
            void** arrays[3] = {s.xPP, s.yPP, s.zPP};
            for (auto a : arrays)
            {
                CS_TRY(cstone_hip_gather(ctx_, sizeof(T), order_.as<uint32_t>(), s.numAssigned, *a, *s.scratch));
                std::swap(*a, *s.scratch);
            }
        }
        for (int p = 0; p < s.numProps; ++p)
        {
            if (s.propBytes[p] > int(sizeof(T)))
                return fail(ctx_, CSTONE_E_ARG, "domain_sync: property %d is wider than the scratch element", p);
            CS_TRY(cstone_hip_gather(ctx_, s.propBytes[p], order_.as<uint32_t>(), s.numAssigned, s.props[p], *s.scratch));
            std::swap(s.props[p], *s.scratch);
        }
        return CSTONE_OK;
    }

    //! bookkeeping of a completed sync, and the sticky device-side error word (look-back spin bail-out of the sort,
    //! traversal stack overflow ...): a sync that tripped one of those checks must not report success
    int finishSync(const SyncState& s)
    {
        startIndex_ = 0;
        endIndex_   = s.numAssigned;
        lastN_      = s.n;
        haveExpansion_ = false; // (the tree and the particles' order may have changed)
        bufSize_    = s.numAssigned;
        ++syncs_;
        firstCall_  = false;
#ifdef CSTONE_TEST_HOOKS // (tests: CSTONE_FORCE_DEVICE_ERROR raises the error word)
        if (std::getenv("CSTONE_FORCE_DEVICE_ERROR")) CS_HIP(ctx_, hipMemsetAsync(ctx_->devScalars + 63, 1, 1, ctx_->stream));
#endif
        const int rc = cstone_hip_ctx_sync(ctx_);
        // (the stream has been synchronised: the global counts stepGlobalTree queued are here)
        if (rc != CSTONE_E_HIP) gHost_.takeReadBack();
        return rc;
    }
    int buildFocusOctree()
    {
        const NodeIdx L = fLeaves_, M = L + (L - 1) / 7;
        CS_TRY(fPrefixes_.ensure(ctx_, size_t(M) * sizeof(K)));
        CS_TRY(fChild_.ensure(ctx_, size_t(M + 1) * sizeof(NodeIdx)));
        CS_TRY(fParents_.ensure(ctx_, size_t(std::max(1, (M - 1) / 8)) * sizeof(NodeIdx)));
        CS_TRY(fLevelRange_.ensure(ctx_, (maxLevel<K>() + 2) * sizeof(NodeIdx)));
        CS_TRY(fItl_.ensure(ctx_, size_t(M) * sizeof(NodeIdx)));
        CS_TRY(fLti_.ensure(ctx_, size_t(M) * sizeof(NodeIdx)));
        // a focus update refines by one level at most: the leaves of the new tree are no deeper than the deepest of the
        // tree before + 1.  deepestBound_ is exact at the start of a sync (above) and grows by one per rebuild inside it.
        const int deepest = std::min(int(maxLevel<K>()), deepestBound_ + 1);
        CS_TRY(buildLinkedOctree(ctx_, 8 * sizeof(K), fTree_.p, L, fPrefixes_.p, fChild_.as<int32_t>(),
                                 fParents_.as<int32_t>(), fLevelRange_.as<int32_t>(), fItl_.as<int32_t>(),
                                 fLti_.as<int32_t>(), deepest));
        deepestBound_ = deepest;
        // the exact level ranges go to a pinned block WITHOUT waiting for them: the upsweep of this sync launches the
        // levels up to the bound (one of them may be empty), the next sync reads the block
        if (!pinnedLevels_)
            CS_HIP(ctx_, hipHostMalloc(reinterpret_cast<void**>(&pinnedLevels_), 32 * sizeof(NodeIdx), hipHostMallocDefault));
        CS_TRY(copyToPinned(ctx_, pinnedLevels_, fLevelRange_.p, (maxLevel<K>() + 2) * sizeof(NodeIdx)));
        levelsPending_ = true;
        return CSTONE_OK;
    }

    /*! one FocusedOctree::updateTree + updateCounts + updateGeoCenters step on one rank
     *  (octree_focus_mpi.hpp:108-187,205-273; octree_focus.hpp:83-137; rebalance.hpp:50-184), cut where the data
     *  dependencies are: focusOps and focusRebuild need the tree, its links and its counts as the previous sync left
     *  them, only focusCounts needs this sync's keys (and box).  All three queue on ctx_->stream. */
    int updateFocus(const K* keys, size_t n, int* converged)
    {
        CS_TRY(focusOps());
        CS_HIP(ctx_, hipStreamSynchronize(ctx_->stream));
        NodeIdx newL = 0;
        CS_TRY(readFocusOps(converged, &newL));
        CS_TRY(focusRebuild(*converged, newL));
        return focusCounts(keys, n, *converged);
    }

    //! node ops from the counts at hand, their scan over the leaves, {changed, new leaf count} on the way to the host; no wait
    int focusOps()
    {
        const NodeIdx L = fLeaves_, I = (L - 1) / 7, M = L + I;
        CS_TRY(ops_.ensure(ctx_, size_t(M + 1) * sizeof(NodeIdx)));
        CS_TRY(ops2_.ensure(ctx_, size_t(M + 1) * sizeof(NodeIdx)));
        CS_TRY(leafOps_.ensure(ctx_, size_t(L + 1) * sizeof(uint32_t)));
        int* scalars = ctx_->devScalars + FOCUS_SCALARS;
        CS_HIP(ctx_, hipMemsetAsync(scalars, 0, 2 * sizeof(int), ctx_->stream));
        hipLaunchKernelGGL(focusOpsKernel<K>, gridFor(M, 256), 256, 0, ctx_->stream, fPrefixes_.as<K>(),
                           fChild_.as<NodeIdx>(), fParents_.as<NodeIdx>(), fCounts_.as<uint32_t>(), M, bucketFocus_,
                           ops_.as<NodeIdx>());
        // enforceKeys({focusStart, focusEnd}) is a no-op for the keys 0 and 2^(3 maxLevel) (rebalance.hpp:205)
        hipLaunchKernelGGL(protectAncestorsKernel<K>, gridFor(M, 256), 256, 0, ctx_->stream, fPrefixes_.as<K>(),
                           fParents_.as<NodeIdx>(), ops_.as<NodeIdx>(), M, ops2_.as<NodeIdx>(), scalars);
        hipLaunchKernelGGL(leafOpsKernel, gridFor(L + 1, 256), 256, 0, ctx_->stream, ops2_.as<NodeIdx>(),
                           fLti_.as<NodeIdx>(), I, L, leafOps_.as<uint32_t>());
        CS_TRY(arenaReserve(ctx_, scanArenaBytes(size_t(L) + 1)));
        int rc = scanU32(ctx_, leafOps_.as<uint32_t>(), leafOps_.as<uint32_t>(), size_t(L) + 1, 0u, false,
                         (uint32_t*)scalars + 1);
        arenaReset(ctx_);
        CS_TRY(rc);
        return copyToPinned(ctx_, ctx_->hostScalars + FOCUS_SCALARS, scalars, 2 * sizeof(int));
    }

    //! behind a wait for focusOps
    int readFocusOps(int* converged, NodeIdx* newL)
    {
        *converged = ctx_->hostScalars[FOCUS_SCALARS] == 0;
        *newL      = ctx_->hostScalars[FOCUS_SCALARS + 1];
        if (*newL < 1) return fail(ctx_, CSTONE_E_INTERNAL, "focus rebalance produced %d leaves", *newL);
        return CSTONE_OK;
    }

    //! a tree that changed: the rebalanced leaf array and its linked octree; fLeaves_ = newL from here on
    int focusRebuild(int converged, NodeIdx newL)
    {
        // every node op is "keep" -- the leaf array and with it the linked octree are what they were; the reference
        // rebuilds them regardless (octree_focus.hpp:121-134) because it parks its temporaries in the tree's own arrays
        if (converged) return CSTONE_OK;
        const NodeIdx L = fLeaves_;
        CS_TRY(newTree_.ensure(ctx_, size_t(newL + 1) * sizeof(K)));
        CS_TRY(cstone_hip_rebalance_tree(ctx_, 8 * sizeof(K), fTree_.p, L, newL, leafOps_.as<int32_t>(), newTree_.p));
        // the new leaf array BECOMES the tree (the two buffers change places; the counts are made anew in focusCounts).
        // It used to be copied back: 18 MB at 10^8 particles, a blit with a handful of waves that got next to nothing
        // of the memory system while the gather of x, y, z ran on the second stream -- 0.62 ms during which the
        // rest of the tree update waited (profiles/r04: the copy ended with the gather)
        std::swap(fTree_.p, newTree_.p);
        std::swap(fTree_.bytes, newTree_.bytes);
        CS_TRY(fLeafCounts_.ensure(ctx_, size_t(newL) * sizeof(uint32_t)));
        fCap_    = int(std::min(fTree_.bytes / sizeof(K) - 1, fLeafCounts_.bytes / sizeof(uint32_t)));
        fLeaves_ = newL;
        return buildFocusOctree();
    }

    //! updateCounts: leaf counts from the particle keys, scattered to the linked layout, summed bottom-up; then the
    //! geometric centres, which need the box this sync ends with
    int focusCounts(const K* keys, size_t n, int converged)
    {
        const NodeIdx newL = fLeaves_, newI = (newL - 1) / 7, newM = newL + newI;
        treeChanged_       = !converged;
        // the leaf boundaries of an unchanged tree are searched from where they were at the previous sync (layout_)
        const uint32_t* guess = (converged && layoutLeaves_ == newL) ? layout_.as<uint32_t>() : nullptr;
        // a sync that was re-sorted knows where the particles of every old leaf went: a boundary that an old leaf had
        // already is looked up, any other is searched inside one old leaf (resort.hip, countLeaves)
        if (resortedThisSync_)
            CS_TRY(resort_.countLeaves(ctx_, fTree_.as<K>(), newL, keys, 0xFFFFFFFFu, fLeafCounts_.as<uint32_t>()));
        else
            CS_TRY(cstone_hip_compute_node_counts_guided(ctx_, 8 * sizeof(K), fTree_.p, fLeafCounts_.as<uint32_t>(), newL,
                                                         keys, n, 0xFFFFFFFFu, guess));
        CS_TRY(fCounts_.ensure(ctx_, size_t(newM) * sizeof(uint32_t)));
        hipLaunchKernelGGL(scatterLeafCountsKernel, gridFor(newL, 256), 256, 0, ctx_->stream,
                           fLeafCounts_.as<uint32_t>(), fLti_.as<NodeIdx>(), newI, newL, fCounts_.as<uint32_t>());
        CS_TRY(cstone_hip_upsweep_sum_bounded(ctx_, int(maxLevel<K>()) + 2, fLevelRange_.as<int32_t>(),
                                              fChild_.as<int32_t>(), fCounts_.as<uint32_t>(), deepestBound_));
        // updateGeoCenters: the geometry of the nodes follows from the tree and the box alone -- nothing to do for an
        // unchanged tree inside an unchanged box (the reference recomputes it in every sync, octree_focus_mpi.hpp:259-273)
        const bool sameBox = centersNodes_ == newM && sameLimits(centersBox_, box_);
        if (!(converged && sameBox))
        {
            CS_TRY(fCenters_.ensure(ctx_, size_t(newM) * 3 * sizeof(T)));
            CS_TRY(fSizes_.ensure(ctx_, size_t(newM) * 3 * sizeof(T)));
            CS_TRY(cstone_hip_node_centers(ctx_, curve_, 8 * sizeof(K), 8 * sizeof(T), fPrefixes_.p, newM, &box_,
                                           fCenters_.p, fSizes_.p));
            centersBox_   = box_;
            centersNodes_ = newM;
        }
        CS_HIP(ctx_, hipGetLastError());
        return CSTONE_OK;
    }

    cstone_hip_ctx* ctx_;
    int curve_;
    uint32_t bucket_, bucketFocus_;
    float theta_;
    cstone_box box_;
    bool firstCall_ = true;
    uint32_t startIndex_ = 0, endIndex_ = 0, bufSize_ = 0;

    DevBuf order_, orderAlt_, keysAlt_, sortTmp_;
    LeafResort<K> resort_;
    int resortBackoff_ = 0, resorts_ = 0, resortFallbacks_ = 0;
    bool resortedThisSync_ = false;
    DevBuf gTree_, gCounts_;
    int gCap_ = 0, gLeaves_ = 0;
    GlobalTreeHost<K> gHost_; // host copies of the global tree and its counts (the host makes its update step)
    bool hostGlobalStep_ = std::getenv("CSTONE_DEVICE_GLOBAL_STEP") == nullptr; // (tests: the device-side step)
    DevBuf fTree_, fLeafCounts_, fCounts_, newTree_;
    int fCap_ = 0, fLeaves_ = 0;
    int layoutLeaves_ = -1; // number of leaves layout_ was computed for
    cstone_box centersBox_{}; // box and node count fCenters_ / fSizes_ were computed for
    NodeIdx centersNodes_ = -1;
    std::vector<NodeIdx> levelRangeHost_; // of the tree the LAST sync left behind (exact)
    NodeIdx* pinnedLevels_ = nullptr;     // where the level ranges of a rebuilt tree arrive
    bool levelsPending_    = false;
    bool treeChanged_      = true;  // the last focus update rebuilt the tree
    bool treeInFlight_     = false; // work of this sync is queued on the tree stream and not joined yet
    int deepestBound_      = int(maxLevel<K>()); // no leaf of the current focus tree is deeper
    int fullSortFallbacks_ = 0;
    DevBuf fPrefixes_, fChild_, fParents_, fLevelRange_, fItl_, fLti_, fCenters_, fSizes_;
    DevBuf fExpansion_;          // T[M][4]: centre of mass + MAC radius^2 per node (updateExpansionCenters)
    bool haveExpansion_ = false; // ... of the tree of the last sync
    DevBuf fMultipoles_;         // T[M][8]: multipoles about the expansion centres (computeGravity)
    DevBuf fOctupoles_;          // T[M][8]: octupoles about them (computeGravity at order 3 only)
    DevBuf groups_;              // u32[numGroups_ + 1]: target groups of computeGravity, from the sync number groupsSync_
    uint32_t numGroups_ = 0, groupsSync_ = 0;
    DevBuf ops_, ops2_, leafOps_, layout_, radii_, flags_;
};

} // namespace cship

using namespace cship;

struct cstone_hip_domain
{
    cstone_hip_ctx* ctx;
    std::unique_ptr<DomainBase> impl;
};

extern "C"
{

int cstone_hip_domain_create(cstone_hip_ctx* ctx, cstone_hip_domain** out, int curve, int key_bits, int real_bits,
                             int rank, int num_ranks, uint32_t bucket_size, uint32_t bucket_size_focus, float theta,
                             const cstone_box* box_host)
{
    if (!ctx || !out || !box_host) return fail(ctx, CSTONE_E_ARG, "domain_create: bad argument");
    *out = nullptr;
    if (bucket_size < bucket_size_focus)
        return fail(ctx, CSTONE_E_ARG,
                    "The bucket size of the global tree must not be smaller than the bucket size of the focused tree");
    if (num_ranks != 1 || rank != 0)
        return fail(ctx, CSTONE_E_ARG, "domain_create: only single-rank domains are implemented in this round");
    if (curve != CSTONE_MORTON && curve != CSTONE_HILBERT) return fail(ctx, CSTONE_E_ARG, "domain_create: bad curve");
    auto* d = new cstone_hip_domain{ctx, nullptr};
    if (key_bits == 32 && real_bits == 32)
        d->impl.reset(new DomainImpl<uint32_t, float>(ctx, curve, bucket_size, bucket_size_focus, theta, *box_host));
    else if (key_bits == 32 && real_bits == 64)
        d->impl.reset(new DomainImpl<uint32_t, double>(ctx, curve, bucket_size, bucket_size_focus, theta, *box_host));
    else if (key_bits == 64 && real_bits == 32)
        d->impl.reset(new DomainImpl<uint64_t, float>(ctx, curve, bucket_size, bucket_size_focus, theta, *box_host));
    else if (key_bits == 64 && real_bits == 64)
        d->impl.reset(new DomainImpl<uint64_t, double>(ctx, curve, bucket_size, bucket_size_focus, theta, *box_host));
    else
    {
        delete d;
        return fail(ctx, CSTONE_E_ARG, "domain_create: unsupported key/real width");
    }
    *out = d;
    return CSTONE_OK;
}

int cstone_hip_domain_destroy(cstone_hip_domain* dom)
{
    if (!dom) return CSTONE_E_ARG;
    // (a domain outliving its context -- a client tearing down in the wrong order: the object and its device buffers are
    //  still released, the dead context is not touched, the caller learns about it)
    const bool alive = ctxAlive(dom->ctx);
    if (alive) (void)hipStreamSynchronize(dom->ctx->stream);
    else (void)hipDeviceSynchronize();
    delete dom;
    return alive ? CSTONE_OK : CSTONE_E_ARG;
}

int cstone_hip_domain_sync(cstone_hip_domain* dom, void** keys, void** x, void** y, void** z, void** h, size_t n,
                           void** scratch, void** props, const int* prop_bytes, int num_props)
{
    if (!dom || !keys || !x || !y || !z || !h || !scratch || !*keys || !*x || !*y || !*z || !*h || !*scratch ||
        num_props < 0 || (num_props && (!props || !prop_bytes)))
        return fail(dom ? dom->ctx : nullptr, CSTONE_E_ARG, "domain_sync: bad argument");
    return dom->impl->sync(keys, x, y, z, h, n, scratch, 1, props, prop_bytes, num_props);
}

int cstone_hip_domain_sync_scratch(cstone_hip_domain* dom, void** keys, void** x, void** y, void** z, void** h, size_t n,
                                   void** scratch, int num_scratch, void** props, const int* prop_bytes, int num_props)
{
    if (!dom || !keys || !x || !y || !z || !h || !scratch || !*keys || !*x || !*y || !*z || !*h || num_scratch < 1 ||
        num_props < 0 || (num_props && (!props || !prop_bytes)))
        return fail(dom ? dom->ctx : nullptr, CSTONE_E_ARG, "domain_sync: bad argument");
    for (int q = 0; q < num_scratch; ++q)
        if (!scratch[q]) return fail(dom->ctx, CSTONE_E_ARG, "domain_sync: null scratch buffer %d", q);
    return dom->impl->sync(keys, x, y, z, h, n, scratch, num_scratch, props, prop_bytes, num_props);
}

int cstone_hip_domain_update_expansion_centers(cstone_hip_domain* dom, const void* x, const void* y, const void* z,
                                               const void* m, int mass_bits)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->updateExpansionCenters(x, y, z, m, mass_bits);
}

int cstone_hip_domain_sync_grav(cstone_hip_domain* dom, void** keys, void** x, void** y, void** z, void** h, void** m,
                                int mass_bits, size_t n, void** scratch, int num_scratch, void** props,
                                const int* prop_bytes, int num_props)
{
    if (!dom || !m || !*m || (mass_bits != 32 && mass_bits != 64) || num_props < 0 || (num_props && (!props || !prop_bytes)))
        return fail(dom ? dom->ctx : nullptr, CSTONE_E_ARG, "domain_sync_grav: bad argument");
    // the masses follow their particles as one more property behind the caller's
    std::vector<void*> pp(props, props + num_props);
    std::vector<int> pb(prop_bytes, prop_bytes + num_props);
    pp.push_back(*m);
    pb.push_back(mass_bits / 8);
    int rc = cstone_hip_domain_sync_scratch(dom, keys, x, y, z, h, n, scratch, num_scratch, pp.data(), pb.data(),
                                            num_props + 1);
    for (int q = 0; q < num_props; ++q)
        props[q] = pp[q];
    *m = pp[num_props];
    if (rc != CSTONE_OK) return rc;
    return dom->impl->updateExpansionCenters(*x, *y, *z, *m, mass_bits);
}

int cstone_hip_domain_compute_gravity(cstone_hip_domain* dom, const void* x, const void* y, const void* z,
                                      const void* m, int mass_bits, int order, double G, double eps2, void* ax, void* ay,
                                      void* az, void* phi)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->computeGravity(x, y, z, m, nullptr, mass_bits, order, G, eps2, ax, ay, az, phi);
}

int cstone_hip_domain_compute_gravity_h(cstone_hip_domain* dom, const void* x, const void* y, const void* z,
                                        const void* m, const void* h, int mass_bits, int order, double G, double eps2,
                                        void* ax, void* ay, void* az, void* phi)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->computeGravity(x, y, z, m, h, mass_bits, order, G, eps2, ax, ay, az, phi);
}

int cstone_hip_domain_adapt_h(cstone_hip_domain* dom, const void* x, const void* y, const void* z, void* h, uint32_t ng0,
                              uint32_t tol, uint32_t max_iter, float grow_limit, uint32_t* counts, uint32_t* status)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->adaptH(x, y, z, h, ng0, tol, max_iter, grow_limit, counts, status);
}

int cstone_hip_domain_fof(cstone_hip_domain* dom, const void* x, const void* y, const void* z, double linking_length,
                          uint32_t* labels, uint32_t* group_sizes, uint32_t* num_groups)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->fof(x, y, z, linking_length, labels, group_sizes, num_groups);
}

int cstone_hip_domain_fof_properties(cstone_hip_domain* dom, const void* x, const void* y, const void* z, const void* m,
                                     int mass_bits, const void* vx, const void* vy, const void* vz,
                                     const uint32_t* group_offsets, const uint32_t* members, uint32_t num_groups, void* mass,
                                     void* center, void* velocity, void* radius, uint32_t* flags)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->fofProperties(x, y, z, m, mass_bits, vx, vy, vz, group_offsets, members, num_groups, mass, center,
                                    velocity, radius, flags);
}

int cstone_hip_domain_sphere_profiles(cstone_hip_domain* dom, const void* x, const void* y, const void* z, const void* w,
                                      int mass_bits, const void* query_centers, const void* query_scale,
                                      uint32_t num_queries, const double* edges_host, int num_bins, uint64_t* counts,
                                      double* sums, uint32_t* flags)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->sphereProfiles(x, y, z, w, mass_bits, query_centers, query_scale, num_queries, edges_host, num_bins,
                                     counts, sums, flags);
}

int cstone_hip_domain_knn(cstone_hip_domain* dom, const void* x, const void* y, const void* z, const void* query_centers,
                          const void* query_rmax, const uint32_t* query_self, uint32_t num_queries, uint32_t k,
                          uint32_t* neighbors, void* dist2, uint32_t* counts)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->knn(x, y, z, query_centers, query_rmax, query_self, num_queries, k, neighbors, dist2, counts);
}

int cstone_hip_domain_pair_counts(cstone_hip_domain* dom, const void* x, const void* y, const void* z, const void* w,
                                  int w_bits, const double* edges_host, int num_bins, uint64_t* counts, double* sums,
                                  uint64_t* stats_host)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->pairCounts(x, y, z, w, w_bits, edges_host, num_bins, counts, sums, stats_host);
}

int cstone_hip_domain_pair_counts_cross(cstone_hip_domain* dom, const void* x, const void* y, const void* z, const void* w,
                                        int w_bits, const void* query_centers, const void* query_w, uint32_t num_queries,
                                        const double* edges_host, int num_bins, uint64_t* counts, double* sums,
                                        uint64_t* stats_host)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->pairCountsCross(x, y, z, w, w_bits, query_centers, query_w, num_queries, edges_host, num_bins, counts,
                                      sums, stats_host);
}

int cstone_hip_domain_view_get(cstone_hip_domain* dom, cstone_hip_domain_view* out)
{
    if (!dom || !out) return CSTONE_E_ARG;
    return dom->impl->view(out);
}

int cstone_hip_domain_stats_get(cstone_hip_domain* dom, cstone_hip_domain_stats* out)
{
    if (!dom || !out) return CSTONE_E_ARG;
    dom->impl->stats(out);
    return CSTONE_OK;
}

int cstone_hip_domain_reapply_sync(cstone_hip_domain* dom, const void* in, size_t n, int elem_bytes, void* out)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->reapplySync(in, n, elem_bytes, out);
}

int cstone_hip_domain_set_halo_factor(cstone_hip_domain* dom, float factor)
{
    if (!dom || !(factor > 0.0f)) return CSTONE_E_ARG;
    dom->impl->setHaloFactor(factor);
    return CSTONE_OK;
}

int cstone_hip_domain_set_sort_mode(cstone_hip_domain* dom, int mode)
{
    if (!dom || mode < CSTONE_SORT_INCREMENTAL || mode > CSTONE_SORT_ALL_DIGITS) return CSTONE_E_ARG;
    dom->impl->setSortMode(mode);
    return CSTONE_OK;
}

int cstone_hip_domain_set_speculative_box(cstone_hip_domain* dom, int on)
{
    if (!dom) return CSTONE_E_ARG;
    dom->impl->setSpeculativeBox(on != 0);
    return CSTONE_OK;
}

int cstone_hip_test_hooks(void)
{
#ifdef CSTONE_TEST_HOOKS
    return 1;
#else
    return 0;
#endif
}

} // extern "C"
