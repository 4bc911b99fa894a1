// cstone::Domain::sync on SEVERAL ranks, one process per GPU (R/domain/domain.hpp:196-243).  Decomposition logic and
// all device work live here; the three collectives come from the host application through cstone_hip_comm_ops.
//
//   C1  global box            makeGlobalBox (R/sfc/box_mpi.hpp:85-121): local min/max, all_reduce(MIN) of (lo, -hi)
//   C2  global tree           GlobalAssignment (R/domain/assignment.hpp:42-103): updateOctreeGlobal = rebalance + recount +
//                             all_reduce(SUM) (R/tree/update_mpi.hpp:71-94); uniformBins / makeSfcAssignment /
//                             limitBoundaryShifts (R/domain/domaindecomp.hpp:50-172)
//   C3  particle exchange     createSendRanges (:218-230) on the sorted keys; the fields are NOT reordered first
//                             (assignment.hpp:121-127): ONE all_to_all_v of (x,y,z,h) rows; newcomers are merged into the
//                             kept, already sorted range instead of the second full sort of assignment.hpp:156
//   C4  halo discovery        on the locally essential tree (let.hpp) or on the owner's side
//   C5  halo exchange         ONE all_to_all_v of packed rows
// The stages of a sync, with their collectives and read-backs: DESIGN.md section 2c.
// Result: [halos of lower ranks | assigned, SFC sorted | halos of higher ranks] in domain-owned arrays.
// Box, SFC ranges, global tree and the assigned particles are bit-identical to the reference Domain under MPI
// (tests/golden/ref_domain_mpi_*.npz); the halo set is compared there as well.
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <memory>
#include <numeric>
#include <vector>

#include "ctx.hpp"
#include "devbuf.hpp"
#include "device_keys.hpp"
#include "fof_mr.hpp"
#include "fof_props.hpp"
#include "knn.hpp"
#include "pair_counts.hpp"
#include "sphere.hpp"
#include "host_tree.hpp"
#include "let.hpp"
#include "resort.hpp"
#include "scan.hpp"

namespace cship
{

namespace
{

// ---- host-side decomposition rules -------------------------------------------------------------------------------

//! smallest l with 8^l >= n (R/sfc/common.hpp:134-142)
inline unsigned log8ceilHost(uint64_t n)
{
    unsigned l = 0;
    uint64_t p = 1;
    while (p < n)
    {
        p *= 8;
        ++l;
    }
    return l;
}

//! computeSpanningTree(initialDomainSplits(numRanks, level)) (R/tree/csarray.hpp:508-531, domaindecomp.hpp:242-255):
//! per segment the canonical cover by maximal aligned power-of-8 nodes (spanSfcRange, R/sfc/common.hpp:376-438)
template<class K>
void appendCover(std::vector<K>& out, uint64_t a, uint64_t b)
{
    const uint64_t end = uint64_t(endKey<K>());
    while (a < b)
    {
        uint64_t size = end;
        while (size > 1 && (a % size != 0 || size > b - a))
            size /= 8;
        out.push_back(K(a));
        a += size;
    }
}

template<class K>
std::vector<K> initialGlobalTree(int numRanks)
{
    const uint64_t end   = uint64_t(endKey<K>());
    const unsigned level = log8ceilHost(100ull * uint64_t(numRanks));
    const unsigned shift = 3 * (maxLevel<K>() - level);
    const uint64_t delta = end / uint64_t(numRanks);
    std::vector<uint64_t> splits(numRanks + 1, 0);
    for (int i = 1; i < numRanks; ++i)
        splits[i] = ((uint64_t(i) * delta) >> shift) << shift;
    splits[numRanks] = end;
    std::vector<K> tree;
    for (int i = 0; i < numRanks; ++i)
        appendCover(tree, splits[i], splits[i + 1]);
    tree.push_back(K(end));
    return tree;
}

//! uniformBins (R/domain/domaindecomp.hpp:50-75)
inline std::vector<int> uniformBinsHost(const std::vector<uint32_t>& counts, int numBins)
{
    std::vector<uint64_t> scan(counts.size() + 1, 0);
    for (size_t i = 0; i < counts.size(); ++i)
        scan[i + 1] = scan[i] + counts[i];
    double binCount = double(scan.back()) / numBins;
    std::vector<int> bins(numBins + 1, 0);
    bins[numBins] = int(counts.size());
    for (int i = 1; i < numBins; ++i)
    {
        uint64_t target = uint64_t(i * binCount);
        bins[i]         = int(std::lower_bound(scan.begin(), scan.end(), target) - scan.begin());
    }
    return bins;
}

// ---- device helpers ------------------------------------------------------------------------------------------------

//! for each of two keys: the index of the leaf that contains it and that leaf's start and end key (one thread per key);
//! out[3 q] = index, out[3 q + 1] = start, out[3 q + 2] = end.  A key at or behind the end of the curve gives index L.
template<class K>
__global__ void containingLeavesKernel(const K* __restrict__ tree, int numLeaves, K key0, K key1,
                                       uint64_t* __restrict__ out)
{
    const int q = threadIdx.x;
    if (q > 1) return;
    const K key = q == 0 ? key0 : key1;
    int lo = 0, hi = numLeaves + 1; // first entry of tree[0 .. L] greater than key
    while (lo < hi)
    {
        int mid = (lo + hi) >> 1;
        if (tree[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    const int idx  = lo - 1; // tree[0] = 0 <= key: idx >= 0; key >= tree[L]: idx = L
    out[3 * q]     = uint64_t(idx);
    out[3 * q + 1] = uint64_t(tree[idx]);
    out[3 * q + 2] = idx < numLeaves ? uint64_t(tree[idx + 1]) : uint64_t(tree[idx]);
}


//! counts[i] = max(counts[i], local[i]): a wrapped 32-bit sum over the ranks cannot make a full node look empty
//! (R/tree/update_mpi.hpp:60-64)
__global__ __launch_bounds__(256) void maxWithLocalKernel(uint32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ local, int n)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) counts[i] = max(counts[i], local[i]);
}

//! rows[i] = {x, y, z, h}[idx[i]]: the fields of a particle travel as one record
template<class T>
__global__ __launch_bounds__(256) void packRowsKernel(const uint32_t* __restrict__ idx, size_t m,
                                                      const T* __restrict__ x, const T* __restrict__ y,
                                                      const T* __restrict__ z, const T* __restrict__ h,
                                                      T* __restrict__ rows)
{
    size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= m) return;
    uint32_t j      = idx[i];
    rows[4 * i]     = x[j];
    rows[4 * i + 1] = y[j];
    rows[4 * i + 2] = z[j];
    rows[4 * i + 3] = h[j];
}

template<class T>
__global__ __launch_bounds__(256) void unpackRowsKernel(const T* __restrict__ rows, size_t m, T* __restrict__ x,
                                                        T* __restrict__ y, T* __restrict__ z, T* __restrict__ h)
{
    size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= m) return;
    x[i] = rows[4 * i];
    y[i] = rows[4 * i + 1];
    z[i] = rows[4 * i + 2];
    h[i] = rows[4 * i + 3];
}

/*! the cut points of an assignment in the sorted keys and what follows from them, in one launch (it used to be a search,
 *  a difference and an upload): cut[p] = first key >= assignment[p] for p <= P, send[p] = cut[p + 1] - cut[p] for
 *  p < P (this rank's row of the count matrix) and send[P] = the rank's status word.  A lane searches both ends of its
 *  range itself: nothing to wait for */
template<class K>
__global__ void cutPointsKernel(const K* __restrict__ keys, size_t n, const K* __restrict__ assignment, int P,
                                uint64_t* __restrict__ cut, uint64_t* __restrict__ send, uint64_t status)
{
    auto firstNotBelow = [&](K v)
    {
        size_t lo = 0, len = n;
        while (len > 0)
        {
            size_t half = len / 2;
            if (keys[lo + half] < v) lo += half + 1, len -= half + 1;
            else len = half;
        }
        return uint64_t(lo);
    };
    int p = blockIdx.x * 64 + threadIdx.x;
    if (p > P) return;
    uint64_t mine = firstNotBelow(assignment[p]);
    cut[p]        = mine;
    if (p < P) send[p] = firstNotBelow(assignment[p + 1]) - mine;
    else send[P] = status;
}

//! keys (already sorted) and x, y, z, h (from their input slots order[i]) of the kept particles to their final slots
//! (pos[i], or i when pos is null): the two index maps are read once for the columns of a launch.  WHICH = 0: all five
//! columns; 1: keys and h (what the locally essential tree and the halo discovery need); 2: x, y, z (nobody reads them
//! before the halo exchange: they go out on the context's second stream, next to the tree update)
constexpr int PLACE_PER = 4; // elements per lane, strided by the workgroup: all index loads, then all field loads in flight
template<class K, class T, int WHICH>
__global__ __launch_bounds__(256) void placeColumnsKernel(const uint32_t* __restrict__ order,
                                                          const uint32_t* __restrict__ pos, size_t m,
                                                          const K* __restrict__ keys, const T* __restrict__ x,
                                                          const T* __restrict__ y, const T* __restrict__ z,
                                                          const T* __restrict__ h, K* __restrict__ dk,
                                                          T* __restrict__ dx, T* __restrict__ dy, T* __restrict__ dz,
                                                          T* __restrict__ dh)
{
    // (one element per lane -- three dependent loads in flight -- ran at 0.54 of the HBM peak where gatherMultiKernel, four
    //  elements per lane, reaches 0.71 on the same bytes)
    const size_t base = size_t(blockIdx.x) * (256 * PLACE_PER) + threadIdx.x;
    uint32_t s[PLACE_PER];
    size_t d[PLACE_PER];
    bool ok[PLACE_PER];
#pragma unroll
    for (int k = 0; k < PLACE_PER; ++k)
    {
        const size_t i = base + size_t(k) * 256;
        ok[k]          = i < m;
        s[k]           = ok[k] ? order[i] : 0u;
        d[k]           = (pos && ok[k]) ? size_t(pos[i]) : i;
    }
    if constexpr (WHICH != 2)
    {
        K vk[PLACE_PER];
        T vh[PLACE_PER];
#pragma unroll
        for (int k = 0; k < PLACE_PER; ++k)
            if (ok[k]) vk[k] = keys[base + size_t(k) * 256], vh[k] = h[s[k]]; // the kept keys are already in sorted order
#pragma unroll
        for (int k = 0; k < PLACE_PER; ++k)
            if (ok[k]) dk[d[k]] = vk[k], dh[d[k]] = vh[k];
    }
    if constexpr (WHICH != 1)
    {
        T vx[PLACE_PER], vy[PLACE_PER], vz[PLACE_PER];
#pragma unroll
        for (int k = 0; k < PLACE_PER; ++k)
            if (ok[k]) vx[k] = x[s[k]], vy[k] = y[s[k]], vz[k] = z[s[k]];
#pragma unroll
        for (int k = 0; k < PLACE_PER; ++k)
            if (ok[k]) dx[d[k]] = vx[k], dy[d[k]] = vy[k], dz[d[k]] = vz[k];
    }
}

__global__ __launch_bounds__(256) void boxFlagsKernel(const int32_t* __restrict__ boxes, int n,
                                                      uint32_t* __restrict__ flags)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = boxes[8 * i + 6] != 0;
}

//! keeps the records with flag != 0; scan = exclusive scan of the flags
__global__ __launch_bounds__(256) void compactBoxesKernel(const int32_t* __restrict__ boxes,
                                                          const uint32_t* __restrict__ scan, int n, int owner,
                                                          int32_t* __restrict__ out)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || boxes[8 * i + 6] == 0) return;
    const int4* src = reinterpret_cast<const int4*>(boxes + 8 * size_t(i));
    int4* dst       = reinterpret_cast<int4*>(out + 8 * size_t(scan[i]));
    int4 hi         = src[1];
    hi.w            = owner; // record[7]: who exports the box (find_overlaps marks bit `owner`)
    dst[0]          = src[0];
    dst[1]          = hi;
}

//! cnt[q * nLocal + (i - first)] = particles of leaf i if peer q's boxes touch it (bit `peer` of flags), else 0;
//! q enumerates the peers in rank order without the own rank
__global__ __launch_bounds__(256) void peerCountsKernel(const int32_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ layout, int first, int last,
                                                        int numRanks, int rank, uint32_t* __restrict__ cnt)
{
    int k = blockIdx.x * 256 + threadIdx.x;
    int n = last - first;
    if (k >= n) return;
    uint32_t f = uint32_t(flags[first + k]);
    uint32_t c = layout[first + k + 1] - layout[first + k];
    for (int p = 0, q = 0; p < numRanks; ++p)
    {
        if (p == rank) continue;
        cnt[size_t(q) * n + k] = ((f >> p) & 1u) ? c : 0u;
        ++q;
    }
}

//! totals[q] = particles served to peer q, from the exclusive scan of cnt (grand total in *total)
//! my row of the halo count matrix, one u64 per rank (0 for myself): what the all-gather of the rows takes
__global__ void peerTotalsKernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ total, int n,
                                 int numPeers, int rank, uint64_t* __restrict__ row)
{
    int q = threadIdx.x;
    if (q == numPeers) row[rank] = 0;
    if (q >= numPeers) return;
    uint32_t a = scan[size_t(q) * n];
    uint32_t b = (q + 1 < numPeers) ? scan[size_t(q + 1) * n] : *total;
    row[q < rank ? q : q + 1] = b - a;
}

//! particle indices of the leaves each peer needs, grouped by peer in rank order, 16 lanes per (peer, leaf)
__global__ __launch_bounds__(256) void peerFillKernel(const int32_t* __restrict__ flags,
                                                      const uint32_t* __restrict__ layout,
                                                      const uint32_t* __restrict__ scan, int first, int last,
                                                      int numRanks, int rank, uint32_t* __restrict__ out)
{
    const unsigned sub = threadIdx.x & 15u;
    const int n        = last - first;
    size_t item        = size_t(blockIdx.x) * 16 + (threadIdx.x >> 4);
    if (item >= size_t(numRanks - 1) * n) return;
    int q = int(item / n), k = int(item % n);
    int p = q < rank ? q : q + 1;
    if (!((uint32_t(flags[first + k]) >> p) & 1u)) return;
    uint32_t a = layout[first + k], b = layout[first + k + 1], o = scan[item];
    uint32_t base = layout[first];
    for (uint32_t j = a + sub; j < b; j += 16)
        out[o + (j - a)] = j - base;
}

//! cnt[i - first] = number of particles of leaf i if it is flagged, else 0
__global__ __launch_bounds__(256) void flaggedCountsKernel(const int32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ layout, int first, int last,
                                                           uint32_t* __restrict__ cnt)
{
    int i = first + blockIdx.x * 256 + threadIdx.x;
    if (i < last) cnt[i - first] = flags[i] ? layout[i + 1] - layout[i] : 0u;
}

//! particle indices (relative to the first assigned particle) of the flagged leaves, 16 lanes per leaf
__global__ __launch_bounds__(256) void fillIndicesKernel(const int32_t* __restrict__ flags,
                                                         const uint32_t* __restrict__ layout,
                                                         const uint32_t* __restrict__ scan, int first, int last,
                                                         uint32_t* __restrict__ out)
{
    const unsigned sub = threadIdx.x & 15u;
    int i              = first + blockIdx.x * 16 + int(threadIdx.x >> 4);
    if (i >= last || !flags[i]) return;
    uint32_t a = layout[i], b = layout[i + 1], o = scan[i - first];
    uint32_t base = layout[first];
    for (uint32_t j = a + sub; j < b; j += 16)
        out[o + (j - a)] = j - base;
}

//! the element sizes gatherGpu is instantiated for (R/primitives/primitives_gpu.cu:126-148)
constexpr bool gatherableElement(int e) { return e == 1 || e == 2 || e == 4 || e == 8 || e == 12 || e == 16 || e == 24 || e == 32; }

//! one set of result arrays
constexpr int MAX_PROPS = 16;
struct Out
{
    DevBuf keys, x, y, z, h;
    DevBuf props[MAX_PROPS];
};

struct MrBase
{
    virtual ~MrBase()                                                                    = default;
    virtual int sync(const void* x, const void* y, const void* z, const void* h, size_t n, const void* const* props,
                     const int* propBytes, int numProps, const void* keysIn, const void* mass = nullptr,
                     int massBits = 0) = 0;
    virtual int updateExpansionCenters(const void* x, const void* y, const void* z, const void* m, int massBits) = 0;
    virtual int computeGravity(const void* x, const void* y, const void* z, const void* m, const void* h, int massBits,
                               int order, double G, double eps2, void* ax, void* ay, void* az, void* phi) = 0;
    virtual int adaptH(const void* x, const void* y, const void* z, void* h, uint32_t ng0, uint32_t tol, uint32_t maxIter,
                       float growLimit, uint32_t* counts, uint32_t* status)                = 0;
    virtual int friendsOfFriends(const void* x, const void* y, const void* z, double linkingLength, uint32_t maxRounds,
                                 uint64_t* labels, uint64_t* groupSizes, uint64_t* numGroups, uint32_t* rounds) = 0;
    virtual int fofCatalog(const void* x, const void* y, const void* z, const void* m, int massBits, const void* vx,
                           const void* vy, const void* vz, const uint64_t* labels, uint64_t minMembers, size_t capacity,
                           uint64_t* groupLabels, uint64_t* groupSizes, void* mass, void* center, void* velocity,
                           void* radius, uint32_t* flags, uint32_t* numGroupsHost) = 0;
    virtual int sphereProfiles(const void* x, const void* y, const void* z, const void* w, int massBits, const void* queryCenters,
                               const void* queryScale, uint32_t numQueries, const double* edgesHost, int numBins,
                               uint64_t* counts, double* sums, uint32_t* flags) = 0;
    virtual int knn(const void* x, const void* y, const void* z, const void* queryCenters, const void* queryRmax,
                    uint32_t numQueries, uint32_t k, uint64_t* ids, void* dist2, uint32_t* counts) = 0;
    virtual void knnLast(uint32_t* numChunks, uint64_t* gatherBytes) = 0;
    virtual int pairCounts(bool cross, const void* x, const void* y, const void* z, const void* w, int wBits,
                           const void* queryCenters, const void* queryW, uint32_t numQueries, const double* edgesHost,
                           int numBins, uint64_t* counts, double* sums, uint64_t* statsHost) = 0;
    virtual int multipoles(const void** out, int32_t* numNodes)                           = 0;
    virtual int octupoles(const void** out, int32_t* numNodes)                            = 0;
    virtual int view(cstone_hip_domain_mr_view* out)                                     = 0;
    virtual void setHaloFactor(float f)                                                  = 0;
    virtual int exchangeHalos(void* array, int elemBytes)                                = 0;
    virtual int reapplySync(const void* in, size_t n, int elemBytes, void* out)          = 0;
    virtual int octree(cstone_hip_domain_mr_octree* out)                                 = 0;
    virtual int setHaloMode(int mode)                                                    = 0;
    virtual int setTheta(float theta)                                                    = 0;
    virtual void setSortMode(int mode)                                                   = 0;
    virtual void contextGone(bool gone)                                                  = 0;
};

template<class K, class T>
class MultiRankDomain final : public MrBase
{
    static constexpr int kb = 8 * sizeof(K), rb = 8 * sizeof(T);

public:
    MultiRankDomain(cstone_hip_ctx* ctx, int curve, int rank, int numRanks, uint32_t bucket, uint32_t bucketFocus,
                    const cstone_box& box, const cstone_hip_comm_ops& comm)
        : ctx_(ctx)
        , curve_(curve)
        , rank_(rank)
        , P_(numRanks)
        , bucket_(bucket)
        , bucketFocus_(bucketFocus)
        , box_(box)
        , comm_(comm)
    {
    }

    void setHaloFactor(float f) override { haloExt_ = f; }
    void setSortMode(int mode) override { sortMode_ = mode; }
    void contextGone(bool gone) override { ctxGone_ = gone; }

    //! before the first sync: how halos are found (CSTONE_MR_HALOS_LET: the reference's way, CSTONE_MR_HALOS_OWNER_SIDE)
    int setHaloMode(int mode) override
    {
        if (!firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_set_halo_mode: only before the first sync");
        if (mode != CSTONE_MR_HALOS_LET && mode != CSTONE_MR_HALOS_OWNER_SIDE)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_set_halo_mode: unknown mode %d", mode);
        useLet_ = mode == CSTONE_MR_HALOS_LET;
        return CSTONE_OK;
    }

    //! before the first sync: the opening angle of the focus tree's MAC (Domain ctor, R/domain/domain.hpp:95-113)
    int setTheta(float theta) override
    {
        if (!firstCall_ || !(theta > 0.0f)) return fail(ctx_, CSTONE_E_ARG, "domain_mr_set_theta: only before the first sync");
        theta_ = theta;
        return CSTONE_OK;
    }

    /*! Domain::exchangeHalos (R/domain/domain.hpp:381-386, R/halos/halos.hpp:224-257): repeats the halo exchange of the
     *  last sync for another field.  array: device, laid out like the result arrays (num_particles_with_halos elements
     *  of 1, 2, 4, 8, 12, 16, 24 or 32 bytes); its assigned range is read, its halo ranges are overwritten. */
    int exchangeHalos(void* array, int elemBytes) override
    {
        if (!gatherableElement(elemBytes)) return fail(ctx_, CSTONE_E_ARG, "exchange_halos: element size %d", elemBytes);
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "exchange_halos: no sync yet");
        if (useLet_) return let_->exchangeHalos(array, elemBytes);
        // every rank must take part if anybody exchanges: the totals of the last sync's count matrix decide
        if (P_ == 1 || haloAnyLast_ == 0) return CSTONE_OK;
        char* a = static_cast<char*>(array);
        std::vector<size_t> sb(P_), rb(P_);
        for (int p = 0; p < P_; ++p)
            sb[p] = haloSend_[p] * elemBytes, rb[p] = haloRecv_[p] * elemBytes;
        CS_TRY(sendRows_.ensure(ctx_, std::max<size_t>(haloSel_, 1) * elemBytes));
        CS_TRY(recvRows_.ensure(ctx_, std::max<size_t>(haloRecvLo_ + haloRecvHi_, 1) * elemBytes));
        if (haloSel_)
            CS_TRY(cstone_hip_gather(ctx_, elemBytes, sel_.as<uint32_t>(), haloSel_, a + haloRecvLo_ * elemBytes,
                                     sendRows_.p));
        CS_TRY(callComm(comm_.all_to_all_v(comm_.user, sendRows_.p, sb.data(), recvRows_.p, rb.data()),
                        "all_to_all_v (exchangeHalos)"));
        if (haloRecvLo_)
            CS_HIP(ctx_, hipMemcpyAsync(a, recvRows_.p, haloRecvLo_ * elemBytes, hipMemcpyDeviceToDevice, ctx_->stream));
        if (haloRecvHi_)
            CS_HIP(ctx_, hipMemcpyAsync(a + (haloRecvLo_ + haloAssigned_) * elemBytes,
                                        recvRows_.as<char>() + haloRecvLo_ * elemBytes, haloRecvHi_ * elemBytes,
                                        hipMemcpyDeviceToDevice, ctx_->stream));
        return CSTONE_OK;
    }

    /*! Domain::reapplySync (R/domain/domain.hpp:334-378): sends one more per-particle field along the routes of the last
     *  sync -- the same particles leave to the same ranks, the kept ones and the newcomers land in the same slots.
     *  in: n elements laid out like the INPUT arrays of the last sync; out: laid out like the result arrays
     *  (num_particles_with_halos elements), only its assigned range is written (exchangeHalos fills the rest). */
    int reapplySync(const void* in, size_t n, int elemBytes, void* out) override
    {
        if (!gatherableElement(elemBytes)) return fail(ctx_, CSTONE_E_ARG, "reapply_sync: element size %d", elemBytes);
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "reapply_sync: no sync yet");
        if (n != rsN_) // checkSizesEqual(prevBufDesc_.size, arrays...), R/domain/domain.hpp:341
            return fail(ctx_, CSTONE_E_ARG, "reapply_sync: array of %zu elements, the last sync took %zu", n, size_t(rsN_));
        if ((n && !in) || !out) return fail(ctx_, CSTONE_E_ARG, "reapply_sync: null array");
        const size_t e        = size_t(elemBytes);
        const uint32_t* keptO = order_.as<uint32_t>() + rsKeptOffset_;
        char* dst             = static_cast<char*>(out) + size_t(view_.start_index) * e;
        const void* recvSorted = nullptr;
        if (rsMoved_)
        {
            const std::vector<size_t> sb = peerBytes(rsSendCounts_.data(), 1, e), rbv = peerBytes(rsRecvCounts_.data(), 1, e);
            // 32-byte elements are moved as 16-byte vectors: keep every staging buffer 16-byte aligned (DevBuf is)
            CS_TRY(sendRows_.ensure(ctx_, std::max<size_t>(rsSend_, 1) * e));
            CS_TRY(recvRows_.ensure(ctx_, std::max<size_t>(rsNb_, 1) * e));
            CS_TRY(moveTmp_.ensure(ctx_, std::max<size_t>(rsNb_, 1) * e));
            if (rsSend_) CS_TRY(cstone_hip_gather(ctx_, elemBytes, leaving_.as<uint32_t>(), rsSend_, in, sendRows_.p));
            CS_TRY(callComm(comm_.all_to_all_v(comm_.user, sendRows_.p, sb.data(), recvRows_.p, rbv.data()),
                            "all_to_all_v (reapplySync)"));
            if (rsNb_)
            {
                CS_TRY(cstone_hip_gather(ctx_, elemBytes, ro_.as<uint32_t>(), rsNb_, recvRows_.p, moveTmp_.p));
                recvSorted = moveTmp_.p;
            }
        }
        if (rsNb_)
        {
            CS_TRY(cstone_hip_gather_scatter(ctx_, elemBytes, keptO, posA_.as<uint32_t>(), rsNa_, in, dst));
            CS_TRY(cstone_hip_scatter(ctx_, elemBytes, posB_.as<uint32_t>(), rsNb_, recvSorted, dst));
        }
        else { CS_TRY(cstone_hip_gather(ctx_, elemBytes, keptO, rsNa_, in, dst)); }
        return CSTONE_OK;
    }

    /*! Domain::octreeProperties() / layout() (R/domain/domain.hpp:388-437) for the result arrays of the last sync: a
     *  cornerstone tree (bucketFocus) over ALL local particles, halos included -- the keys of
     *  [halos of lower ranks | assigned | halos of higher ranks] ascend over the whole array, so the tree machinery of
     *  the single-rank path applies as it is.  Built on the first request after a sync, from the tree of the previous
     *  request; a sync that nobody asks a tree for does not pay for one. */
    int octree(cstone_hip_domain_mr_octree* out) override
    {
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_octree: no sync yet");
        if (useLet_)
        {
            // Domain::octreeProperties() is the focus tree itself (R/domain/domain.hpp:425-437): leaves whose particles
            // are not here have empty layout ranges
            const FocusLet<K, T>& t = *let_;
            out->num_leaves = t.numLeaves(), out->num_nodes = t.numNodes();
            out->leaves = t.leaves(), out->leaf_counts = t.leafCounts();
            out->prefixes = t.prefixes(), out->child_offsets = t.childOffsets();
            out->parents = t.parents(), out->level_range = t.levelRange();
            out->internal_to_leaf = t.internalToLeaf(), out->leaf_to_internal = t.leafToInternal();
            out->layout = t.layout();
            out->centers = t.geoCenters(), out->sizes = t.geoSizes();
            out->expansion_centers = haveExpansionCenters_ ? t.expansionCenters() : nullptr;
            return CSTONE_OK;
        }
        if (nsSync_ != syncs_)
        {
            CS_TRY(buildNsTree());
            nsSync_ = syncs_;
        }
        const NodeIdx L = nsLeaves_, M = L + (L - 1) / 7;
        out->num_leaves = L, out->num_nodes = M;
        out->leaves = nsTree_.p, out->leaf_counts = nsCounts_.as<uint32_t>();
        out->prefixes = nsPrefixes_.p, out->child_offsets = nsChild_.as<int32_t>();
        out->parents = nsParents_.as<int32_t>(), out->level_range = nsLevelRange_.as<int32_t>();
        out->internal_to_leaf = nsItl_.as<int32_t>(), out->leaf_to_internal = nsLti_.as<int32_t>();
        out->layout = nsLayout_.as<uint32_t>();
        out->centers = nsCenters_.p, out->sizes = nsSizes_.p;
        out->expansion_centers = nullptr;
        return CSTONE_OK;
    }

    int updateExpansionCenters(const void* x, const void* y, const void* z, const void* m, int massBits) override
    {
        if (firstCall_ || !useLet_ || !let_) return fail(ctx_, CSTONE_E_ARG, "update_expansion_centers: no sync with the LET yet");
        if ((massBits != 32 && massBits != 64) || !x || !y || !z || !m)
            return fail(ctx_, CSTONE_E_ARG, "update_expansion_centers: bad argument");
        const size_t si = view_.start_index;
        int rc = let_->updateExpansionCenters(static_cast<const T*>(x) + si, static_cast<const T*>(y) + si,
                                              static_cast<const T*>(z) + si, static_cast<const char*>(m) + si * size_t(massBits / 8),
                                              massBits, gTree_.as<K>(), gHost_.leaves.data(), gLeaves_);
        haveExpansionCenters_ = rc == CSTONE_OK;
        return rc;
    }

    /*! Barnes-Hut gravity on the locally essential tree (csrc/gravity.hip): the multipoles of every node of the focus
     *  tree about the current expansion centres (FocusLet::updateMultipoles, with its exchanges), then the LET walk over
     *  the assigned particles (order 3: the octupoles with them, through the same exchanges once more).
     *  x, y, z, m are laid out like the result arrays and read on the halo ranges too; the
     *  caller has exchanged the halos of m.  h (nullable): per-particle softening lengths laid out like x and read on the
     *  halo ranges too; the sync's h has them filled (sync: x, y, z and h travel in one halo message).  Whatever makes the call fail on its arguments is decided before the first
     *  collective, from state that is the same on every rank, so nobody is left waiting. */
    int computeGravity(const void* x, const void* y, const void* z, const void* m, const void* h, int massBits,
                       int order, double G, double eps2, void* ax, void* ay, void* az, void* phi) override
    {
        if (!useLet_)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_compute_gravity: needs the locally essential tree "
                                            "(CSTONE_MR_HALOS_LET)");
        if (firstCall_ || !let_ || !haveExpansionCenters_)
            return fail(ctx_, CSTONE_E_ARG,
                        "domain_mr_compute_gravity: no expansion centres (sync_grav or update_expansion_centers after "
                        "the last sync)");
        if (box_.bc[0] == 1 || box_.bc[1] == 1 || box_.bc[2] == 1)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_compute_gravity: periodic boundaries need Ewald summation, which "
                                            "is not provided");
        // (a rank without particles may pass null arrays, like an empty rank of a sync)
        const bool null = view_.num_particles_with_halos > 0 && (!x || !y || !z || !m || !ax || !ay || !az);
        if ((massBits != 32 && massBits != 64) || (order != 0 && order != 2 && order != 3) || !(eps2 >= 0.0) || null)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_compute_gravity: bad argument");
        FocusLet<K, T>& t     = *let_;
        const uint32_t si = view_.start_index, ei = view_.end_index;
        const size_t mb   = size_t(massBits / 8);
        if (gravGroupsSync_ != syncs_)
        {
            CS_TRY(gravGroups_.ensure(ctx_, size_t(ei - si + 1) * sizeof(uint32_t)));
            uint32_t numGroups = 0;
            if (ei > si)
                CS_TRY(cstone_hip_compute_group_splits(ctx_, kb, rb, si, ei, x, y, z, t.leaves(), t.numLeaves(), t.layout(),
                                                       &box_, 64, CSTONE_GRAVITY_GROUP_TOL, gravGroups_.as<uint32_t>(),
                                                       size_t(ei - si) + 1, &numGroups));
            gravNumGroups_  = numGroups;
            gravGroupsSync_ = syncs_;
        }
        CS_TRY(t.updateMultipoles(static_cast<const T*>(x) + si, static_cast<const T*>(y) + si,
                                  static_cast<const T*>(z) + si, static_cast<const char*>(m) + si * mb, massBits,
                                  gTree_.as<K>(), gHost_.leaves.data(), gLeaves_, order));
        if (ei == si) return CSTONE_OK;
        const size_t off = size_t(si) * sizeof(T);
        if (order == 3)
            return cstone_hip_compute_gravity_o3(
                ctx_, rb, massBits, x, y, z, m, h, si, ei, gravGroups_.as<uint32_t>(), gravNumGroups_, &box_,
                t.childOffsets(), t.internalToLeaf(), t.layout(), t.expansionCenters(), t.multipoles(), t.octupoles(), 1, G,
                eps2, static_cast<char*>(ax) + off, static_cast<char*>(ay) + off, static_cast<char*>(az) + off,
                phi ? static_cast<char*>(phi) + off : nullptr, nullptr, nullptr, nullptr);
        return cstone_hip_compute_gravity_let_h(
            ctx_, rb, massBits, x, y, z, m, h, si, ei, gravGroups_.as<uint32_t>(), gravNumGroups_, &box_, t.childOffsets(),
            t.internalToLeaf(), t.layout(), t.expansionCenters(), t.multipoles(), order, G, eps2,
            static_cast<char*>(ax) + off, static_cast<char*>(ay) + off, static_cast<char*>(az) + off,
            phi ? static_cast<char*>(phi) + off : nullptr, nullptr, nullptr, nullptr);
    }

    /*! cstone_hip_adapt_smoothing_lengths for the assigned particles on the tree octree() returns (both halo modes serve
     *  it: the LET's focus tree has empty layout ranges where the particles are elsewhere).  LOCAL, no collective.  The
     *  halos of the last sync cover 2 h x haloExt_ of every assigned particle, so h may grow by haloExt_ at most:
     *  growLimit == 0 means haloExt_, a larger one is refused, and so is a second call before the next sync (the cap is
     *  relative to the h it is handed, it would compound).  x, y, z, h laid out like the result arrays; counts and status
     *  are indexed from start_index; the halo ranges of h are stale afterwards (exchangeHalos). */
    int adaptH(const void* x, const void* y, const void* z, void* h, uint32_t ng0, uint32_t tol, uint32_t maxIter,
               float growLimit, uint32_t* counts, uint32_t* status) override
    {
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_adapt_h: no sync yet");
        if (growLimit == 0.0f) growLimit = haloExt_;
        if (!(growLimit >= 1.0f) || growLimit > haloExt_)
            return fail(ctx_, CSTONE_E_ARG,
                        "domain_mr_adapt_h: grow_limit %g outside [1, halo factor %g]: neighbours beyond the halos are not "
                        "on this rank",
                        double(growLimit), double(haloExt_));
        if (adapted_)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_adapt_h: called twice since the last sync (the cap on h would compound)");
        const uint32_t si = view_.start_index, ei = view_.end_index;
        // (a rank without particles may pass null arrays, like an empty rank of a sync)
        if (ei > si && (!x || !y || !z || !h || !counts || !status))
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_adapt_h: bad argument");
        if (ng0 == 0) return fail(ctx_, CSTONE_E_ARG, "domain_mr_adapt_h: ng0 must be at least 1");
        if (ei > si)
        {
            cstone_hip_domain_mr_octree t;
            CS_TRY(octree(&t));
            CS_TRY(cstone_hip_adapt_smoothing_lengths(ctx_, rb, x, y, z, h, si, ei, &view_.box, t.child_offsets,
                                                      t.internal_to_leaf, t.layout, t.centers, t.sizes, ng0, tol, maxIter,
                                                      growLimit, 0, nullptr, counts, status));
        }
        adapted_ = true;
        return CSTONE_OK;
    }

    /*! Friends-of-friends groups over the particles of ALL ranks (cstone_hip_domain_mr_fof, the definitions are in
     *  include/cstone_hip.h, the method and its proof in DESIGN.md section 5f): global ids as initial labels, the local
     *  components of everything present on the rank (halos included), then rounds of { lower the labels to the minimum of
     *  their local component, exchange the halos of the labels, all-reduce "somebody changed an assigned label" } up to the
     *  first quiet round; the group sizes through one exchange of (label, count) pairs with the owners of the labels.
     *  Works on buffers of the domain and copies to the caller's arrays at the very end: a refused call writes nothing.
     *  Whatever is the same on every rank is refused before the first collective; rank-local trouble rides in the status
     *  word of the all-gather, so that everybody returns from the same point.  A list of stages that share one FofState. */
    int friendsOfFriends(const void* x, const void* y, const void* z, double b, uint32_t maxRounds, uint64_t* labels,
                         uint64_t* groupSizes, uint64_t* numGroups, uint32_t* rounds) override
    {
        FofState s{x, y, z, b, maxRounds, labels, groupSizes, numGroups, rounds};
        CS_TRY(fofRefuseEverywhere(s));
        fofLocalComponents(s);
        CS_TRY(fofAgree(s));
        CS_TRY(fofAssignIds(s));
        CS_TRY(fofRounds(s));
        CS_TRY(fofCountGroups(s));
        if (s.wantSizes) CS_TRY(fofGroupSizes(s.offset, fofComp_.as<uint32_t>(), fofLabels_.as<uint64_t>()));
        return fofHandOut(s);
    }

    /*! The group catalogue across ranks (cstone_hip_domain_mr_fof_catalog; the rule and the method: include/cstone_hip.h,
     *  DESIGN.md section 5f): one partial per distinct label of the assigned range about its first member, the partials
     *  to the owners of the labels, the owner's combine in (label, source rank) order, filter and finish.  Two
     *  collectives: the all-gather of the counts per owner, with the status of the local steps on board, and the
     *  all_to_all_v of the records.  The capacity is judged behind them.  A list of stages that share one CatalogState. */
    int fofCatalog(const void* x, const void* y, const void* z, const void* m, int massBits, const void* vx, const void* vy,
                   const void* vz, const uint64_t* labels, uint64_t minMembers, size_t capacity, uint64_t* groupLabels,
                   uint64_t* groupSizes, void* mass, void* center, void* velocity, void* radius, uint32_t* flags,
                   uint32_t* numGroupsHost) override
    {
        CatalogState s{x, y, z, m, massBits, vx, vy, vz, labels, minMembers, capacity, groupLabels, groupSizes, mass, center,
                       velocity, radius, flags, numGroupsHost};
        CS_TRY(catalogRefuseEverywhere(s));
        catalogLocalTrouble(s);
        catalogLocalSteps(s);
        CS_TRY(catalogAgree(s));
        CS_TRY(catalogExchange(s));
        if (s.numRecv == 0) return CSTONE_OK;
        CS_TRY(catalogCombine(s));
        return catalogFinish(s);
    }

    /*! Sphere profiles over the particles of all ranks (cstone_hip_domain_mr_sphere_profiles; the rule: include/
     *  cstone_hip.h).  Every rank bins its assigned range on its own octree into the caller's arrays; one all-gather of
     *  {status, Q, NB, w given} lets every rank fail together; one all-reduce of {counts as doubles, sums} follows.  A list
     *  of stages that share one ProfilesState. */
    int sphereProfiles(const void* x, const void* y, const void* z, const void* w, int massBits, const void* queryCenters,
                       const void* queryScale, uint32_t numQueries, const double* edgesHost, int numBins, uint64_t* counts,
                       double* sums, uint32_t* flags) override
    {
        ProfilesState s{x, y, z, w, massBits, queryCenters, queryScale, numQueries, edgesHost, numBins, counts, sums, flags};
        CS_TRY(profilesRefuseEverywhere(s));
        if (P_ == 1) return profilesOnOneRank(s);
        profilesLocalTrouble(s);
        CS_TRY(profilesAgree(s));
        if (numQueries == 0) return CSTONE_OK;
        CS_TRY(profilesLocal(s));
        return profilesReduce(s);
    }

    /*! The k nearest neighbours of arbitrary points among the particles of all ranks (cstone_hip_domain_mr_knn; the
     *  rule: include/cstone_hip.h).  Every rank searches its assigned range on its own octree; one all-gather of {status, Q,
     *  k, rmax given, assigned count} lets every rank fail together and gives the id ranges; the ranks' rows travel in
     *  chunks of queries through all_gather and a merge kernel keeps the k best of them.  A list of stages that share one
     *  KnnState. */
    int knn(const void* x, const void* y, const void* z, const void* queryCenters, const void* queryRmax, uint32_t numQueries,
            uint32_t k, uint64_t* ids, void* dist2, uint32_t* counts) override
    {
        KnnState s{x, y, z, queryCenters, queryRmax, numQueries, k, ids, dist2, counts};
        CS_TRY(knnRefuseEverywhere(s));
        knnLocalTrouble(s);
        CS_TRY(knnAgree(s));
        for (uint32_t q0 = 0; q0 < numQueries; q0 += s.chunk)
        {
            const uint32_t nq = std::min(s.chunk, numQueries - q0);
            CS_TRY(knnLocal(s, q0, nq));
            CS_TRY(knnGather(s, nq));
            CS_TRY(knnMerge(s, q0, nq));
            ++knnChunks_;
        }
        return CSTONE_OK;
    }

    /*! Pair counts in radial bins over the particles of all ranks (cstone_hip_domain_mr_pair_counts and ..._cross; the
     *  rule: include/cstone_hip.h).  Auto: targets are my assigned range, sources everything on the rank, so every ordered
     *  pair is counted at the owner of i -- under the cover rule of friendsOfFriends.  Cross: every rank bins its assigned
     *  range about the same queries.  One all-gather lets every rank fail together; one all-reduce of {counts as doubles,
     *  sums} follows.  A list of stages that share one PairState. */
    int pairCounts(bool cross, const void* x, const void* y, const void* z, const void* w, int wBits, const void* queryCenters,
                   const void* queryW, uint32_t numQueries, const double* edgesHost, int numBins, uint64_t* counts, double* sums,
                   uint64_t* statsHost) override
    {
        PairState s{cross, x, y, z, w, wBits, queryCenters, queryW, numQueries, edgesHost, numBins, counts, sums, statsHost};
        CS_TRY(pairRefuseEverywhere(s));
        if (P_ == 1) return pairOnOneRank(s);
        pairLocalTrouble(s);
        CS_TRY(pairAgree(s));
        CS_TRY(pairLocal(s));
        return pairReduce(s);
    }

    void knnLast(uint32_t* numChunks, uint64_t* gatherBytes) override
    {
        if (numChunks) *numChunks = knnChunks_;
        if (gatherBytes) *gatherBytes = knnGatherBytes_;
    }

    int multipoles(const void** out, int32_t* numNodes) override
    {
        const bool have = useLet_ && let_ && !firstCall_ && haveExpansionCenters_;
        *out            = have ? let_->multipoles() : nullptr;
        *numNodes       = have ? let_->numNodes() : 0;
        return CSTONE_OK;
    }

    int octupoles(const void** out, int32_t* numNodes) override
    {
        const bool have = useLet_ && let_ && !firstCall_ && haveExpansionCenters_ && let_->octupoles();
        *out            = have ? let_->octupoles() : nullptr;
        *numNodes       = have ? let_->numNodes() : 0;
        return CSTONE_OK;
    }

    ~MultiRankDomain() override
    {
        if (hostLevelRange_)
        {
            if (!ctxGone_) (void)hipStreamSynchronize(ctx_->stream); // a copy into the block may still be queued
            (void)hipHostFree(hostLevelRange_);
        }
        if (timing_ && rank_ == 0)
        {
            std::fprintf(stderr, "[cstone_hip_domain_mr] phase times per sync over %d syncs (ms, synchronising):", syncs_);
            for (auto& [name, sec] : phase_)
                std::fprintf(stderr, "  %s %.3f", name.c_str(), sec * 1e3 / std::max(1, syncs_));
            std::fprintf(stderr, "\n");
        }
    }

    int view(cstone_hip_domain_mr_view* v) override
    {
        *v = view_;
        return CSTONE_OK;
    }

    /*! Domain::sync on several ranks (R/domain/domain.hpp:196-243): a list of stages that share one SyncState.  What
     *  each stage decides, which collective and which read-back it issues and where the status word rides: DESIGN.md,
     *  section 2c.  The tick() marks are the phases CSTONE_MR_TIMING reports. */
    int sync(const void* x, const void* y, const void* z, const void* h, size_t n, const void* const* props,
             const int* propBytes, int numProps, const void* keysIn, const void* mass, int massBits) override
    {
        SyncState s{static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const T*>(z), static_cast<const T*>(h),
                    n, keysIn, props, propBytes, numProps, massBits};
        CS_TRY(beginSync(s, mass));
        tick(nullptr);
        CS_TRY(chooseBox(s));
        tick("1 box");
        CS_TRY(reserveSortBuffers(s));
        takeLevelRanges();
        CS_TRY(tryResort(s));
        CS_TRY(encodeAndSort(s));
        tick("2 encode+sort");
        CS_TRY(stepGlobalTreeAndAssign(s));
        tick("3 global tree+assign");
        CS_TRY(redoCutsIfAssignmentChanged(s));
        CS_TRY(planExchange(s));
        CS_TRY(exchangeParticles(s));
        CS_TRY(sortNewcomers(s));
        CS_TRY(exchangeProperties(s));
        CS_TRY(reserveResultArrays(s));
        CS_TRY(mergeAndPlace(s));
        tick("4 exchange+merge+place");
        if (useLet_)
        {
            CS_TRY(updateLet(s));
            tick("5 focus tree (LET)");
        }
        else
        {
            // ---- this rank's finest tree over its assigned particles; its SFC range must end on leaf boundaries
            CS_TRY(updateFocusTree(s.keysM, s.nm));
            tick("5a focus update");
            CS_TRY(enforceBoundaries(s.keysM, s.nm, &s.first, &s.last));
            tick("5b boundaries");
            CS_TRY(buildFocusOctree());
            tick("5c linked octree");
            CS_TRY(layoutOwnTree(s));
            tick("5 focus tree");
            CS_TRY(discoverHalosOwnerSide(s));
        }
        tick("6 halo discovery");
        CS_TRY(joinPlace());
        CS_TRY(makeRoomForHalos(s));
        tick("7 margins");
        CS_TRY(exchangeHaloParticles(s));
        tick("8 halo exchange");
        return finishSync(s);
    }

private:
    //! What the stages of one sync share: the caller's arrays and what the stages before have decided.  Made by sync().
    struct SyncState
    {
        const T *x, *y, *z, *h;
        size_t n; // (0 from beginSync on for a rank that limps on as an empty rank)
        const void* keysIn;
        const void* const* props; // the caller's properties; syncGrav: propList, the masses behind them
        const int* propBytes;
        int numProps, massBits; // massBits 0: not a syncGrav
        const void* propList[MAX_PROPS + 1] = {};
        int propSizes[MAX_PROPS + 1]        = {};
        const K* resortTree = nullptr; // the leaves of my range as the last COMPLETED sync left them, and their number
        int resortLeaves    = 0;
        bool resortReady    = false; // everything a re-sort needs holds, but for the box being that of the layout still
        bool speculate      = false; // the keys are computed with the box of the previous sync, the same pass measures
        bool resorted       = false; // the re-sort has put keys_ and order_ into their final order
        bool partialSort    = false; // the radix sort left runs to the fix-up: its flag is on its way to the pinned block
        bool speculateCuts  = false; // the cut points were asked for before assign()
        std::vector<K> cutKeys;      // ... for this assignment
        std::vector<uint64_t> cut, rows; // cut points in my sorted keys; the all-gathered count rows, word P = status
        uint64_t *pinRows = nullptr, *pinCut = nullptr;
        ExchangePlan plan;
        uint64_t nm = 0; // assigned particles: plan.na kept (keys and input slots at keptKeys, keptO) + plan.nb received
        const K* keptKeys     = nullptr;
        const uint32_t* keptO = nullptr;
        Out* o        = nullptr;
        uint64_t M = 0, cap = 0, off = 0; // first assigned slot, length of the result arrays, start of what is handed out
        K* keysM      = nullptr;
        int first = 0, last = 0; // my leaves in the focus tree
        std::vector<uint64_t> hsCounts, hmatrix; // halos I send to rank p; hmatrix[src * P + dst] (owner-side mode)
        uint64_t numMyBoxes = 0, selTotal = 0, nlo = 0, nhi = 0, haloAny = 0; // haloAny: the same on every rank
    };

    // ---- The slots of scal_, one block of device scalars (sized in beginSync).  extentsDev and gatherRow are the SAME
    //      address: the box reduction of tryResort consumes the extents before the first cut points are queued.  The four
    //      counters of the re-sort follow boxOperand (bytes 56..71) and overlap scanTotal: they are read back in tryResort,
    //      scanTotal belongs to the owner-side halo discovery.
    template<class V>
    V* slot(size_t byte) const { return reinterpret_cast<V*>(scal_.as<char>() + byte); }
    double* boxOperand() const { return slot<double>(0); }        // (lo, -hi) per axis, status: the MIN all-reduce
    uint32_t* scanTotal() const { return slot<uint32_t>(64); }    // {total of a scan, status word}
    int* tooLongFlag() const { return slot<int>(128); }           // the partial sort met a run it cannot fix up
    T* extentsDev() const { return slot<T>(256); }                // {min, max} per axis, measured by the encode
    uint64_t* gatherRow() const { return slot<uint64_t>(256); }   // my row of an all-gather, up to P + 1 words
    uint64_t* leafQuery() const { return slot<uint64_t>(1024); }  // enforceBoundaries: 2 x (index, start, end)
    K* cutKeysDev() const { return slot<K>(2048); }               // the assignment, P + 1 keys, then as many cut points
    uint64_t* cutPointsDev() const { return slot<uint64_t>(2048 + size_t(P_ + 1) * 8); }
    uint64_t* gatherRecv() const { return slot<uint64_t>(4096); } // the rows of everybody, up to P (P + 1) words

    //! bytes[p] = counts[p * stride] elements of e bytes for every peer p, 0 for myself: what all_to_all_v takes
    std::vector<size_t> peerBytes(const uint64_t* counts, size_t stride, size_t e) const
    {
        std::vector<size_t> bytes(P_, 0);
        for (int p = 0; p < P_; ++p)
            if (p != rank_) bytes[p] = counts[p * stride] * e;
        return bytes;
    }

    //! The arguments; syncGrav: the masses travel as one more property behind the caller's.  A failure of the arguments (or
    //! one injected by the tests, CSTONE_MR_FAIL_AT) becomes the pending status the peers must learn about
    int beginSync(SyncState& s, const void* mass)
    {
        if (s.massBits)
        {
            if (!useLet_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_sync_grav: needs the locally essential tree (CSTONE_MR_HALOS_LET)");
            if ((s.massBits != 32 && s.massBits != 64) || s.massBits > rb || (s.n && !mass) || s.numProps < 0 || s.numProps >= MAX_PROPS)
                return fail(ctx_, CSTONE_E_ARG, "domain_mr_sync_grav: masses of 32 or 64 bits (not wider than the coordinates), "
                                                "at most %d further properties", MAX_PROPS - 1);
            for (int q = 0; q < s.numProps; ++q)
                s.propList[q] = s.props[q], s.propSizes[q] = s.propBytes[q];
            s.propList[s.numProps] = mass, s.propSizes[s.numProps] = s.massBits / 8;
            s.props = s.propList, s.propBytes = s.propSizes, ++s.numProps;
        }
        pending_ = 0, toggled_ = false;
        CS_TRY(joinPlace()); // (a sync that was abandoned behind its fork: whatever it left on the second stream comes first)
        ctx_->sideBusy &= ~SIDE_AUX;
        if (s.numProps < 0 || s.numProps > MAX_PROPS) setPending(CSTONE_E_ARG, "domain_mr_sync: at most %d properties", MAX_PROPS);
        for (int q = 0; q < s.numProps && !pending_; ++q)
            if ((s.n && !s.props[q]) || !gatherableElement(s.propBytes[q])) // an empty rank may pass null arrays
                setPending(CSTONE_E_ARG, "domain_mr_sync: property %d must have elements of 1, 2, 4, 8, 12, 16, 24 or 32 bytes", q);
        if (s.n >= (size_t(1) << 30)) setPending(CSTONE_E_ARG, "domain_mr_sync: too many particles per rank");
        injectFailure("start");
        if (pending_)
        {
            if (P_ == 1) return agreed(rank_);
            s.n = 0, s.numProps = 0; // limp on as an empty rank until the peers know
        }
        s.hsCounts.assign(P_, 0), s.hmatrix.assign(size_t(P_) * P_, 0);
        CS_TRY(scal_.ensure(ctx_, 4096 + size_t(P_) * (P_ + 1) * 8 + size_t(P_ + 1) * 16));
        ++syncs_;
        adapted_ = false;
        return CSTONE_OK;
    }

    //! The box: measured first, or, in a sync that is going to re-sort, speculated to be that of the previous sync and
    //! measured by the encode (tryResort).  The box all-reduce is the first collective of the sync either way
    int chooseBox(SyncState& s)
    {
        const bool anyOpen = !(box_.bc[0] == 1 && box_.bc[1] == 1 && box_.bc[2] == 1);
        // What the re-sort of THIS sync starts from.  The members are set again only behind the tree update: a sync that
        // fails half way may have rebalanced, swapped or freed the buffers they point into, and the retry sorts from scratch
        s.resortTree = resortTree_, s.resortLeaves = resortLeaves_;
        const uint64_t layoutParticles = layoutParticles_;
        resortTree_ = nullptr, resortLeaves_ = 0, layoutParticles_ = 0;
        s.resortReady = !firstCall_ && s.n >= resortMinParticles() && s.n == layoutParticles &&
                        LeafResort<K>::leavesPerTile(bucketFocus_) > 0 && s.resortLeaves > 0 && resortBackoff_ == 0 &&
                        !pending_ && mayResort(sortMode_);
        // (CSTONE_NO_SPECULATIVE_BOX: read once, in the constructor; the single-rank path reads it per sync)
        s.speculate = s.resortReady && anyOpen && !measureFirst_ && speculativeBox_ && sameLimits(box_, layoutBox_);
        if (s.speculate) return CSTONE_OK;
        const cstone_box before = box_;
        CS_TRY(updateBox(s.x, s.y, s.z, s.n));
        if (!firstCall_ && anyOpen) measureFirst_ = !sameLimits(box_, before);
        return CSTONE_OK;
    }

    //! buffers of keys + SFC ordering of the present particles, and the caller's keys into them
    int reserveSortBuffers(SyncState& s)
    {
        const size_t nAlloc = std::max<size_t>(s.n, 64);
        CS_TRY(keys_.ensure(ctx_, nAlloc * sizeof(K)));
        CS_TRY(order_.ensure(ctx_, nAlloc * sizeof(uint32_t)));
        CS_TRY(ensureSortScratch(nAlloc));
        // encode leaves entries that hold the remove marker 2^(3 maxLevel) alone (R/sfc/sfc.hpp:284-291): such particles sort
        // behind the end of the curve and leave the domain (no key array from the caller: no markers, keys_ is pure output)
        if (s.keysIn && s.n)
            CS_HIP(ctx_, hipMemcpyAsync(keys_.p, s.keysIn, s.n * sizeof(K), hipMemcpyDeviceToDevice, ctx_->stream));
        return CSTONE_OK;
    }

    //! the level ranges of the previous sync's tree (in the pinned block since its build, many stream synchronisations
    //! ago): at EVERY sync -- buildFocusOctree() bounds its digit passes by them, also on the syncs that re-sort
    void takeLevelRanges()
    {
        if (levelRangePending_) prevMaxLeafLevel_ = deepestLevel<K>(hostLevelRange_);
        levelRangePending_ = false;
    }

    /*! The incremental re-sort (resort.hpp), as in the single-rank domain: the input is the assigned block the previous
     *  sync handed out, ordered by the leaves of this rank's tree (layout_).  Unlike there, a sync that speculates on the
     *  box has the box all-reduce in the middle, whose read-back brings the re-sort's counters too.  Sets s.resorted. */
    int tryResort(SyncState& s)
    {
        // (box_ may be a freshly measured one by now; a sync that speculates has left it alone, so it always attempts:
        //  no box is left unmeasured)
        const bool attempt = s.resortReady && sameLimits(box_, layoutBox_);
        if (resortBackoff_ > 0) --resortBackoff_;
        if (!attempt) return CSTONE_OK;
        const int tileLeaves = LeafResort<K>::leavesPerTile(bucketFocus_);
        CS_TRY(resort_.prepare(ctx_, s.resortTree, layout_.as<uint32_t>(), s.resortLeaves, s.n, keysAlt_.as<K>(),
                               lastMovers_ > 100000));
        const ResortArgs<K> ra = resort_.args();
        bool done              = false;
        CS_TRY(computeKeysResort(ctx_, curve_, kb, rb, s.x, s.y, s.z, s.keysIn ? keys_.p : nullptr, s.n, box_, &ra,
                                 s.speculate ? extentsDev() : nullptr, &done));
        bool boxHolds = true, foundHere = false;
        int found[4] = {0, 0, 0, 0};
        if (s.speculate)
        {
            // (the keys above were computed with the box of the previous sync: was it still the box?)
            double* dev = boxOperand();
            if (done)
            {
                CS_TRY(resort_.binMovers(ctx_, tileLeaves));
                // (the re-sort's counters and this rank's status word become part of the operand: one launch, and
                //  one copy and one synchronisation bring the reduced extents and the counters)
                CS_TRY(extentsToReduceOperand(ctx_, rb, extentsDev(), dev, statusWord(), ctx_->devScalars + RESORT_SCALARS));
                foundHere = true;
            }
            else
            {
                const void* arrays[3] = {s.x, s.y, s.z};
                CS_TRY(minMaxCoordinatesDev(ctx_, rb, arrays, 3, s.n, dev));
            }
            cstone_box next;
            CS_TRY(reduceBox(dev, &next, foundHere, foundHere ? found : nullptr));
            boxHolds = sameLimits(next, box_);
            if (!boxHolds) box_ = next, measureFirst_ = true, ++boxRedos_;
        }
        else if (done) { CS_TRY(resort_.binMovers(ctx_, tileLeaves)); }
        if (!done || !boxHolds) return CSTONE_OK;
        if (!foundHere) CS_TRY(copyToHost(ctx_, found, ctx_->devScalars + RESORT_SCALARS, sizeof found));
        const uint32_t markers = uint32_t(found[0]), J = uint32_t(found[2]), movers = uint32_t(found[3]);
        if (!resortAccepted(found[1], movers, s.n))
        {
            resortBackoff_ = RESORT_BACKOFF_SYNCS; // (not counted here, unlike the single-rank path)
            return CSTONE_OK;
        }
        CS_TRY(resort_.sortLeaves(ctx_, keysAlt_.as<K>(), keys_.as<K>(), order_.as<uint32_t>(), movers, markers, J,
                                  tileLeaves, (found[1] & RESORT_LARGE_QUIET_TILES) != 0));
        s.resorted  = true;
        lastMovers_ = movers;
        ++resorts_;
        return CSTONE_OK;
    }

    //! the radix path: passes only over the digits above the leaf level (+1) of the previous tree, runs of equal high
    //! digits are finished by a fix-up pass; a run that is too long raises a flag and the regular sort completes the job
    int encodeAndSort(SyncState& s)
    {
        if (!s.n || s.resorted) return CSTONE_OK;
        int startPass = 0;
        // (the deepest level: as the last read of the pinned block left it; the single-rank path keeps the whole array)
        if (!firstCall_ && prevMaxLeafLevel_ >= 0 && !allDigits(sortMode_))
            startPass = partialSortStartPass<K>(prevMaxLeafLevel_, bucketFocus_);
        CS_TRY(sfcKeysAndOrderingHint(ctx_, curve_, kb, rb, s.x, s.y, s.z, keys_.p, order_.as<uint32_t>(), s.n, box_,
                                      keysAlt_.p, orderAlt_.as<uint32_t>(), sortTmp_.p, sortTmp_.bytes, startPass,
                                      tooLongFlag(), s.keysIn != nullptr));
        // the flag travels to the pinned host block behind the sort; the read-back of the global tree update completes the
        // stream (the global leaf boundaries cannot fall inside a run: that update is not affected by an unfinished order)
        s.partialSort = startPass > 0;
        if (s.partialSort) CS_TRY(copyToPinned(ctx_, ctx_->hostScalars + 3, tooLongFlag(), sizeof(int)));
        return CSTONE_OK;
    }

    //! cut points of assignment_ in my sorted keys and my row of the count matrix, which goes from the device into the
    //! all-gather of the rows (word P of a row: the status of that rank, 0 = fine); all queued, into gHost_'s pinned block
    int queueCuts(SyncState& s)
    {
        s.cutKeys = assignment_;
        CS_TRY(cstone_hip_upload(ctx_, cutKeysDev(), assignment_.data(), size_t(P_ + 1) * sizeof(K)));
        hipLaunchKernelGGL(cutPointsKernel<K>, gridFor(size_t(P_) + 1, 64), 64, 0, ctx_->stream, keys_.as<K>(), s.n,
                           cutKeysDev(), P_, cutPointsDev(), gatherRow(), uint64_t(pending_ ? 1 : 0));
        CS_HIP(ctx_, hipGetLastError());
        if (!s.pinRows)
        {
            s.pinRows = static_cast<uint64_t*>(gHost_.pin.take(s.rows.size() * 8));
            s.pinCut  = static_cast<uint64_t*>(gHost_.pin.take(size_t(P_ + 1) * 8));
        }
        if (P_ > 1)
        {
            CS_TRY(callComm(comm_.all_gather(comm_.user, gatherRow(), gatherRecv(), size_t(P_ + 1) * 8),
                            "all_gather (counts)"));
            CS_TRY(copyToPinned(ctx_, s.pinRows, gatherRecv(), s.rows.size() * 8));
        }
        return copyToPinned(ctx_, s.pinCut, cutPointsDev(), size_t(P_ + 1) * 8);
    }
    //! ... behind a synchronisation of the stream
    void takeCuts(SyncState& s)
    {
        std::copy(s.pinCut, s.pinCut + P_ + 1, s.cut.begin());
        if (P_ > 1) std::copy(s.pinRows, s.pinRows + s.rows.size(), s.rows.begin());
    }

    //! C2 and the first half of C3.  The assignment rarely changes: the cut points for that of the LAST sync are queued
    //! right behind the global counts, and ONE read-back brings counts, cut points and count matrix
    int stepGlobalTreeAndAssign(SyncState& s)
    {
        CS_TRY(updateGlobalTree(s.n));
        // (counts, and the leaf array when the device made it; room behind them for the cut points and the count matrix)
        CS_TRY(gHost_.queueReadBack(ctx_, gTree_, gCounts_, gLeaves_, !gLeavesOnHost_, size_t(P_ + 1) * (P_ + 2) * 8 + 1024));
        s.cut.assign(P_ + 1, 0), s.rows.assign(size_t(P_) * (P_ + 1), 0);
        injectFailure("assign");
        s.speculateCuts = !firstCall_ && int(assignment_.size()) == P_ + 1 && speculateCuts_;
        if (s.speculateCuts) CS_TRY(queueCuts(s));
        CS_HIP(ctx_, hipStreamSynchronize(ctx_->stream)); // global counts (+ leaves), the sort's flag, cut points, matrix
        gHost_.takeReadBack();
        if (s.speculateCuts) takeCuts(s);
        if (s.partialSort && ctx_->hostScalars[3] != 0)
            CS_TRY(cstone_hip_sort_pairs(ctx_, kb, keys_.p, order_.as<uint32_t>(), s.n, keysAlt_.p, orderAlt_.as<uint32_t>(),
                                         sortTmp_.p, sortTmp_.bytes));
        return assign();
    }

    //! only a sync whose assignment did change (or that did not speculate on it) asks for the cut points again
    int redoCutsIfAssignmentChanged(SyncState& s)
    {
        if (s.speculateCuts && s.cutKeys == assignment_) return CSTONE_OK;
        if (s.speculateCuts) ++cutRedos_;
        CS_TRY(queueCuts(s));
        CS_HIP(ctx_, hipStreamSynchronize(ctx_->stream));
        takeCuts(s);
        return CSTONE_OK;
    }

    //! who sends what to whom (exchangePlan, host_rules.hpp); every rank derives the same errors from the same matrix
    int planExchange(SyncState& s)
    {
        s.plan                = exchangePlan(rank_, P_, s.cut, s.rows);
        const ExchangePlan& e = s.plan;
        if (e.failedRank >= 0) return agreed(e.failedRank);
        if (e.badRank >= 0 && e.badArriving == 0)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_sync: rank %d is left without particles", e.badRank);
        if (e.badRank >= 0) return fail(ctx_, CSTONE_E_ARG, "domain_mr_sync: too many particles for rank %d", e.badRank);
        s.keptKeys = keys_.as<K>() + s.cut[rank_];
        s.keptO    = order_.as<uint32_t>() + s.cut[rank_];
        s.nm       = e.na + e.nb;
        return CSTONE_OK;
    }

    //! C3: leaving particles are packed through the ordering as (x, y, z, h) rows, ONE all_to_all_v
    int exchangeParticles(SyncState& s)
    {
        const uint64_t mSend = s.plan.mSend;
        if (!s.plan.movedAny) return CSTONE_OK;
        CS_TRY(leaving_.ensure(ctx_, std::max<size_t>(mSend, 1) * sizeof(uint32_t)));
        CS_TRY(sendRows_.ensure(ctx_, std::max<size_t>(mSend, 1) * 4 * sizeof(T)));
        CS_TRY(recvRows_.ensure(ctx_, std::max<size_t>(s.plan.nb, 1) * 4 * sizeof(T)));
        size_t nLow = s.cut[rank_] - s.cut[0], nHigh = s.cut[P_] - s.cut[rank_ + 1];
        if (nLow)
            CS_HIP(ctx_, hipMemcpyAsync(leaving_.p, order_.as<uint32_t>() + s.cut[0], nLow * 4, hipMemcpyDeviceToDevice,
                                        ctx_->stream));
        if (nHigh)
            CS_HIP(ctx_, hipMemcpyAsync(leaving_.as<uint32_t>() + nLow, order_.as<uint32_t>() + s.cut[rank_ + 1], nHigh * 4,
                                        hipMemcpyDeviceToDevice, ctx_->stream));
        if (mSend)
            hipLaunchKernelGGL(packRowsKernel<T>, gridFor(mSend, 256), 256, 0, ctx_->stream, leaving_.as<uint32_t>(),
                               size_t(mSend), s.x, s.y, s.z, s.h, sendRows_.as<T>());
        const std::vector<size_t> sb = peerBytes(s.plan.sendCounts.data(), 1, 4 * sizeof(T)),
                                  rbv = peerBytes(s.plan.matrix.data() + rank_, P_, 4 * sizeof(T));
        return callComm(comm_.all_to_all_v(comm_.user, sendRows_.p, sb.data(), recvRows_.p, rbv.data()), "all_to_all_v (particles)");
    }

    //! newcomers: sorted among themselves
    int sortNewcomers(SyncState& s)
    {
        const uint64_t nb = s.plan.nb;
        if (!nb) return CSTONE_OK;
        for (int c = 0; c < 4; ++c)
        {
            CS_TRY(rcol_[c].ensure(ctx_, nb * sizeof(T)));
            CS_TRY(rcolS_[c].ensure(ctx_, nb * sizeof(T)));
        }
        hipLaunchKernelGGL(unpackRowsKernel<T>, gridFor(nb, 256), 256, 0, ctx_->stream, recvRows_.as<T>(), size_t(nb),
                           rcol_[0].as<T>(), rcol_[1].as<T>(), rcol_[2].as<T>(), rcol_[3].as<T>());
        CS_TRY(rk_.ensure(ctx_, nb * sizeof(K)));
        CS_TRY(ro_.ensure(ctx_, nb * sizeof(uint32_t)));
        CS_TRY(ensureSortScratch(std::max<size_t>({s.n, 64, nb})));
        CS_HIP(ctx_, hipMemsetAsync(rk_.p, 0, nb * sizeof(K), ctx_->stream));
        CS_TRY(cstone_hip_compute_sfc_keys(ctx_, curve_, kb, rb, rcol_[0].p, rcol_[1].p, rcol_[2].p, rk_.p, nb, &box_));
        CS_TRY(cstone_hip_sort_keys_ordering(ctx_, kb, rk_.p, ro_.as<uint32_t>(), nb, keysAlt_.p, orderAlt_.as<uint32_t>(),
                                             sortTmp_.p, sortTmp_.bytes));
        for (int c = 0; c < 4; ++c) // (rcolS_: in the newcomers' sorted order)
            CS_TRY(cstone_hip_gather(ctx_, sizeof(T), ro_.as<uint32_t>(), nb, rcol_[c].p, rcolS_[c].p));
        return CSTONE_OK;
    }

    //! further conserved fields travel the same way, one collective per field (the volume is small in the steady state);
    //! received values are brought into the newcomers' sorted order (propRecvS_)
    int exchangeProperties(SyncState& s)
    {
        const ExchangePlan& e = s.plan;
        for (int q = 0; q < s.numProps && e.movedAny; ++q)
        {
            const size_t b = size_t(s.propBytes[q]);
            const std::vector<size_t> sb = peerBytes(e.sendCounts.data(), 1, b), rbv = peerBytes(e.matrix.data() + rank_, P_, b);
            CS_TRY(sendRows_.ensure(ctx_, std::max<size_t>(e.mSend, 1) * b));
            CS_TRY(propRecv_[q].ensure(ctx_, std::max<size_t>(e.nb, 1) * b));
            CS_TRY(propRecvS_[q].ensure(ctx_, std::max<size_t>(e.nb, 1) * b));
            if (e.mSend) CS_TRY(cstone_hip_gather(ctx_, int(b), leaving_.as<uint32_t>(), e.mSend, s.props[q], sendRows_.p));
            CS_TRY(callComm(comm_.all_to_all_v(comm_.user, sendRows_.p, sb.data(), propRecv_[q].p, rbv.data()),
                            "all_to_all_v (property)"));
            if (e.nb) CS_TRY(cstone_hip_gather(ctx_, int(b), ro_.as<uint32_t>(), e.nb, propRecv_[q].p, propRecvS_[q].p));
        }
        return CSTONE_OK;
    }

    //! Result arrays.  The assigned block is written ONCE, at an offset M that leaves room for the halos of the lower ranks
    //! (resultMargins, host_rules.hpp: their number is only known after the discovery); what is handed out starts below M
    int reserveResultArrays(SyncState& s)
    {
        cur_ ^= 1; // the inputs may live in the other buffer set
        toggled_ = true;
        Out& o   = out_[cur_];
        s.o      = &o;
        const ResultMargins m = resultMargins(s.nm, prevLo_, prevHi_, firstCall_, P_ > 1 && !noMargin_);
        s.M = m.M, s.cap = m.cap;
        CS_TRY(o.keys.ensure(ctx_, s.cap * sizeof(K)));
        for (DevBuf* b : {&o.x, &o.y, &o.z, &o.h})
            CS_TRY(b->ensure(ctx_, s.cap * sizeof(T)));
        for (int q = 0; q < s.numProps; ++q)
            CS_TRY(o.props[q].ensure(ctx_, s.cap * size_t(s.propBytes[q])));
        s.keysM = o.keys.as<K>() + s.M;
        return CSTONE_OK;
    }

    //! the columns WHICH of the kept particles to their final slots (placeColumnsKernel), on the current stream
    template<int WHICH>
    void placeColumns(const SyncState& s, T* const* dst)
    {
        if (!s.plan.na) return;
        StageTimer timer(ctx_, CSTONE_STAGE_PLACE);
        hipLaunchKernelGGL((placeColumnsKernel<K, T, WHICH>), gridFor(s.plan.na, 256, PLACE_PER), 256, 0, ctx_->stream, s.keptO,
                           s.plan.nb ? posA_.as<uint32_t>() : nullptr, size_t(s.plan.na), s.keptKeys, s.x, s.y, s.z, s.h,
                           s.keysM, dst[0], dst[1], dst[2], dst[3]);
    }

    //! merge of the kept, already sorted range with the newcomers: positions, then every field from its input slot
    //! straight to its final slot
    int mergeAndPlace(SyncState& s)
    {
        Out& o            = *s.o;
        const uint64_t na = s.plan.na, nb = s.plan.nb, M = s.M;
        if (nb)
        {
            CS_TRY(posA_.ensure(ctx_, std::max<size_t>(na, 1) * sizeof(uint32_t)));
            CS_TRY(posB_.ensure(ctx_, nb * sizeof(uint32_t)));
            CS_TRY(cstone_hip_merge_positions(ctx_, kb, s.keptKeys, na, rk_.p, nb, 0, posA_.as<uint32_t>(),
                                              posB_.as<uint32_t>()));
            CS_TRY(cstone_hip_scatter(ctx_, sizeof(K), posB_.as<uint32_t>(), nb, rk_.p, s.keysM));
        }
        T* dst[4] = {o.x.as<T>() + M, o.y.as<T>() + M, o.z.as<T>() + M, o.h.as<T>() + M};
        // keys and h first: the locally essential tree and the halo discovery work on them.  x, y, z are not read before the
        // halo exchange: they go out on the context's second stream, next to the tree update, and are joined by joinPlace
        const bool overlap = useLet_ && overlapPlace_ && !s.massBits; // (syncGrav reads x, y, z for the mass centres)
        if (overlap) CS_TRY(ensureAuxStream(ctx_));
        if (overlap) placeColumns<1>(s, dst);
        else placeColumns<0>(s, dst);
        if (nb) CS_TRY(cstone_hip_scatter(ctx_, sizeof(T), posB_.as<uint32_t>(), nb, rcolS_[3].p, dst[3]));
        if (overlap)
        {
            CS_HIP(ctx_, hipEventRecord(ctx_->evFork, ctx_->stream));
            CS_HIP(ctx_, hipStreamWaitEvent(ctx_->aux, ctx_->evFork, 0));
            int rc = CSTONE_OK;
            {
                StreamScope scope(ctx_, ctx_->aux);
                placeColumns<2>(s, dst);
                for (int c = 0; c < 3 && nb && rc == CSTONE_OK; ++c)
                    rc = cstone_hip_scatter(ctx_, sizeof(T), posB_.as<uint32_t>(), nb, rcolS_[c].p, dst[c]);
            }
            CS_TRY(rc);
            CS_HIP(ctx_, hipEventRecord(ctx_->evJoin, ctx_->aux));
            placeForked_  = true;
            ctx_->sideBusy |= SIDE_AUX;
        }
        for (int c = 0; c < 3 && nb && !overlap; ++c)
            CS_TRY(cstone_hip_scatter(ctx_, sizeof(T), posB_.as<uint32_t>(), nb, rcolS_[c].p, dst[c]));
        for (int q = 0; q < s.numProps; ++q)
        {
            const int b = s.propBytes[q];
            char* to    = o.props[q].as<char>() + M * b;
            if (nb)
            {
                CS_TRY(cstone_hip_gather_scatter(ctx_, b, s.keptO, posA_.as<uint32_t>(), na, s.props[q], to));
                CS_TRY(cstone_hip_scatter(ctx_, b, posB_.as<uint32_t>(), nb, propRecvS_[q].p, to));
            }
            else { CS_TRY(cstone_hip_gather(ctx_, b, s.keptO, na, s.props[q], to)); }
        }
        return CSTONE_OK;
    }

    //! the pinned block the level ranges of this sync's tree travel to; the NEXT sync looks at it (takeLevelRanges)
    int ensureHostLevelRange()
    {
        if (!hostLevelRange_)
            CS_HIP(ctx_, hipHostMalloc(reinterpret_cast<void**>(&hostLevelRange_), 32 * sizeof(NodeIdx), hipHostMallocDefault));
        return CSTONE_OK;
    }

    //! The reference's way (R/domain/domain.hpp:217-237): peers, locally essential tree, halo discovery on it, key-range
    //! requests to the owners -- csrc/let.hpp, which carries the status word on its count exchanges.  h: in SFC order
    int updateLet(SyncState& s)
    {
        Out& o           = *s.o;
        const uint64_t M = s.M, nm = s.nm;
        if (!let_) let_ = std::make_unique<FocusLet<K, T>>(ctx_, curve_, rank_, P_, bucketFocus_, theta_, comm_);
        injectFailure("exchange");
        int rc;
        if (s.massBits)
        {
            const DevBuf& masses = o.props[s.numProps - 1];
            const char* mSorted  = masses.as<char>() + M * size_t(s.massBits / 8);
            rc = let_->updateGrav(box_, s.keysM, size_t(nm), assignment_.data(), gTree_.as<K>(), gHost_.leaves.data(),
                                  gCounts_.as<uint32_t>(), gLeaves_, o.x.as<T>() + M, o.y.as<T>() + M, o.z.as<T>() + M, mSorted,
                                  s.massBits, o.h.as<T>() + M, haloExt_, &centerDriftTol_, pending_ ? rank_ + 1 : 0, gTreeSame_);
            haveExpansionCenters_ = rc == CSTONE_OK;
        }
        else
        {
            rc = let_->update(box_, s.keysM, size_t(nm), assignment_.data(), gTree_.as<K>(), gCounts_.as<uint32_t>(),
                              gLeaves_, o.h.as<T>() + M, haloExt_, pending_ ? rank_ + 1 : 0, gTreeSame_);
            haveExpansionCenters_ = false;
        }
        if (rc != CSTONE_OK)
        {
            // (a failure of my own that the status word of the tree's last count exchange has told everybody about:
            //  reported with its own message)
            if (pending_) return agreed(rank_);
            if (toggled_) cur_ ^= 1, toggled_ = false;
            return rc;
        }
        if (uint64_t(let_->endIndex() - let_->startIndex()) != nm)
            return fail(ctx_, CSTONE_E_INTERNAL, "domain_mr_sync: the focus tree counts %u assigned particles, %llu are here",
                        let_->endIndex() - let_->startIndex(), (unsigned long long)nm);
        s.nlo      = let_->startIndex();
        s.nhi      = let_->numParticlesWithHalos() - let_->endIndex();
        s.haloAny  = 1;
        s.selTotal = let_->halosSent();
        // the leaves of my own range and their offsets among my particles: what the next sync's re-sort starts from
        s.first = let_->startCell(), s.last = let_->endCell();
        fLeaves_      = let_->numLeaves();
        resortTree_   = let_->leaves() + s.first;
        resortLeaves_ = s.last - s.first;
        CS_TRY(layout_.ensure(ctx_, size_t(resortLeaves_ + 1) * sizeof(uint32_t)));
        CS_TRY(cstone_hip_increment(ctx_, 32, let_->layout() + s.first, layout_.p, size_t(resortLeaves_) + 1,
                                    uint64_t(uint32_t(0u - uint32_t(s.nlo)))));
        layoutParticles_ = nm;
        layoutBox_       = box_;
        CS_TRY(ensureHostLevelRange());
        // (the level ranges came back with the layout: no copy of their own)
        std::copy(let_->levelRangeHost().begin(), let_->levelRangeHost().end(), hostLevelRange_);
        levelRangePending_ = true;
        return CSTONE_OK;
    }

    //! owner-side mode: the tree's level ranges to the pinned block (for the NEXT sync) and the layout of its leaves
    int layoutOwnTree(SyncState& s)
    {
        CS_TRY(ensureHostLevelRange());
        CS_TRY(copyToPinned(ctx_, hostLevelRange_, fLevelRange_.p, (maxLevel<K>() + 2) * sizeof(NodeIdx)));
        levelRangePending_ = true;
        const int L = fLeaves_;
        CS_TRY(layout_.ensure(ctx_, size_t(L + 1) * sizeof(uint32_t)));
        CS_HIP(ctx_, hipMemsetAsync(layout_.p, 0, sizeof(uint32_t), ctx_->stream));
        CS_TRY(cstone_hip_inclusive_scan_u32(ctx_, fCounts_.as<uint32_t>(), layout_.as<uint32_t>() + 1, size_t(L)));
        layoutParticles_ = s.nm; // the next sync's re-sort starts from this layout: nm particles in this box
        layoutBox_       = box_;
        resortTree_      = fTree_.as<K>();
        resortLeaves_    = fLeaves_;
        return CSTONE_OK;
    }

    //! C4, owner side.  Result: sel_ (what I send), s.hsCounts, s.hmatrix and what follows from it
    int discoverHalosOwnerSide(SyncState& s)
    {
        if (P_ > 1)
        {
            std::vector<uint64_t> boxCounts(P_);
            uint64_t maxBoxes = 0;
            CS_TRY(exportHaloBoxes(s, boxCounts, maxBoxes));
            CS_TRY(oflags_.ensure(ctx_, size_t(fLeaves_) * sizeof(int32_t)));
            if (maxBoxes && P_ <= 32 && !peerLoop_) { CS_TRY(overlapsAllPeers(s, maxBoxes)); }
            else
            {
                CS_TRY(overlapsPeerByPeer(s, boxCounts, maxBoxes));
                CS_TRY(countMatrix(s.hsCounts, s.hmatrix));
            }
        }
        s.haloAny = std::accumulate(s.hmatrix.begin(), s.hmatrix.end(), uint64_t(0));
        for (int p = 0; p < P_; ++p)
            if (p != rank_) (p < rank_ ? s.nlo : s.nhi) += s.hmatrix[size_t(p) * P_ + rank_];
        return CSTONE_OK;
    }

    //! my boxes to everybody: boxCounts[p] and the boxes of rank p in allBoxes_, each list padded to maxBoxes records
    int exportHaloBoxes(SyncState& s, std::vector<uint64_t>& boxCounts, uint64_t& maxBoxes)
    {
        const int first = s.first, last = s.last, nLocal = last - first, L = fLeaves_;
        CS_TRY(radii_.ensure(ctx_, size_t(L) * sizeof(float)));
        CS_TRY(boxes_.ensure(ctx_, size_t(std::max(nLocal, 1)) * 32));
        CS_TRY(boxFlags_.ensure(ctx_, size_t(nLocal + 1) * sizeof(uint32_t)));
        const DevBuf& h = s.o->h;
        CS_TRY(cstone_hip_halo_radii(ctx_, rb, h.as<T>() + s.M, layout_.as<uint32_t>() + first, first, last, L,
                                     haloExt_, radii_.as<float>()));
        // only boxes that really reach a leaf outside my range are exported (a third to a tenth of those the
        // enclosing-node test alone lets through: less to gather, fewer targets for every owner's traversal)
        CS_TRY(cstone_hip_halo_boxes_foreign(ctx_, curve_, kb, rb, fPrefixes_.p, fChild_.as<int32_t>(), fItl_.as<int32_t>(),
                                             fTree_.p, radii_.as<float>(), &box_, first, last, boxes_.as<int32_t>()));
        hipLaunchKernelGGL(boxFlagsKernel, gridFor(nLocal, 256), 256, 0, ctx_->stream, boxes_.as<int32_t>(), nLocal,
                           boxFlags_.as<uint32_t>());
        uint32_t* total = scanTotal();
        CS_TRY(exclusiveScanWithTotal(boxFlags_.as<uint32_t>(), nLocal, total));
        // box counts of everybody straight from the device scalar (one read-back for mine and theirs), then the boxes
        injectFailure("exchange");
        statusW32_ = pending_ ? 1u : 0u; // second word: the status of this rank (a member: an asynchronous copy reads it)
        CS_HIP(ctx_, hipMemcpyAsync(total + 1, &statusW32_, 4, hipMemcpyHostToDevice, ctx_->stream));
        CS_TRY(callComm(comm_.all_gather(comm_.user, total, gatherRecv(), 8), "all_gather (box counts)"));
        std::vector<uint32_t> c32(size_t(P_) * 2);
        CS_TRY(copyToHost(ctx_, c32.data(), gatherRecv(), c32.size() * 4));
        for (int p = 0; p < P_; ++p)
        {
            if (c32[2 * p + 1] != 0) return agreed(p);
            boxCounts[p] = c32[2 * p];
        }
        s.numMyBoxes = boxCounts[rank_];
        CS_TRY(myBoxes_.ensure(ctx_, size_t(std::max<uint64_t>(s.numMyBoxes, 1)) * 32));
        hipLaunchKernelGGL(compactBoxesKernel, gridFor(nLocal, 256), 256, 0, ctx_->stream, boxes_.as<int32_t>(),
                           boxFlags_.as<uint32_t>(), nLocal, rank_, myBoxes_.as<int32_t>());
        maxBoxes = *std::max_element(boxCounts.begin(), boxCounts.end());
        if (!maxBoxes) return CSTONE_OK;
        const size_t mine = s.numMyBoxes * 32, longest = maxBoxes * 32; // bytes
        CS_TRY(myBoxes_.ensure(ctx_, longest, true));
        if (longest > mine) // padding records must read "no box"
            CS_HIP(ctx_, hipMemsetAsync(myBoxes_.as<char>() + mine, 0, longest - mine, ctx_->stream));
        CS_TRY(allBoxes_.ensure(ctx_, longest * P_));
        return callComm(comm_.all_gather(comm_.user, myBoxes_.p, allBoxes_.p, longest), "all_gather (halo boxes)");
    }

    //! marks in oflags_ the leaves of [s.first, s.last) that one of numBoxes records touches
    int findOverlaps(const SyncState& s, const int32_t* boxes, size_t numBoxes)
    {
        return cstone_hip_find_overlaps(ctx_, curve_, kb, fPrefixes_.p, fChild_.as<int32_t>(), fItl_.as<int32_t>(), fTree_.p,
                                        boxes, int(numBoxes), s.first, s.last, oflags_.as<int32_t>());
    }

    //! all peers in one go: find_overlaps sets one bit per exporter (two calls: the records before and behind my own);
    //! then counts, one scan, one fill.  My row of the count matrix goes from the device into the all-gather; one read-back
    int overlapsAllPeers(SyncState& s, uint64_t maxBoxes)
    {
        const int first = s.first, last = s.last, nLocal = last - first, np = P_ - 1;
        CS_HIP(ctx_, hipMemsetAsync(oflags_.p, 0, size_t(fLeaves_) * sizeof(int32_t), ctx_->stream));
        if (rank_ > 0) CS_TRY(findOverlaps(s, allBoxes_.as<int32_t>(), size_t(rank_) * maxBoxes));
        if (rank_ + 1 < P_)
            CS_TRY(findOverlaps(s, allBoxes_.as<int32_t>() + size_t(rank_ + 1) * maxBoxes * 8,
                                size_t(P_ - rank_ - 1) * maxBoxes));
        const size_t items = size_t(np) * nLocal;
        CS_TRY(cnt_.ensure(ctx_, (items + 1) * sizeof(uint32_t)));
        hipLaunchKernelGGL(peerCountsKernel, gridFor(nLocal, 256), 256, 0, ctx_->stream, oflags_.as<int32_t>(),
                           layout_.as<uint32_t>(), first, last, P_, rank_, cnt_.as<uint32_t>());
        CS_TRY(exclusiveScanWithTotal(cnt_.as<uint32_t>(), int(items), scanTotal()));
        hipLaunchKernelGGL(peerTotalsKernel, 1, 64, 0, ctx_->stream, cnt_.as<uint32_t>(), scanTotal(), nLocal, np, rank_,
                           gatherRow());
        CS_TRY(callComm(comm_.all_gather(comm_.user, gatherRow(), gatherRecv(), size_t(P_) * 8),
                        "all_gather (halo counts)"));
        CS_TRY(copyToHost(ctx_, s.hmatrix.data(), gatherRecv(), size_t(P_) * P_ * 8));
        std::copy_n(s.hmatrix.begin() + size_t(rank_) * P_, P_, s.hsCounts.begin());
        s.selTotal = std::accumulate(s.hsCounts.begin(), s.hsCounts.end(), uint64_t(0));
        if (!s.selTotal) return CSTONE_OK;
        CS_TRY(sel_.ensure(ctx_, s.selTotal * sizeof(uint32_t)));
        hipLaunchKernelGGL(peerFillKernel, gridFor(items, 16), 256, 0, ctx_->stream, oflags_.as<int32_t>(),
                           layout_.as<uint32_t>(), cnt_.as<uint32_t>(), first, last, P_, rank_, sel_.as<uint32_t>());
        return CSTONE_OK;
    }

    //! more than 32 ranks (or CSTONE_MR_PEER_LOOP): one traversal, one scan, one read-back and one fill per peer
    int overlapsPeerByPeer(SyncState& s, const std::vector<uint64_t>& boxCounts, uint64_t maxBoxes)
    {
        const int first = s.first, last = s.last, nLocal = last - first;
        CS_TRY(cnt_.ensure(ctx_, size_t(nLocal + 1) * sizeof(uint32_t)));
        for (int p = 0; p < P_; ++p)
        {
            if (p == rank_ || boxCounts[p] == 0) continue;
            CS_HIP(ctx_, hipMemsetAsync(oflags_.p, 0, size_t(fLeaves_) * sizeof(int32_t), ctx_->stream));
            CS_TRY(findOverlaps(s, allBoxes_.as<int32_t>() + size_t(p) * maxBoxes * 8, boxCounts[p]));
            hipLaunchKernelGGL(flaggedCountsKernel, gridFor(nLocal, 256), 256, 0, ctx_->stream, oflags_.as<int32_t>(),
                               layout_.as<uint32_t>(), first, last, cnt_.as<uint32_t>());
            CS_TRY(exclusiveScanWithTotal(cnt_.as<uint32_t>(), nLocal, scanTotal()));
            uint32_t tp = 0;
            CS_TRY(copyToHost(ctx_, &tp, scanTotal(), 4));
            if (tp)
            {
                CS_TRY(sel_.ensure(ctx_, (s.selTotal + tp) * sizeof(uint32_t), true));
                hipLaunchKernelGGL(fillIndicesKernel, gridFor(nLocal, 16), 256, 0, ctx_->stream, oflags_.as<int32_t>(),
                                   layout_.as<uint32_t>(), cnt_.as<uint32_t>(), first, last,
                                   sel_.as<uint32_t>() + s.selTotal);
            }
            s.hsCounts[p] = tp;
            s.selTotal += tp;
        }
        return CSTONE_OK;
    }

    //! x, y, z of the assigned block are needed from here on (a block that has to be moved, the halo exchange)
    int joinPlace()
    {
        if (!placeForked_) return CSTONE_OK;
        CS_HIP(ctx_, hipStreamWaitEvent(ctx_->stream, ctx_->evJoin, 0));
        placeForked_  = false;
        ctx_->sideBusy &= ~SIDE_AUX;
        return CSTONE_OK;
    }

    //! the assigned block of one result array from slot s.M to slot M2 of an array of cap2 elements, through a scratch copy
    int shiftBlock(const SyncState& s, DevBuf& buf, size_t elem, uint64_t M2, uint64_t cap2)
    {
        const size_t bytes = s.nm * elem;
        CS_TRY(moveTmp_.ensure(ctx_, bytes));
        CS_HIP(ctx_, hipMemcpyAsync(moveTmp_.p, buf.as<char>() + s.M * elem, bytes, hipMemcpyDeviceToDevice, ctx_->stream));
        CS_TRY(buf.ensure(ctx_, cap2 * elem));
        CS_HIP(ctx_, hipMemcpyAsync(buf.as<char>() + M2 * elem, moveTmp_.p, bytes, hipMemcpyDeviceToDevice, ctx_->stream));
        return CSTONE_OK;
    }

    //! room for the halos on both sides of the assigned block (blockWithHalos, host_rules.hpp); margins that were too small
    //! (first syncs, abrupt changes): the block is moved once
    int makeRoomForHalos(SyncState& s)
    {
        const BlockWithHalos b = blockWithHalos(s.M, s.cap, s.nm, s.nlo, s.nhi);
        if (b.move)
        {
            Out& o = *s.o;
            CS_TRY(shiftBlock(s, o.keys, sizeof(K), b.M2, b.cap2));
            for (DevBuf* f : {&o.x, &o.y, &o.z, &o.h})
                CS_TRY(shiftBlock(s, *f, sizeof(T), b.M2, b.cap2));
            for (int q = 0; q < s.numProps; ++q)
                CS_TRY(shiftBlock(s, o.props[q], size_t(s.propBytes[q]), b.M2, b.cap2));
        }
        s.off   = b.off;
        prevLo_ = s.nlo, prevHi_ = s.nhi;
        return CSTONE_OK;
    }

    //! keys of `count` halo particles from slot `start` on (encode skips entries that hold the remove marker: clear first)
    int encodeHaloKeys(Out& o, uint64_t start, uint64_t count)
    {
        if (!count) return CSTONE_OK;
        CS_HIP(ctx_, hipMemsetAsync(o.keys.as<K>() + start, 0, count * sizeof(K), ctx_->stream));
        return cstone_hip_compute_sfc_keys(ctx_, curve_, kb, rb, o.x.as<T>() + start, o.y.as<T>() + start,
                                           o.z.as<T>() + start, o.keys.as<K>() + start, count, &box_);
    }

    //! C5: halos below | assigned | halos above; x, y, z and h travel together, then the keys of the halo particles
    int exchangeHaloParticles(SyncState& s)
    {
        Out& o           = *s.o;
        const uint64_t off = s.off, nlo = s.nlo, nhi = s.nhi, A = off + nlo, B = A + s.nm; // A: assigned, B: upper halos
        if (P_ > 1 && useLet_)
        {
            // in the order of the focus tree's leaves (R/domain/domain.hpp:522-540), one message per peer instead of four
            void* xyzh[4] = {o.x.as<T>() + off, o.y.as<T>() + off, o.z.as<T>() + off, o.h.as<T>() + off};
            CS_TRY(let_->exchangeHalosRows(xyzh, 4, int(sizeof(T))));
        }
        else if (P_ > 1 && s.haloAny)
        {
            CS_TRY(sendRows_.ensure(ctx_, std::max<size_t>(s.selTotal, 1) * 4 * sizeof(T)));
            CS_TRY(recvRows_.ensure(ctx_, std::max<size_t>(nlo + nhi, 1) * 4 * sizeof(T)));
            if (s.selTotal)
                hipLaunchKernelGGL(packRowsKernel<T>, gridFor(s.selTotal, 256), 256, 0, ctx_->stream, sel_.as<uint32_t>(),
                                   size_t(s.selTotal), o.x.as<T>() + A, o.y.as<T>() + A, o.z.as<T>() + A, o.h.as<T>() + A,
                                   sendRows_.as<T>());
            const std::vector<size_t> sb = peerBytes(s.hsCounts.data(), 1, 4 * sizeof(T)),
                                      rbv = peerBytes(s.hmatrix.data() + rank_, P_, 4 * sizeof(T));
            CS_TRY(callComm(comm_.all_to_all_v(comm_.user, sendRows_.p, sb.data(), recvRows_.p, rbv.data()), "all_to_all_v (halos)"));
            if (nlo)
                hipLaunchKernelGGL(unpackRowsKernel<T>, gridFor(nlo, 256), 256, 0, ctx_->stream, recvRows_.as<T>(), size_t(nlo),
                                   o.x.as<T>() + off, o.y.as<T>() + off, o.z.as<T>() + off, o.h.as<T>() + off);
            if (nhi)
                hipLaunchKernelGGL(unpackRowsKernel<T>, gridFor(nhi, 256), 256, 0, ctx_->stream, recvRows_.as<T>() + 4 * nlo,
                                   size_t(nhi), o.x.as<T>() + B, o.y.as<T>() + B, o.z.as<T>() + B, o.h.as<T>() + B);
        }
        if (P_ > 1 && (useLet_ || s.haloAny))
        {
            CS_TRY(encodeHaloKeys(o, off, nlo));
            CS_TRY(encodeHaloKeys(o, B, nhi));
        }
        CS_HIP(ctx_, hipGetLastError());
        return CSTONE_OK;
    }

    //! the bookkeeping reapplySync / exchangeHalos / octree() work from, and the view
    int finishSync(SyncState& s)
    {
        const ExchangePlan& e = s.plan;
        const Out& o          = *s.o;
        const uint64_t off = s.off, nlo = s.nlo, nhi = s.nhi, nm = s.nm;
        // the particle routes of this sync (reapplySync)
        rsN_ = s.n, rsNa_ = e.na, rsNb_ = e.nb, rsSend_ = e.mSend, rsMoved_ = e.movedAny, rsKeptOffset_ = s.cut[rank_];
        rsSendCounts_ = e.sendCounts;
        haloAnyLast_ = s.haloAny;
        haloSend_ = s.hsCounts, haloRecvLo_ = nlo, haloRecvHi_ = nhi, haloAssigned_ = nm, haloSel_ = s.selTotal;
        rsRecvCounts_.assign(P_, 0), haloRecv_.assign(P_, 0); // (what the others send me: my column of the two matrices)
        for (int p = 0; p < P_; ++p)
            if (p != rank_) rsRecvCounts_[p] = e.matrix[size_t(p) * P_ + rank_], haloRecv_[p] = s.hmatrix[size_t(p) * P_ + rank_];

        firstCall_                     = false;
        view_.start_index              = uint32_t(nlo);
        view_.end_index                = uint32_t(nlo + nm);
        view_.num_particles_with_halos = uint32_t(nlo + nm + nhi);
        view_.box                      = box_;
        view_.keys = o.keys.as<K>() + off;
        view_.x = o.x.as<T>() + off, view_.y = o.y.as<T>() + off, view_.z = o.z.as<T>() + off, view_.h = o.h.as<T>() + off;
        for (int q = 0; q < MAX_PROPS; ++q)
            view_.props[q] = q < s.numProps ? static_cast<const void*>(o.props[q].as<char>() + off * s.propBytes[q]) : nullptr;
        view_.num_global_leaves = gLeaves_, view_.num_focus_leaves = fLeaves_;
        view_.global_leaves = gTree_.p, view_.global_counts = gCounts_.as<uint32_t>();
        view_.focus_leaves = fTree_.p, view_.focus_leaf_counts = fCounts_.as<uint32_t>();
        view_.start_cell = 0, view_.end_cell = fLeaves_, view_.num_peers = 0;
        view_.layout = nullptr, view_.halo_flags = nullptr;
        if (useLet_)
        {
            view_.focus_leaves = let_->leaves(), view_.focus_leaf_counts = let_->leafCounts();
            view_.start_cell = let_->startCell(), view_.end_cell = let_->endCell();
            view_.num_peers  = int32_t(let_->peers().size());
            view_.layout = let_->layout(), view_.halo_flags = let_->haloFlags();
        }
        view_.range_start = uint64_t(assignment_[rank_]), view_.range_end = uint64_t(assignment_[rank_ + 1]);
        view_.particles_sent      = e.mSend;
        view_.halos_received      = nlo + nhi;
        view_.halos_sent          = s.selTotal;
        view_.halo_boxes_exported = s.numMyBoxes;
        view_.resorts             = uint64_t(resorts_);
        // the sticky device-side error word: a sync that tripped a device-side check must not report success
        CS_TRY(cstone_hip_ctx_sync(ctx_));
        viewSync_ = syncs_;
        return CSTONE_OK;
    }

    //! CSTONE_MR_TIMING=1: synchronising wall clock per phase, printed by rank 0 when the domain is destroyed
    void tick(const char* name)
    {
        if (!timing_) return;
        (void)hipStreamSynchronize(ctx_->stream);
        auto now = std::chrono::steady_clock::now();
        if (name) phase_[name] += std::chrono::duration<double>(now - t0_).count();
        t0_ = now;
    }

    //! a failure of THIS rank that the peers must learn about before anybody returns (see the top of sync())
    void setPending(int code, const char* fmt, ...)
    {
        if (pending_) return;
        char buf[384];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        pending_    = code;
        pendingMsg_ = buf;
    }

    /*! below some 6e6 particles per rank the chain of small launches of the re-sort and its read-back cost more than the
     *  digit passes they replace: measured in round 3, every particle drifting, re-sorted against radix-sorted: 0.73 / 0.60
     *  ms per sync at 1e6, 0.91 / 0.90 at 3e6, 0.90 / 0.95 at 6e6, 1.49 / 1.53 at 1.25e7, 2.62 / 2.66 at 2.5e7, 3.36 / 3.7
     *  at 5e7 (tools/mr_bench.py --rccl) */
    static size_t resortMinParticles()
    {
        static const size_t v = []
        {
            const char* e = std::getenv("CSTONE_MR_RESORT_MIN");
            return e ? size_t(std::strtoull(e, nullptr, 10)) : size_t(6) << 20;
        }();
        return v;
    }

    //! tests: CSTONE_MR_FAIL_AT="<rank>:<point>" makes that rank fail at the named point of sync()
    void injectFailure(const char* point)
    {
#ifdef CSTONE_TEST_HOOKS // (the product library carries no fault injection: lib/libcstone_hip_hooks.so is the tests' build)
        const char* e = std::getenv("CSTONE_MR_FAIL_AT");
        if (!e) return;
        const std::string want = std::to_string(rank_) + ":" + point;
        if (want == e) setPending(CSTONE_E_INTERNAL, "domain_mr_sync: failure injected at '%s'", point);
#else
        (void)point;
#endif
    }

    //! every rank has seen that rank `culprit` failed: all of them return an error from the same point of the sync
    int agreed(int culprit)
    {
        const int code      = culprit == rank_ && pending_ ? pending_ : CSTONE_E_INTERNAL;
        const std::string m = culprit == rank_ ? pendingMsg_ : "rank " + std::to_string(culprit) + " reported a failure";
        pending_            = 0;
        if (toggled_) cur_ ^= 1, toggled_ = false; // the client's arrays of the last good sync stay untouched by the next one
        resortTree_ = nullptr, resortLeaves_ = 0, layoutParticles_ = 0; // an abandoned sync is nothing to re-sort from
        return fail(ctx_, code, "%s (the sync was abandoned on every rank)", m.c_str());
    }

    int callComm(int rc, const char* what)
    {
        return rc == 0 ? CSTONE_OK : fail(ctx_, CSTONE_E_INTERNAL, "collective %s failed with code %d", what, rc);
    }

    int ensureSortScratch(size_t n)
    {
        CS_TRY(keysAlt_.ensure(ctx_, n * sizeof(K)));
        CS_TRY(orderAlt_.ensure(ctx_, n * sizeof(uint32_t)));
        CS_TRY(sortTmp_.ensure(ctx_, cstone_hip_sort_pairs_temp_bytes(kb, n)));
        return CSTONE_OK;
    }

    //! in-place exclusive scan of n values, grand total to *totalDev
    int exclusiveScanWithTotal(uint32_t* data, int n, uint32_t* totalDev)
    {
        if (n == 0)
        {
            CS_HIP(ctx_, hipMemsetAsync(totalDev, 0, 4, ctx_->stream));
            return CSTONE_OK;
        }
        CS_TRY(arenaReserve(ctx_, scanArenaBytes(size_t(n))));
        int rc = scanU32(ctx_, data, data, size_t(n), 0u, false, totalDev);
        arenaReset(ctx_);
        return rc;
    }

    //! m[src * P + dst] of every rank's counts
    int countMatrix(const std::vector<uint64_t>& mine, std::vector<uint64_t>& matrix)
    {
        matrix.assign(size_t(P_) * P_, 0);
        if (P_ == 1) matrix[0] = mine[0];
        // (staged by the runtime's copy, not by stageRow: the owner-side sync keeps its sequence of calls)
        else CS_HIP(ctx_, hipMemcpyAsync(gatherRow(), mine.data(), size_t(P_) * 8, hipMemcpyHostToDevice, ctx_->stream));
        return gatherRows(P_, "all_gather (counts)", matrix);
    }

    // ---- C1
    int updateBox(const T* x, const T* y, const T* z, size_t n)
    {
        // periodic axes keep their limits (R/sfc/box_mpi.hpp:81-121): with three of them there is nothing to measure
        if (box_.bc[0] == 1 && box_.bc[1] == 1 && box_.bc[2] == 1) return CSTONE_OK;
        // (lo, -hi) per axis stay on the device from the reduction over the particles through the MIN all-reduce over
        // the ranks; one read-back at the end
        static const double inf = std::numeric_limits<double>::infinity(), nothing[6] = {inf, inf, inf, inf, inf, inf};
        double* dev = boxOperand();
        if (n)
        {
            const void* arrays[3] = {x, y, z};
            CS_TRY(minMaxCoordinatesDev(ctx_, rb, arrays, 3, n, dev));
        }
        else { CS_HIP(ctx_, hipMemcpyAsync(dev, nothing, sizeof nothing, hipMemcpyHostToDevice, ctx_->stream)); }
        cstone_box next;
        CS_TRY(reduceBox(dev, &next));
        box_ = next;
        return CSTONE_OK;
    }

    //! seventh value of the box reduction: the status of this rank (0, or -(rank + 1) if it has a failure pending)
    double statusWord() const { return pending_ ? -double(rank_ + 1) : 0.0; }

    /*! MIN over the ranks of dev[0..6] = (min, -max) per axis + status, read back and put through the box rule: box_ ->
     *  *next (box_ itself is not changed).  statusSet: the operand is complete (the kernel
     *  that wrote the extents wrote the status too); counters: four ints behind the operand come back in the same copy */
    int reduceBox(double* dev, cstone_box* next, bool statusSet = false, int* counters = nullptr)
    {
        if (!statusSet)
        {
            const double status = statusWord();
            CS_TRY(cstone_hip_upload(ctx_, dev + 6, &status, sizeof status));
        }
        if (P_ > 1) CS_TRY(callComm(comm_.all_reduce(comm_.user, dev, 7, 0, 1), "all_reduce (box)"));
        double ext[9];
        CS_TRY(copyToHost(ctx_, ext, dev, counters ? sizeof ext : 7 * sizeof(double)));
        if (counters) std::memcpy(counters, ext + 7, 4 * sizeof(int));
        if (ext[6] < 0) return agreed(int(-ext[6]) - 1);
        double fit[6]; // (lo, -hi) -> {min, max}; limitBoxShrinking keeps the limits of the periodic axes
        for (int d = 0; d < 3; ++d)
            fit[2 * d] = ext[2 * d], fit[2 * d + 1] = -ext[2 * d + 1];
        *next = limitBoxShrinking<T>(box_, fit, firstCall_);
        return CSTONE_OK;
    }

    //! the counts of the global tree summed over the ranks, and no smaller than this rank's own (maxWithLocalKernel)
    int allReduceGlobalCounts()
    {
        if (P_ == 1) return CSTONE_OK;
        CS_TRY(gLocalCounts_.ensure(ctx_, size_t(gLeaves_) * sizeof(uint32_t)));
        CS_HIP(ctx_, hipMemcpyAsync(gLocalCounts_.p, gCounts_.p, size_t(gLeaves_) * sizeof(uint32_t),
                                    hipMemcpyDeviceToDevice, ctx_->stream));
        CS_TRY(callComm(comm_.all_reduce(comm_.user, gCounts_.p, size_t(gLeaves_), 1, 0), "all_reduce (counts)"));
        hipLaunchKernelGGL(maxWithLocalKernel, gridFor(size_t(gLeaves_), 256), 256, 0, ctx_->stream,
                           gCounts_.as<uint32_t>(), gLocalCounts_.as<uint32_t>(), gLeaves_);
        return CSTONE_OK;
    }

    // ---- C2: GlobalAssignment ctor + assign() tree part
    int updateGlobalTree(size_t n)
    {
        if (gLeaves_ == 0)
        {
            std::vector<K> init = initialGlobalTree<K>(P_);
            int leaves          = int(init.size()) - 1;
            CS_TRY(ensureTree<K>(ctx_, gTree_, gCounts_, gCap_, std::max(4096, 2 * leaves)));
            std::vector<uint32_t> c0(leaves, bucket_ - 1);
            CS_HIP(ctx_, hipMemcpy(gTree_.p, init.data(), init.size() * sizeof(K), hipMemcpyHostToDevice));
            CS_HIP(ctx_, hipMemcpy(gCounts_.p, c0.data(), c0.size() * 4, hipMemcpyHostToDevice));
            gLeaves_ = leaves;
        }
        if (!firstCall_ && hostGlobalStep_ && gHost_.matches(gLeaves_))
        {
            // later calls take exactly ONE update step (assignment.hpp:92-98).  The tree is small and replicated and the
            // host holds its leaves and the all-reduced counts of the last sync (assign() read them): the decision and the
            // new leaf array are made here; the device counts this rank's keys, the counts are reduced, and assign() reads
            // them back together with everything else the sync needs at that point -- no read-back in between
            CS_TRY(gHost_.stepOnHost(ctx_, bucket_, gTree_, gCounts_, gCap_, gLeaves_, &gTreeSame_));
            CS_TRY(cstone_hip_compute_node_counts(ctx_, kb, gTree_.p, gCounts_.as<uint32_t>(), gLeaves_, keys_.p, n,
                                                  0xFFFFFFFFu));
            CS_TRY(allReduceGlobalCounts());
            gLeavesOnHost_ = true;
            return CSTONE_OK;
        }
        gLeavesOnHost_ = false;
        int steps = 0;
        while (true)
        {
            int conv = 0;
            CS_TRY(updateOctreeGrowing<K>(ctx_, keys_.p, n, bucket_, gTree_, gCounts_, gCap_, gLeaves_, &conv));
            gTreeSame_ = steps == 0 && !firstCall_ && conv != 0; // the one step of a later sync kept every leaf
            CS_TRY(allReduceGlobalCounts());
            ++steps;
            // later calls: exactly one step; first call: one step, then `while (!update)` (assignment.hpp:92-98)
            if (!firstCall_ || (steps >= 2 && conv)) break;
            if (steps > 64) return fail(ctx_, CSTONE_E_INTERNAL, "global tree does not converge");
        }
        return CSTONE_OK;
    }

    //! makeSfcAssignment + limitBoundaryShifts from the host copies of the global tree (after the read-back completed)
    int assign()
    {
        const std::vector<uint32_t>& counts = gHost_.counts;
        const std::vector<K>& leaves        = gHost_.leaves;
        std::vector<int> bins = uniformBinsHost(counts, P_);
        std::vector<K> fresh(P_ + 1);
        for (int r = 0; r <= P_; ++r)
            fresh[r] = leaves[bins[r]];
        if (int(assignment_.size()) == P_ + 1)
        {
            // limitBoundaryShifts (domaindecomp.hpp:140-172): a boundary moves at most into a neighbour's old range
            std::vector<K> old = assignment_;
            for (int r = 1; r < P_; ++r)
                fresh[r] = std::min(std::max(fresh[r], old[r - 1]), old[r + 1]);
        }
        assignment_ = fresh;
        return CSTONE_OK;
    }

    int updateFocusTree(const K* keysM, size_t nm)
    {
        if (fLeaves_ == 0)
        {
            const int cap = std::max<int>(4096, int(4 * nm / std::max(1u, bucketFocus_)) + 4096);
            treeSteps_    = 0;
            return computeOctreeGrowing<K>(ctx_, keysM, nm, bucketFocus_, fTree_, fCounts_, fCap_, cap, fLeaves_);
        }
        ++treeSteps_;
        int conv = 0;
        return updateOctreeGrowing<K>(ctx_, keysM, nm, bucketFocus_, fTree_, fCounts_, fCap_, fLeaves_, &conv);
    }

    /*! The rank's SFC range must start and end on leaf boundaries of its own tree (the job of enforceKeys in the
     *  reference's focus tree, R/focus/rebalance.hpp:199-266): a leaf that straddles a range boundary is replaced by the
     *  coarsest set of octree nodes that resolves the boundary key.  Such leaves are mostly empty, so the count-driven
     *  update merges them again and the split is redone at every sync: a copy of the leaf array and a recount.
     *  One device query and ONE read-back serve both boundaries; the leaf range [*first, *last) of the rank in the
     *  resulting tree follows on the host. */
    int enforceBoundaries(const K* keysM, size_t nm, int* first, int* last)
    {
        const uint64_t end = uint64_t(endKey<K>());
        const uint64_t b[2] = {uint64_t(assignment_[rank_]), uint64_t(assignment_[rank_ + 1])};
        uint64_t* dq = leafQuery();
        hipLaunchKernelGGL(containingLeavesKernel<K>, 1, 64, 0, ctx_->stream, fTree_.as<K>(), fLeaves_,
                           K(std::min(b[0], end)), K(std::min(b[1], end)), dq);
        uint64_t q[6];
        CS_TRY(copyToHost(ctx_, q, dq, sizeof q));
        const int L = fLeaves_;
        // leaves to replace, in ascending order: (index, start, end, boundary keys strictly inside)
        struct Cut
        {
            int idx;
            uint64_t s, e;
            std::vector<uint64_t> keys;
        };
        std::vector<Cut> cuts;
        for (int k = 0; k < 2; ++k)
        {
            const int idx = int(q[3 * k]);
            if (b[k] == 0 || b[k] >= end || idx >= L || q[3 * k + 1] == b[k]) continue; // already a leaf boundary
            if (!cuts.empty() && cuts.back().idx == idx) { cuts.back().keys.push_back(b[k]); }
            else { cuts.push_back({idx, q[3 * k + 1], q[3 * k + 2], {b[k]}}); }
        }
        // position of a boundary key in the new leaf array: leaves before it in the old array + what the covers add
        coverHost_.clear();
        coverDeepest_ = 0;
        std::vector<int> coverBegin, coverSize;
        for (const Cut& c : cuts)
        {
            coverBegin.push_back(int(coverHost_.size()));
            uint64_t a = c.s;
            for (uint64_t key : c.keys)
            {
                appendCover(coverHost_, a, key);
                a = key;
            }
            appendCover(coverHost_, a, c.e);
            coverSize.push_back(int(coverHost_.size()) - coverBegin.back());
            // how deep the inserted leaves go (the sort of the node keys in buildFocusOctree leaves out the digit passes
            // above the deepest level of the tree)
            for (int i = 0; i < coverSize.back(); ++i)
            {
                const uint64_t lo   = uint64_t(coverHost_[coverBegin.back() + i]);
                const uint64_t hi   = i + 1 < coverSize.back() ? uint64_t(coverHost_[coverBegin.back() + i + 1]) : c.e;
                const uint64_t span = hi - lo;
                int level           = 0;
                while (level < int(maxLevel<K>()) && (uint64_t(1) << (3 * (maxLevel<K>() - level))) > span)
                    ++level;
                coverDeepest_ = std::max(coverDeepest_, level);
            }
        }
        auto newIndexOf = [&](uint64_t key, int containing, bool aligned) -> int
        {
            if (key == 0) return 0;
            int shift = 0;
            for (size_t c = 0; c < cuts.size(); ++c)
            {
                if (cuts[c].idx < containing) { shift += coverSize[c] - 1; }
                else if (cuts[c].idx == containing && !aligned)
                {
                    const K* cb = coverHost_.data() + coverBegin[c];
                    return containing + shift + int(std::find(cb, cb + coverSize[c], K(key)) - cb);
                }
            }
            return containing + shift;
        };
        int extra = 0;
        for (int sz : coverSize)
            extra += sz - 1;
        const int newL = L + extra;
        *first = newIndexOf(b[0], int(q[0]), b[0] == 0 || q[1] == b[0]);
        *last  = b[1] >= end ? newL : newIndexOf(b[1], int(q[3]), q[4] == b[1]);
        if (!cuts.empty())
        {
            CS_TRY(ensureTree<K>(ctx_, fTree_, fCounts_, fCap_, newL));
            CS_TRY(fTmp_.ensure(ctx_, size_t(newL + 1) * sizeof(K)));
            K* t        = fTmp_.as<K>();
            const K* ft = fTree_.as<K>();
            int src = 0, dst = 0; // old leaves [src, ...) still to copy, new position dst
            for (size_t c = 0; c < cuts.size(); ++c)
            {
                const int keep = cuts[c].idx - src;
                if (keep)
                    CS_HIP(ctx_, hipMemcpyAsync(t + dst, ft + src, size_t(keep) * sizeof(K), hipMemcpyDeviceToDevice,
                                                ctx_->stream));
                dst += keep;
                // coverHost_ is a member: it outlives the copy (the next sync refills it behind a stream sync)
                CS_HIP(ctx_, hipMemcpyAsync(t + dst, coverHost_.data() + coverBegin[c], size_t(coverSize[c]) * sizeof(K),
                                            hipMemcpyHostToDevice, ctx_->stream));
                dst += coverSize[c];
                src = cuts[c].idx + 1;
            }
            CS_HIP(ctx_, hipMemcpyAsync(t + dst, ft + src, size_t(L + 1 - src) * sizeof(K), hipMemcpyDeviceToDevice,
                                        ctx_->stream));
            CS_HIP(ctx_, hipMemcpyAsync(fTree_.p, t, size_t(newL + 1) * sizeof(K), hipMemcpyDeviceToDevice,
                                        ctx_->stream));
            fLeaves_ = newL;
            CS_TRY(cstone_hip_compute_node_counts(ctx_, kb, fTree_.p, fCounts_.as<uint32_t>(), fLeaves_, keysM, nm,
                                                  0xFFFFFFFFu));
        }
        if (*first < 0 || *last > fLeaves_ || *last <= *first)
            return fail(ctx_, CSTONE_E_INTERNAL, "domain_mr_sync: bad leaf range [%d, %d) of %d", *first, *last, fLeaves_);
        return CSTONE_OK;
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
        // leaves of the new tree: at most one level below the deepest of the previous sync's tree (one update step), or as
        // deep as the leaves inserted at the range boundaries; the first tree of a domain may be of any depth
        const int deepest = (treeSteps_ > 0 && prevMaxLeafLevel_ >= 0) ? std::max(prevMaxLeafLevel_ + 1, coverDeepest_)
                                                                       : int(maxLevel<K>());
        return buildLinkedOctree(ctx_, kb, fTree_.p, L, fPrefixes_.p, fChild_.as<int32_t>(), fParents_.as<int32_t>(),
                                 fLevelRange_.as<int32_t>(), fItl_.as<int32_t>(), fLti_.as<int32_t>(), deepest);
    }

    int buildNsTree()
    {
        const K* keysAll = static_cast<const K*>(view_.keys);
        const size_t n   = view_.num_particles_with_halos;
        if (nsLeaves_ == 0)
        {
            const int cap = std::max<int>(4096, int(4 * n / std::max(1u, bucketFocus_)) + 4096);
            CS_TRY(computeOctreeGrowing<K>(ctx_, keysAll, n, bucketFocus_, nsTree_, nsCounts_, nsCap_, cap, nsLeaves_));
        }
        else
        {
            // the particles moved a little since the last request: a few update steps (each one level of splits or
            // merges, R/tree/csarray.hpp:430-448); the search stays correct if the last one still changed something
            for (int it = 0, conv = 0; it < 4 && !conv; ++it)
                CS_TRY(updateOctreeGrowing<K>(ctx_, keysAll, n, bucketFocus_, nsTree_, nsCounts_, nsCap_, nsLeaves_, &conv));
        }
        const NodeIdx L = nsLeaves_, M = L + (L - 1) / 7;
        CS_TRY(nsLayout_.ensure(ctx_, size_t(L + 1) * sizeof(uint32_t)));
        CS_HIP(ctx_, hipMemsetAsync(nsLayout_.p, 0, sizeof(uint32_t), ctx_->stream));
        CS_TRY(cstone_hip_inclusive_scan_u32(ctx_, nsCounts_.as<uint32_t>(), nsLayout_.as<uint32_t>() + 1, size_t(L)));
        CS_TRY(nsPrefixes_.ensure(ctx_, size_t(M) * sizeof(K)));
        CS_TRY(nsChild_.ensure(ctx_, size_t(M + 1) * sizeof(NodeIdx)));
        CS_TRY(nsParents_.ensure(ctx_, size_t(std::max(1, (M - 1) / 8)) * sizeof(NodeIdx)));
        CS_TRY(nsLevelRange_.ensure(ctx_, (maxLevel<K>() + 2) * sizeof(NodeIdx)));
        CS_TRY(nsItl_.ensure(ctx_, size_t(M) * sizeof(NodeIdx)));
        CS_TRY(nsLti_.ensure(ctx_, size_t(M) * sizeof(NodeIdx)));
        CS_TRY(cstone_hip_build_octree(ctx_, kb, nsTree_.p, L, nsPrefixes_.p, nsChild_.as<int32_t>(),
                                       nsParents_.as<int32_t>(), nsLevelRange_.as<int32_t>(), nsItl_.as<int32_t>(),
                                       nsLti_.as<int32_t>()));
        CS_TRY(nsCenters_.ensure(ctx_, size_t(M) * 3 * sizeof(T)));
        CS_TRY(nsSizes_.ensure(ctx_, size_t(M) * 3 * sizeof(T)));
        return cstone_hip_node_centers(ctx_, curve_, kb, rb, nsPrefixes_.p, M, &box_, nsCenters_.p, nsSizes_.p);
    }

    // ---- What the collective analyses (friendsOfFriends, fofCatalog, sphereProfiles) share: DESIGN.md, section 5f,
    //      "The agreement the collective analyses share"

    //! Rank-local trouble of an analysis, the status word of its all-gather; also the order of every call's table of texts
    enum Trouble : uint64_t { FINE, NULL_ARRAY, STALE_SYNC, NO_MEMORY, BAD_LABEL, LOCAL_STEP, MISMATCH, NUM_TROUBLES };
    static int troubleCode(uint64_t t) { return t == NO_MEMORY ? CSTONE_E_HIP : t == LOCAL_STEP ? CSTONE_E_INTERNAL : CSTONE_E_ARG; }

    /*! The agreement: every rank scans the same gathered rows (stride words each, the status at word `status`) and the first
     *  rank in trouble decides, so all ranks return from here or none does -- that rank with its own text and code, the
     *  others with "reported a failure".  MISMATCH is nobody's own: the caller derives it from the rows, it is the same
     *  refusal on every rank and names the first rank that differs. */
    int agree(const char* call, const std::vector<uint64_t>& rows, size_t stride, size_t status, const char* const* why)
    {
        for (int p = 0; p < P_; ++p)
        {
            const uint64_t st = rows[stride * p + status];
            if (st == FINE) continue;
            if (st == MISMATCH) return fail(ctx_, troubleCode(st), "%s: %s (rank %d; refused on every rank)", call, why[st], p);
            if (p != rank_) return fail(ctx_, CSTONE_E_INTERNAL, "%s: rank %d reported a failure (refused on every rank)", call, p);
            return fail(ctx_, troubleCode(st), "%s: %s (refused on every rank)", call, why[st]);
        }
        return CSTONE_OK;
    }

    //! The row gather, first half: my row of `words` 64-bit words to gatherRow() (one rank: it is all of rows already)
    int stageRow(const uint64_t* row, size_t words, std::vector<uint64_t>& rows)
    {
        rows.assign(row, row + words);
        rows.resize(words * P_);
        return P_ > 1 ? cstone_hip_upload(ctx_, gatherRow(), row, words * 8) : CSTONE_OK;
    }

    //! ... second half: what is staged at gatherRow() on every rank (a kernel may have added to it) to rows, on the host
    int gatherRows(size_t words, const char* what, std::vector<uint64_t>& rows)
    {
        if (P_ == 1) return CSTONE_OK;
        CS_TRY(callComm(comm_.all_gather(comm_.user, gatherRow(), gatherRecv(), words * 8), what));
        return copyToHost(ctx_, rows.data(), gatherRecv(), rows.size() * 8);
    }

    //! recvCounts[p] = what rank p has for me: column rank_ of the gathered count rows (stride words each); their sum
    uint64_t recvColumn(const std::vector<uint64_t>& rows, size_t stride, std::vector<uint64_t>& recvCounts) const
    {
        uint64_t numRecv = 0;
        recvCounts.assign(P_, 0);
        for (int p = 0; p < P_; ++p)
            numRecv += recvCounts[p] = rows[stride * p + rank_];
        return numRecv;
    }

    //! sendCounts[p] = how many of the n ascending labels owner p holds, whose ids start at offset[p]: the lower bounds of
    //! the owners' first ids.  firstIds (P words) and boundsDev (P + 1 u32) are the caller's device scratch
    int countsPerOwner(const uint64_t* labels, uint32_t n, const std::vector<uint64_t>& offset, uint64_t* firstIds,
                       uint32_t* boundsDev, std::vector<uint64_t>& sendCounts)
    {
        sendCounts.assign(P_, 0);
        sendCounts[0] = n;
        if (P_ == 1) return CSTONE_OK;
        std::vector<uint32_t> bounds(size_t(P_) + 1, n);
        CS_TRY(cstone_hip_upload(ctx_, firstIds, offset.data(), size_t(P_) * 8));
        CS_TRY(cstone_hip_lower_bound_u32(ctx_, 64, labels, n, firstIds, P_, boundsDev));
        CS_TRY(copyToHost(ctx_, bounds.data(), boundsDev, size_t(P_) * 4));
        for (int p = 0; p < P_; ++p)
            sendCounts[p] = bounds[p + 1] - bounds[p];
        return CSTONE_OK;
    }

    //! the slices of a work buffer, one behind the other on 256-byte boundaries; at: the bytes handed out so far
    struct Slicer
    {
        size_t at = 0;
        size_t take(size_t bytes) { return std::exchange(at, at + alignUp(bytes)); }
    };
    template<class V>
    static V* sliceOf(const DevBuf& buf, size_t byte) { return reinterpret_cast<V*>(buf.as<char>() + byte); }

    //! what an all_to_all_v does, also on one rank (where the one segment is copied)
    int fofAllToAll(const void* send, const std::vector<uint64_t>& sendCounts, void* recv, const std::vector<uint64_t>& recvCounts,
                    size_t elem, const char* what)
    {
        if (P_ == 1)
        {
            if (sendCounts[0])
                CS_HIP(ctx_, hipMemcpyAsync(recv, send, sendCounts[0] * elem, hipMemcpyDeviceToDevice, ctx_->stream));
            return CSTONE_OK;
        }
        std::vector<size_t> sb(P_), rbv(P_);
        for (int p = 0; p < P_; ++p)
            sb[p] = sendCounts[p] * elem, rbv[p] = recvCounts[p] * elem;
        return callComm(comm_.all_to_all_v(comm_.user, send, sb.data(), recv, rbv.data()), what);
    }

    // ---- friendsOfFriends(), stage by stage

    //! What the stages of one friendsOfFriends() share: the caller's arguments and what the stages before have decided
    struct FofState
    {
        const void *x, *y, *z;
        double b;
        uint32_t maxRounds;
        uint64_t *labels, *groupSizes, *numGroups;
        uint32_t* rounds;
        uint32_t si = 0, ei = 0, nh = 0, na = 0; // the view's: assigned [si, ei) of nh present, na = ei - si
        uint64_t trouble = FINE;
        std::vector<uint64_t> offset; // P + 1 bounds of the ranks' id ranges: global ids are positions in the SFC order
        bool wantSizes = false;       // some rank asked for the sizes
        uint32_t made  = 0;           // rounds made
        double groups  = 0;           // groups over all ranks
    };

    //! what is the same on every rank: refused before any collective
    int fofRefuseEverywhere(FofState& s)
    {
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_fof: no sync yet");
        if (!(s.b > 0.0)) return fail(ctx_, CSTONE_E_ARG, "domain_mr_fof: linking length %g is not > 0", s.b); // (NaN too)
        for (int d = 0; d < 3; ++d)
        {
            const double len = view_.box.lim[2 * d + 1] - view_.box.lim[2 * d];
            if (view_.box.bc[d] == 1 && !(s.b < 0.5 * len))
                return fail(ctx_, CSTONE_E_ARG, "domain_mr_fof: linking length %g is not below half the periodic edge %g", s.b, len);
        }
        if (s.maxRounds == 0) s.maxRounds = CSTONE_FOF_MR_DEFAULT_ROUNDS;
        s.si = view_.start_index, s.ei = view_.end_index, s.nh = view_.num_particles_with_halos, s.na = s.ei - s.si;
        return CSTONE_OK;
    }

    //! rank-local trouble: collected, not returned.  The local components are made here, in front of the all-gather (they
    //! need nothing from the other ranks), so that their failure is part of the agreement too
    void fofLocalComponents(FofState& s)
    {
        const size_t nh1 = std::max<uint32_t>(s.nh, 1);
        if (s.nh && (!s.x || !s.y || !s.z || !s.labels)) s.trouble = NULL_ARRAY;
        else if (viewSync_ != syncs_) s.trouble = STALE_SYNC; // the last sync was abandoned: tree and radii are not the view's
        if (!s.trouble && (fofComp_.ensure(ctx_, nh1 * 4) || fofLabels_.ensure(ctx_, nh1 * 8) || fofScal_.ensure(ctx_, 4096) ||
                           (s.groupSizes && (fofSizes_.ensure(ctx_, nh1 * 8) || fofWork_.ensure(ctx_, fofSlices(s.nh, s.na).end)))))
            s.trouble = NO_MEMORY;
        if (s.trouble || !s.nh) return;
        cstone_hip_domain_mr_octree t;
        if (octree(&t) ||
            cstone_hip_friends_of_friends(ctx_, rb, s.x, s.y, s.z, 0, s.nh, &view_.box, t.child_offsets, t.internal_to_leaf, t.layout,
                                          t.centers, t.sizes, s.b, fofComp_.as<uint32_t>(), nullptr, nullptr))
            s.trouble = LOCAL_STEP;
    }

    //! ONE all-gather: assigned count, smallest halo radius of a non-empty assigned leaf, status, sizes wanted; behind the
    //! agreement the cover condition and the id ranges
    int fofAgree(FofState& s)
    {
        const uint64_t INF_BITS = 0x7f800000u;
        const uint64_t row[4]   = {s.na, INF_BITS, s.trouble, s.groupSizes ? 1u : 0u};
        std::vector<uint64_t> rows;
        CS_TRY(stageRow(row, 4, rows));
        if (P_ > 1 && !s.trouble) // (low word of the second entry: the radii are floats)
            fofMinRadius(ctx_, useLet_ ? let_->haloRadii() : radii_.as<float>(), view_.focus_leaf_counts, view_.start_cell,
                         view_.end_cell, reinterpret_cast<uint32_t*>(gatherRow() + 1));
        CS_TRY(gatherRows(4, "all_gather (fof)", rows));
        static const char* const why[NUM_TROUBLES] = {"", "null array", "the last sync was abandoned", "out of device memory", "",
                                                      "the local group finder failed"};
        CS_TRY(agree("domain_mr_fof", rows, 4, 2, why));
        s.offset.assign(size_t(P_) + 1, 0);
        for (int p = 0; p < P_; ++p)
        {
            // the cover condition, against the very f32 radii the halo discovery of the last sync used.  One rank: every
            // particle is on the rank, there is nothing to cover
            float radius;
            const uint32_t bits = uint32_t(rows[4 * size_t(p) + 1]);
            std::memcpy(&radius, &bits, sizeof radius);
            if (P_ > 1 && !(s.b <= double(radius)))
                return fail(ctx_, CSTONE_E_ARG,
                            "domain_mr_fof: linking length %g exceeds the halo radius %g of a leaf of rank %d: a friend may "
                            "be missing among the halos (refused on every rank)",
                            s.b, double(radius), p);
            s.offset[p + 1] = s.offset[p] + rows[4 * size_t(p)];
            s.wantSizes     = s.wantSizes || rows[4 * size_t(p) + 3] != 0;
        }
        return CSTONE_OK;
    }

    //! ids: the position in the global SFC order; halos carry their owner's
    int fofAssignIds(FofState& s)
    {
        CS_TRY(cstone_hip_sequence_u64(ctx_, fofLabels_.as<uint64_t>() + s.si, s.na, s.offset[rank_]));
        return exchangeHalos(fofLabels_.p, 8);
    }

    //! rounds of { lower the labels, exchange their halos, all-reduce "somebody changed" } up to the first quiet one
    int fofRounds(FofState& s)
    {
        uint64_t* lab        = fofLabels_.as<uint64_t>();
        uint32_t* changedDev = fofScal_.as<uint32_t>(); // [0]: changed, [1]: groups owned, byte 8: their sum over the ranks
        uint32_t any         = 1;
        while (any && s.made < s.maxRounds)
        {
            CS_HIP(ctx_, hipMemsetAsync(changedDev, 0, 8, ctx_->stream));
            CS_TRY(cstone_hip_fof_lower_labels(ctx_, fofComp_.as<uint32_t>(), s.nh, s.si, s.ei, lab, changedDev));
            ++s.made;
            CS_TRY(exchangeHalos(lab, 8));
            if (P_ > 1)
            {
                fofClampFlag(ctx_, changedDev); // (the sum of the counts themselves could wrap to 0)
                CS_TRY(callComm(comm_.all_reduce(comm_.user, changedDev, 1, 1, 0), "all_reduce (fof round)"));
            }
            CS_TRY(copyToHost(ctx_, &any, changedDev, 4));
        }
        if (any)
            return fail(ctx_, CSTONE_E_INTERNAL, "domain_mr_fof: labels still changing after %u rounds (max_rounds)", s.made);
        return CSTONE_OK;
    }

    //! number of groups: every group is counted by the owner of its lowest member.  Exact: an f64 sum below 2^53
    int fofCountGroups(FofState& s)
    {
        uint32_t* ownDev = fofScal_.as<uint32_t>() + 1;
        fofCountOwn(ctx_, fofLabels_.as<uint64_t>() + s.si, s.na, s.offset[rank_], ownDev);
        uint32_t own = 0;
        CS_TRY(copyToHost(ctx_, &own, ownDev, 4));
        s.groups = double(own);
        if (P_ > 1)
        {
            double* sum = sliceOf<double>(fofScal_, 8);
            CS_TRY(cstone_hip_upload(ctx_, sum, &s.groups, 8));
            CS_TRY(callComm(comm_.all_reduce(comm_.user, sum, 1, 0, 0), "all_reduce (fof groups)"));
            CS_TRY(copyToHost(ctx_, &s.groups, sum, 8));
        }
        return CSTONE_OK;
    }

    //! the domain's buffers to the caller's arrays, at the very end: a refused call has written nothing
    int fofHandOut(FofState& s)
    {
        CS_TRY(cstone_hip_ctx_sync(ctx_)); // the sticky device-side error word
        if (s.nh) CS_HIP(ctx_, hipMemcpyAsync(s.labels, fofLabels_.p, size_t(s.nh) * 8, hipMemcpyDeviceToDevice, ctx_->stream));
        if (s.nh && s.groupSizes)
            CS_HIP(ctx_, hipMemcpyAsync(s.groupSizes, fofSizes_.p, size_t(s.nh) * 8, hipMemcpyDeviceToDevice, ctx_->stream));
        if (s.numGroups) *s.numGroups = uint64_t(s.groups);
        if (s.rounds) *s.rounds = s.made;
        fofOffset_     = s.offset; // the id ranges these labels were made with (fofCatalog)
        fofOffsetSync_ = syncs_;
        return CSTONE_OK;
    }

    //! the slices of fofWork_ (fofGroupSizes) for nh particles of which na are assigned
    struct FofSlices { size_t count, keys, keysAlt, values, valuesAlt, temp, tempBytes, pairs, answers, componentTotals, totals, end; };
    static FofSlices fofSlices(uint32_t nh, uint32_t na)
    {
        const size_t n = std::max<uint32_t>(nh, 1), tempBytes = cstone_hip_sort_pairs_temp_bytes(64, n);
        Slicer w; // (a braced list is evaluated from left to right)
        return {w.take(n * 4), w.take(n * 8), w.take(n * 8), w.take(n * 4), w.take(n * 4), w.take(tempBytes + 256), tempBytes,
                w.take(n * sizeof(FofPair)), w.take(n * 8), w.take(n * 8), w.take(size_t(std::max<uint32_t>(na, 1)) * 8), w.at};
    }

    /*! fofSizes_[k] = members of k's group over all ranks.  Every local component with an assigned member sends (label,
     *  assigned members) to the owner of the label -- sorted by label the pairs of one owner are contiguous, owners hold
     *  contiguous id ranges in rank order --, the owner adds them up per own particle and answers every pair with the
     *  total; the halo ranges are the owners' values, by the domain's halo exchange.  offset: P + 1 id range bounds. */
    int fofGroupSizes(const std::vector<uint64_t>& offset, const uint32_t* comp, const uint64_t* lab)
    {
        const uint32_t si = view_.start_index, ei = view_.end_index, nh = view_.num_particles_with_halos, na = ei - si;
        const FofSlices s = fofSlices(nh, na);
        CS_TRY(fofSizes_.ensure(ctx_, size_t(std::max<uint32_t>(nh, 1)) * 8));
        CS_TRY(fofWork_.ensure(ctx_, s.end));
        auto* count = sliceOf<uint32_t>(fofWork_, s.count);
        auto* keys = sliceOf<uint64_t>(fofWork_, s.keys);
        auto* values = sliceOf<uint32_t>(fofWork_, s.values);
        auto* pairs = sliceOf<FofPair>(fofWork_, s.pairs);
        auto* answers = sliceOf<uint64_t>(fofWork_, s.answers);

        uint32_t numPairs = 0;
        CS_TRY(fofComponentPairs(ctx_, comp, nh, si, ei, lab, count, keys, values, &numPairs));
        if (numPairs)
            CS_TRY(cstone_hip_sort_pairs(ctx_, 64, keys, values, numPairs, sliceOf<char>(fofWork_, s.keysAlt),
                                         sliceOf<uint32_t>(fofWork_, s.valuesAlt), sliceOf<char>(fofWork_, s.temp), s.tempBytes));
        fofPackPairs(ctx_, keys, values, count, numPairs, pairs);

        // pairs per owner, the counts travel first
        std::vector<uint64_t> sendCounts, recvCounts, matrix;
        CS_TRY(countsPerOwner(keys, numPairs, offset, sliceOf<uint64_t>(fofScal_, 256), sliceOf<uint32_t>(fofScal_, 2048), sendCounts));
        CS_TRY(countMatrix(sendCounts, matrix));
        const uint64_t numRecv = recvColumn(matrix, P_, recvCounts);
        if (numRecv >= (uint64_t(1) << 32)) return fail(ctx_, CSTONE_E_CAPACITY, "domain_mr_fof: %llu pairs for one owner", (unsigned long long)numRecv);
        const size_t pairBytes = alignUp(std::max<uint64_t>(numRecv, 1) * sizeof(FofPair));
        CS_TRY(fofRecv_.ensure(ctx_, pairBytes + std::max<uint64_t>(numRecv, 1) * 8));
        auto* pairsRecv  = fofRecv_.as<FofPair>();
        auto* answersOut = sliceOf<uint64_t>(fofRecv_, pairBytes);
        CS_TRY(fofAllToAll(pairs, sendCounts, pairsRecv, recvCounts, sizeof(FofPair), "all_to_all_v (fof pairs)"));
        CS_TRY(fofOwnerTotals(ctx_, pairsRecv, uint32_t(numRecv), offset[rank_], na, sliceOf<uint64_t>(fofWork_, s.totals), answersOut));
        CS_TRY(fofAllToAll(answersOut, recvCounts, answers, sendCounts, 8, "all_to_all_v (fof totals)"));
        fofSizesFromAnswers(ctx_, values, answers, numPairs, comp, si, ei, sliceOf<uint64_t>(fofWork_, s.componentTotals),
                            fofSizes_.as<uint64_t>());
        CS_HIP(ctx_, hipGetLastError());
        return exchangeHalos(fofSizes_.p, 8);
    }

    // ---- fofCatalog(), stage by stage

    //! the slices of catWork_ for the sender's n labels, and those of catRecv_ for the owner's n records
    struct CatSendSlices { size_t keys, keysAlt, values, valuesAlt, temp, tempBytes, work, runStart, runLabels, end; };
    static CatSendSlices catSendSlices(size_t n)
    {
        const size_t tempBytes = cstone_hip_sort_pairs_temp_bytes(64, n);
        Slicer w;
        return {w.take(n * 8), w.take(n * 8), w.take(n * 4), w.take(n * 4), w.take(tempBytes + 256), tempBytes,
                w.take((2 * n + 64) * 4), w.take((n + 1) * 4), w.take(n * 8), w.at};
    }
    struct CatOwnerSlices
    {
        size_t records, keys, keysAlt, order, orderAlt, temp, tempBytes, work, runStart, combined, keep, pos, total, end;
    };
    static CatOwnerSlices catOwnerSlices(size_t n)
    {
        const size_t tempBytes = cstone_hip_sort_pairs_temp_bytes(64, n);
        Slicer w;
        return {w.take(n * sizeof(FofPartial)), w.take(n * 8), w.take(n * 8), w.take(n * 4), w.take(n * 4), w.take(tempBytes + 256),
                tempBytes, w.take((2 * n + 64) * 4), w.take((n + 1) * 4), w.take(n * sizeof(FofPartial)), w.take(n * 4),
                w.take(n * 4), w.take(256), w.at};
    }
    //! catScal_: the owners' first ids at byte 256, behind them the bounds of their records -- sized by the number of ranks
    size_t catBoundsAt() const { return 256 + alignUp(size_t(P_) * 8); }

    //! What the stages of one fofCatalog() share: the caller's arguments and what the stages before have decided
    struct CatalogState
    {
        const void *x, *y, *z, *m;
        int massBits;
        const void *vx, *vy, *vz;
        const uint64_t* labels;
        uint64_t minMembers;
        size_t capacity;
        uint64_t *groupLabels, *groupSizes;
        void *mass, *center, *velocity, *radius;
        uint32_t *flags, *numGroupsHost;
        int nv = 0;                    // velocity components given: 0 or 3
        uint32_t si = 0, ei = 0, na = 0;
        uint64_t trouble = FINE;
        CatSendSlices snd{};
        uint32_t runs[2] = {0, 0};     // distinct labels here, labels outside [0, total)
        std::vector<uint64_t> sendCounts, recvCounts; // records per owner, records per source rank
        uint64_t numRecv = 0;
        CatOwnerSlices own{};
        uint32_t ownRuns = 0;          // distinct labels among the records: groups before the filter
    };

    //! what is the same on every rank: refused before any collective
    int catalogRefuseEverywhere(CatalogState& s)
    {
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_fof_catalog: no sync yet");
        if (fofOffsetSync_ != syncs_ || fofOffset_.size() != size_t(P_) + 1)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_fof_catalog: no domain_mr_fof since the last sync");
        s.nv = (s.vx ? 1 : 0) + (s.vy ? 1 : 0) + (s.vz ? 1 : 0);
        if ((s.massBits != 32 && s.massBits != 64) || (s.nv != 0 && s.nv != 3) || !s.numGroupsHost)
            return fail(ctx_, CSTONE_E_ARG, "domain_mr_fof_catalog: bad argument");
        if (s.minMembers == 0) s.minMembers = 1;
        s.si = view_.start_index, s.ei = view_.end_index, s.na = s.ei - s.si;
        return CSTONE_OK;
    }

    //! rank-local trouble: collected, not returned
    void catalogLocalTrouble(CatalogState& s)
    {
        if (s.na && (!s.x || !s.y || !s.z || !s.m || !s.labels || !s.groupLabels || !s.groupSizes || !s.mass || !s.center ||
                     (s.nv == 3 && !s.velocity)))
            s.trouble = NULL_ARRAY;
        else if (s.na >= (1u << 30)) s.trouble = LOCAL_STEP;
        s.snd = catSendSlices(std::max<uint32_t>(s.na, 1));
        if (!s.trouble && (catWork_.ensure(ctx_, s.snd.end) || catPart_.ensure(ctx_, sizeof(FofPartial)) ||
                           catScal_.ensure(ctx_, catBoundsAt() + alignUp((size_t(P_) + 1) * 4))))
            s.trouble = NO_MEMORY;
        s.sendCounts.assign(P_, 0);
    }

    //! the local steps: their failure is trouble too, and a rank in trouble sends nothing
    void catalogLocalSteps(CatalogState& s)
    {
        if (s.trouble || !s.na) return;
        const int rc = catalogPartials(s);
        if (rc != CSTONE_OK) s.trouble = rc == CSTONE_E_HIP ? NO_MEMORY : LOCAL_STEP;
        else if (s.runs[1]) s.trouble = BAD_LABEL;
        if (s.trouble) std::fill(s.sendCounts.begin(), s.sendCounts.end(), uint64_t(0));
    }

    //! ... one partial per distinct label of the assigned range, in label order, and how many of them each owner gets
    int catalogPartials(CatalogState& s)
    {
        auto* keys = sliceOf<uint64_t>(catWork_, s.snd.keys);
        auto* values = sliceOf<uint32_t>(catWork_, s.snd.values);
        auto* runStart = sliceOf<uint32_t>(catWork_, s.snd.runStart);
        auto* runLabels = sliceOf<uint64_t>(catWork_, s.snd.runLabels);
        CS_HIP(ctx_, hipMemcpyAsync(keys, s.labels + s.si, size_t(s.na) * 8, hipMemcpyDeviceToDevice, ctx_->stream));
        CS_TRY(cstone_hip_sequence_u32(ctx_, values, s.na, s.si));
        // stable: the members of a label stay in ascending order, its first member is its lowest index
        CS_TRY(cstone_hip_sort_pairs(ctx_, 64, keys, values, s.na, sliceOf<char>(catWork_, s.snd.keysAlt),
                                     sliceOf<uint32_t>(catWork_, s.snd.valuesAlt), sliceOf<char>(catWork_, s.snd.temp), s.snd.tempBytes));
        CS_TRY(fofRunsU64(ctx_, keys, s.na, fofOffset_[P_], sliceOf<uint32_t>(catWork_, s.snd.work), runStart, runLabels, s.runs));
        if (s.runs[1]) return CSTONE_OK; // (reported as BAD_LABEL)
        if (catPart_.ensure(ctx_, size_t(s.runs[0]) * sizeof(FofPartial))) return CSTONE_E_HIP;
        CS_TRY(fofPropsReduce(ctx_, rb, s.massBits, s.x, s.y, s.z, s.m, s.vx, s.vy, s.vz, view_.box, runStart, values, s.runs[0],
                              FofGroupOut{}, catPart_.as<FofPartial>(), keys));
        return countsPerOwner(runLabels, s.runs[0], fofOffset_, sliceOf<uint64_t>(catScal_, 256),
                              sliceOf<uint32_t>(catScal_, catBoundsAt()), s.sendCounts);
    }

    //! collective 1: the counts per owner and the status; behind the agreement what arrives here
    int catalogAgree(CatalogState& s)
    {
        std::vector<uint64_t> rows, row(s.sendCounts);
        row.push_back(s.trouble);
        CS_TRY(stageRow(row.data(), row.size(), rows));
        CS_TRY(gatherRows(row.size(), "all_gather (fof catalogue)", rows));
        static const char* const why[NUM_TROUBLES] = {"", "null array", "", "out of device memory", "a label outside [0, total)",
                                                      "a local step failed"};
        CS_TRY(agree("domain_mr_fof_catalog", rows, row.size(), P_, why));
        s.numRecv = recvColumn(rows, row.size(), s.recvCounts);
        if (s.numRecv >= (uint64_t(1) << 30))
            return fail(ctx_, CSTONE_E_CAPACITY, "domain_mr_fof_catalog: %llu records for one owner", (unsigned long long)s.numRecv);
        return CSTONE_OK;
    }

    //! collective 2: the records to the owners.  How much arrives is known only now, behind the one agreement: a rank whose
    //! receive buffer cannot be had (or whose share exceeds 2^30 records) returns ALONE, and the others then wait in the
    //! all_to_all_v -- as in the size protocol of friendsOfFriends
    int catalogExchange(CatalogState& s)
    {
        s.own = catOwnerSlices(std::max<uint64_t>(s.numRecv, 1));
        CS_TRY(catRecv_.ensure(ctx_, s.own.end));
        CS_TRY(fofAllToAll(catPart_.p, s.sendCounts, sliceOf<FofPartial>(catRecv_, s.own.records), s.recvCounts, sizeof(FofPartial),
                           "all_to_all_v (fof catalogue)"));
        *s.numGroupsHost = 0;
        return CSTONE_OK;
    }

    //! the owner: stable sort by label (the records arrive by source rank), combine, filter
    int catalogCombine(CatalogState& s)
    {
        auto* records = sliceOf<FofPartial>(catRecv_, s.own.records);
        auto* keys = sliceOf<uint64_t>(catRecv_, s.own.keys);
        auto* order = sliceOf<uint32_t>(catRecv_, s.own.order);
        auto* runStart = sliceOf<uint32_t>(catRecv_, s.own.runStart);
        auto* keep = sliceOf<uint32_t>(catRecv_, s.own.keep);
        fofPartialLabels(ctx_, records, uint32_t(s.numRecv), keys);
        CS_TRY(cstone_hip_sequence_u32(ctx_, order, s.numRecv, 0));
        CS_TRY(cstone_hip_sort_pairs(ctx_, 64, keys, order, s.numRecv, sliceOf<char>(catRecv_, s.own.keysAlt),
                                     sliceOf<uint32_t>(catRecv_, s.own.orderAlt), sliceOf<char>(catRecv_, s.own.temp), s.own.tempBytes));
        uint32_t ownRuns[2] = {0, 0};
        CS_TRY(fofRunsU64(ctx_, keys, uint32_t(s.numRecv), ~uint64_t(0), sliceOf<uint32_t>(catRecv_, s.own.work), runStart, nullptr,
                          ownRuns));
        s.ownRuns = ownRuns[0];
        CS_TRY(fofCombinePartials(ctx_, rb, s.x, s.y, s.z, view_.box, records, order, runStart, s.ownRuns, fofOffset_[rank_], s.si,
                                  s.na, s.minMembers, sliceOf<FofPartial>(catRecv_, s.own.combined), keep));
        CS_TRY(arenaReserve(ctx_, scanArenaBytes(s.ownRuns) + 1024));
        const int scanned = scanU32(ctx_, keep, sliceOf<uint32_t>(catRecv_, s.own.pos), s.ownRuns, 0u, false,
                                    sliceOf<uint32_t>(catRecv_, s.own.total));
        arenaReset(ctx_);
        return scanned;
    }

    //! finish: how many groups are kept, the capacity judged behind both collectives, the kept groups to the caller's arrays
    int catalogFinish(CatalogState& s)
    {
        uint32_t kept = 0;
        CS_TRY(copyToHost(ctx_, &kept, sliceOf<uint32_t>(catRecv_, s.own.total), 4));
        CS_TRY(cstone_hip_ctx_sync(ctx_)); // the sticky device-side error word (a record whose label is not mine)
        *s.numGroupsHost = kept;
        if (kept > s.capacity)
            return fail(ctx_, CSTONE_E_CAPACITY, "domain_mr_fof_catalog: %u groups, capacity %zu", kept, s.capacity);
        return fofFinishCombined(ctx_, rb, s.nv == 3, view_.box, sliceOf<FofPartial>(catRecv_, s.own.combined),
                                 sliceOf<uint32_t>(catRecv_, s.own.keep), sliceOf<uint32_t>(catRecv_, s.own.pos), s.ownRuns,
                                 FofGroupOut{s.mass, s.center, s.velocity, s.radius, s.flags, s.groupLabels, s.groupSizes});
    }

    // ---- sphereProfiles(), stage by stage

    //! What the stages of one sphereProfiles() share: the caller's arguments and what the stages before have decided
    struct ProfilesState
    {
        const void *x, *y, *z, *w;
        int massBits;
        const void *queryCenters, *queryScale;
        uint32_t numQueries;
        const double* edgesHost;
        int numBins;
        uint64_t* counts;
        double* sums;
        uint32_t* flags;
        uint32_t si = 0, ei = 0, na = 0;
        size_t cells     = 0; // numQueries x numBins
        uint64_t trouble = FINE;
        cstone_hip_domain_mr_octree t{}; // my octree; all null on a rank without particles
        bool globalW = false;            // some rank with particles has a w: the sums take part in the all-reduce
    };

    //! what is the same on every rank: refused before any collective
    int profilesRefuseEverywhere(ProfilesState& s)
    {
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_sphere_profiles: no sync yet");
        if (!sphereEdgesOk(s.edgesHost, s.numBins)) return fail(ctx_, CSTONE_E_ARG, "domain_mr_sphere_profiles: bad edges");
        if (s.w && s.massBits != 32 && s.massBits != 64) return fail(ctx_, CSTONE_E_ARG, "domain_mr_sphere_profiles: bad mass_bits");
        s.si = view_.start_index, s.ei = view_.end_index, s.na = s.ei - s.si;
        s.cells = size_t(s.numQueries) * size_t(s.numBins);
        return CSTONE_OK;
    }

    //! one rank: the single-rank call on my octree, no agreement and no operand
    int profilesOnOneRank(ProfilesState& s)
    {
        if (s.numQueries == 0) return CSTONE_OK;
        CS_TRY(octree(&s.t));
        return cstone_hip_sphere_profiles(ctx_, rb, s.massBits, s.x, s.y, s.z, s.w, s.si, s.ei, &view_.box, s.t.child_offsets,
                                          s.t.internal_to_leaf, s.t.layout, s.t.centers, s.t.sizes, s.queryCenters, s.queryScale,
                                          s.numQueries, s.edgesHost, s.numBins, s.counts, s.sums, s.flags);
    }

    //! rank-local trouble: collected, not returned
    void profilesLocalTrouble(ProfilesState& s)
    {
        if (s.numQueries && (!s.queryCenters || !s.counts || (s.w && !s.sums) || (s.na && (!s.x || !s.y || !s.z))))
            s.trouble = NULL_ARRAY;
        else if (sphereBuf_.ensure(ctx_, std::max<size_t>(2 * s.cells * sizeof(double), 256))) s.trouble = NO_MEMORY;
        else if (s.na && octree(&s.t)) s.trouble = LOCAL_STEP;
    }

    //! one all-gather of {status, Q, NB, w given}: every rank fails together, also where the ranks disagree on the last three
    int profilesAgree(ProfilesState& s)
    {
        enum : uint64_t { W_NONE = 0, W_GIVEN = 1, W_ANY = 2 }; // a rank without particles goes with the others
        const uint64_t row[4] = {s.trouble, s.numQueries, uint64_t(s.numBins), s.w ? W_GIVEN : s.na ? W_NONE : W_ANY};
        std::vector<uint64_t> rows;
        CS_TRY(stageRow(row, 4, rows));
        CS_TRY(gatherRows(4, "all_gather (sphere profiles)", rows));
        uint64_t wMode = W_ANY;
        for (int p = 0; p < P_; ++p)
        {
            uint64_t* r = rows.data() + 4 * size_t(p);
            if (r[0] == FINE && (r[1] != rows[1] || r[2] != rows[2])) r[0] = MISMATCH;
            if (r[0] != FINE || r[3] == W_ANY) continue;
            if (wMode == W_ANY) wMode = r[3];
            else if (wMode != r[3]) r[0] = MISMATCH;
        }
        static const char* const why[NUM_TROUBLES] = {"", "null array", "", "out of device memory", "", "no octree",
                                                      "the ranks disagree on num_queries, num_bins or whether there is a w"};
        s.globalW = wMode == W_GIVEN;
        return agree("domain_mr_sphere_profiles", rows, 4, 0, why);
    }

    //! the local profiles, into the caller's arrays.  A rank without particles has nothing to read: its empty range zeroes
    //! the rows and sets the flags, and the operand itself stands in for the arrays it may not have
    int profilesLocal(ProfilesState& s)
    {
        const void* dummy = sphereBuf_.p;
        auto nz           = [&](const void* ptr) { return ptr ? ptr : dummy; };
        return cstone_hip_sphere_profiles(ctx_, rb, s.massBits, nz(s.x), nz(s.y), nz(s.z), s.w, s.si, s.ei, &view_.box,
                                          static_cast<const int32_t*>(nz(s.t.child_offsets)),
                                          static_cast<const int32_t*>(nz(s.t.internal_to_leaf)),
                                          static_cast<const uint32_t*>(nz(s.t.layout)), nz(s.t.centers), nz(s.t.sizes),
                                          s.queryCenters, s.queryScale, s.numQueries, s.edgesHost, s.numBins, s.counts, s.sums,
                                          s.flags);
    }

    //! one all-reduce: {counts as doubles, sums}
    int profilesReduce(ProfilesState& s)
    {
        double* buf = sphereBuf_.as<double>();
        if (s.globalW && !s.w) CS_HIP(ctx_, hipMemsetAsync(buf + s.cells, 0, s.cells * sizeof(double), ctx_->stream));
        spherePackRows(ctx_, s.counts, s.w ? s.sums : nullptr, s.cells, buf);
        CS_TRY(callComm(comm_.all_reduce(comm_.user, buf, (s.globalW ? 2 : 1) * s.cells, 0, 0), "all_reduce (sphere profiles)"));
        sphereUnpackRows(ctx_, buf, s.cells, s.counts, s.globalW ? s.sums : nullptr);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return fail(ctx_, CSTONE_E_HIP, "domain_mr_sphere_profiles: %s", hipGetErrorString(e));
        return CSTONE_OK;
    }

    // ---- pairCounts(), stage by stage

    //! What the stages of one pairCounts() share: the caller's arguments and what the stages before have decided
    struct PairState
    {
        bool cross;
        const void *x, *y, *z, *w;
        int wBits;
        const void *queryCenters, *queryW;
        uint32_t numQueries;
        const double* edgesHost;
        int numBins;
        uint64_t* counts;
        double* sums;
        uint64_t* statsHost;
        uint32_t si = 0, ei = 0, na = 0, nh = 0;
        uint64_t trouble = FINE;
        cstone_hip_domain_mr_octree t{}; // my octree; all null on a rank without particles
        bool globalW = false;            // some rank with particles has a w: the sums take part in the all-reduce
        const char* name() const { return cross ? "domain_mr_pair_counts_cross" : "domain_mr_pair_counts"; }
    };

    //! what is the same on every rank: refused before any collective
    int pairRefuseEverywhere(PairState& s)
    {
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "%s: no sync yet", s.name());
        if (const char* why = pairCountsRefusal(rb, s.wBits, s.w != nullptr, &view_.box, s.edgesHost, s.numBins))
            return fail(ctx_, CSTONE_E_ARG, "%s: %s", s.name(), why);
        s.si = view_.start_index, s.ei = view_.end_index, s.nh = view_.num_particles_with_halos, s.na = s.ei - s.si;
        return CSTONE_OK;
    }

    //! the single-rank call on my octree, into the caller's arrays.  A rank without assigned particles has nothing to read:
    //! its empty range zeroes the outputs
    int pairLocal(PairState& s)
    {
        if (s.cross)
            return cstone_hip_pair_counts_cross(ctx_, rb, s.wBits, s.x, s.y, s.z, s.w, s.si, s.ei, &view_.box, s.t.child_offsets,
                                                s.t.internal_to_leaf, s.t.layout, s.t.centers, s.t.sizes, s.queryCenters,
                                                s.w ? s.queryW : nullptr, s.numQueries, s.edgesHost, s.numBins, s.counts, s.sums,
                                                s.statsHost);
        return cstone_hip_pair_counts(ctx_, rb, s.wBits, s.x, s.y, s.z, s.w, 0, s.nh, s.si, s.ei, &view_.box, s.t.child_offsets,
                                      s.t.internal_to_leaf, s.t.layout, s.t.centers, s.t.sizes, s.edgesHost, s.numBins, s.counts,
                                      s.sums, s.statsHost);
    }

    //! one rank: no agreement, no cover rule (every particle is on the rank) and no operand
    int pairOnOneRank(PairState& s)
    {
        if (s.na) CS_TRY(octree(&s.t));
        return pairLocal(s);
    }

    //! rank-local trouble: collected, not returned
    void pairLocalTrouble(PairState& s)
    {
        const bool queries = s.cross && s.numQueries;
        if (!s.counts || (s.w && !s.sums) || (queries && !s.queryCenters) || (s.na && (!s.x || !s.y || !s.z)) ||
            (s.na && s.queryW && !s.w))
            s.trouble = NULL_ARRAY;
        else if (!s.cross && viewSync_ != syncs_) s.trouble = STALE_SYNC; // the radii of the cover rule are not the view's
        else if (sphereBuf_.ensure(ctx_, std::max<size_t>(2 * size_t(s.numBins) * sizeof(double), 256))) s.trouble = NO_MEMORY;
        else if (s.na && octree(&s.t)) s.trouble = LOCAL_STEP;
    }

    //! one all-gather of {status, NB, w given, smallest halo radius of a non-empty assigned leaf (auto) or Q (cross)}: every
    //! rank fails together, also where the ranks disagree or the cover rule fails on any of them
    int pairAgree(PairState& s)
    {
        enum : uint64_t { W_NONE = 0, W_GIVEN = 1, W_ANY = 2 }; // a rank without particles goes with the others
        const uint64_t INF_BITS = 0x7f800000u;
        const uint64_t row[4]   = {s.trouble, uint64_t(s.numBins), s.w ? W_GIVEN : s.na ? W_NONE : W_ANY,
                                   s.cross ? uint64_t(s.numQueries) : INF_BITS};
        std::vector<uint64_t> rows;
        CS_TRY(stageRow(row, 4, rows));
        if (!s.cross && !s.trouble) // (low word of the last entry: the radii are floats)
            fofMinRadius(ctx_, useLet_ ? let_->haloRadii() : radii_.as<float>(), view_.focus_leaf_counts, view_.start_cell,
                         view_.end_cell, reinterpret_cast<uint32_t*>(gatherRow() + 3));
        CS_TRY(gatherRows(4, "all_gather (pair counts)", rows));
        uint64_t wMode = W_ANY;
        for (int p = 0; p < P_; ++p)
        {
            uint64_t* r = rows.data() + 4 * size_t(p);
            if (r[0] == FINE && (r[1] != rows[1] || (s.cross && r[3] != rows[3]))) r[0] = MISMATCH;
            if (r[0] != FINE || r[2] == W_ANY) continue;
            if (wMode == W_ANY) wMode = r[2];
            else if (wMode != r[2]) r[0] = MISMATCH;
        }
        static const char* const why[NUM_TROUBLES] = {"", "null array", "the last sync was abandoned", "out of device memory", "",
                                                      "no octree",
                                                      "the ranks disagree on num_bins, num_queries or whether there is a w"};
        s.globalW = wMode == W_GIVEN;
        CS_TRY(agree(s.name(), rows, 4, 0, why));
        for (int p = 0; p < P_ && !s.cross; ++p)
        {
            // the cover rule of friendsOfFriends, against the very f32 radii the halo discovery of the last sync used
            float radius;
            const uint32_t bits = uint32_t(rows[4 * size_t(p) + 3]);
            std::memcpy(&radius, &bits, sizeof radius);
            if (!(s.edgesHost[s.numBins] <= double(radius)))
                return fail(ctx_, CSTONE_E_ARG,
                            "%s: the outer edge %g exceeds the halo radius %g of a leaf of rank %d: a partner may be missing "
                            "among the halos (refused on every rank)",
                            s.name(), s.edgesHost[s.numBins], double(radius), p);
        }
        return CSTONE_OK;
    }

    //! one all-reduce: {counts as doubles, sums}
    int pairReduce(PairState& s)
    {
        double* buf    = sphereBuf_.as<double>();
        const size_t n = size_t(s.numBins);
        if (s.globalW && !s.w) CS_HIP(ctx_, hipMemsetAsync(buf + n, 0, n * sizeof(double), ctx_->stream));
        spherePackRows(ctx_, s.counts, s.w ? s.sums : nullptr, n, buf);
        CS_TRY(callComm(comm_.all_reduce(comm_.user, buf, (s.globalW ? 2 : 1) * n, 0, 0), "all_reduce (pair counts)"));
        sphereUnpackRows(ctx_, buf, n, s.counts, s.globalW ? s.sums : nullptr);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(ctx_, CSTONE_E_HIP, "%s: %s", s.name(), hipGetErrorString(e));
        return CSTONE_OK;
    }

    // ---- knn(), stage by stage

    //! What the stages of one knn() share: the caller's arguments and what the stages before have decided
    struct KnnState
    {
        const void *x, *y, *z, *queryCenters, *queryRmax;
        uint32_t numQueries, k;
        uint64_t* ids;
        void* dist2;
        uint32_t* counts;
        uint32_t si = 0, ei = 0, na = 0;
        uint32_t chunk   = 0; // queries per all_gather
        uint64_t trouble = FINE;
        uint64_t idBase  = 0;            // the global id of my first assigned particle
        cstone_hip_domain_mr_octree t{}; // my octree; all null on a rank without particles
        KnnRecord *send = nullptr, *recv = nullptr;
    };

    //! the cap on the receive buffer of one all_gather: CSTONE_KNN_MR_GATHER_BYTES, or what the environment variable of
    //! that name says (a positive number of bytes; for tests of the chunking)
    static uint64_t knnGatherCap()
    {
        if (const char* e = std::getenv("CSTONE_KNN_MR_GATHER_BYTES"))
        {
            char* end                  = nullptr;
            const unsigned long long v = std::strtoull(e, &end, 10);
            if (end != e && *end == 0 && v > 0) return v;
        }
        return CSTONE_KNN_MR_GATHER_BYTES;
    }

    //! what is the same on every rank: refused before any collective
    int knnRefuseEverywhere(KnnState& s)
    {
        knnChunks_ = 0, knnGatherBytes_ = 0;
        if (firstCall_) return fail(ctx_, CSTONE_E_ARG, "domain_mr_knn: no sync yet");
        if (s.k < 1 || s.k > CSTONE_KNN_MAX_K) return fail(ctx_, CSTONE_E_ARG, "domain_mr_knn: k outside 1 .. %d", CSTONE_KNN_MAX_K);
        s.si = view_.start_index, s.ei = view_.end_index, s.na = s.ei - s.si;
        s.chunk = knnChunkQueries(s.numQueries, s.k, P_, knnGatherCap());
        return CSTONE_OK;
    }

    //! rank-local trouble: collected, not returned.  The buffer: my rows of a chunk, then everybody's (one rank: mine are all)
    void knnLocalTrouble(KnnState& s)
    {
        const size_t rowBytes = alignUp(size_t(s.chunk) * s.k * sizeof(KnnRecord));
        if (s.numQueries && (!s.queryCenters || !s.ids || (s.na && (!s.x || !s.y || !s.z)))) s.trouble = NULL_ARRAY;
        else if (knnBuf_.ensure(ctx_, std::max<size_t>(rowBytes * (P_ > 1 ? size_t(P_) + 1 : 1), 256))) s.trouble = NO_MEMORY;
        else if (s.na && octree(&s.t)) s.trouble = LOCAL_STEP;
        s.send = knnBuf_.as<KnnRecord>();
        s.recv = P_ > 1 ? sliceOf<KnnRecord>(knnBuf_, rowBytes) : s.send;
        knnGatherBytes_ = P_ > 1 ? uint64_t(P_) * s.chunk * s.k * sizeof(KnnRecord) : 0;
    }

    //! one all-gather of {status, Q, k, rmax given, assigned count}: every rank fails together, also where the ranks
    //! disagree on the middle three; the counts give the id ranges, those of friendsOfFriends()
    int knnAgree(KnnState& s)
    {
        const uint64_t row[5] = {s.trouble, s.numQueries, s.k, s.queryRmax ? 1u : 0u, s.na};
        std::vector<uint64_t> rows;
        CS_TRY(stageRow(row, 5, rows));
        CS_TRY(gatherRows(5, "all_gather (knn)", rows));
        for (int p = 0; p < P_; ++p)
        {
            uint64_t* r = rows.data() + 5 * size_t(p);
            if (r[0] == FINE && (r[1] != rows[1] || r[2] != rows[2] || r[3] != rows[3])) r[0] = MISMATCH;
            if (p < rank_) s.idBase += r[4];
        }
        static const char* const why[NUM_TROUBLES] = {"", "null array", "", "out of device memory", "", "no octree",
                                                      "the ranks disagree on num_queries, k or whether there is a query_rmax"};
        return agree("domain_mr_knn", rows, 5, 0, why);
    }

    //! byte offset of query q0 in an array of `per` values of the coordinate type per query
    const void* knnAt(const void* base, uint32_t q0, size_t per) const
    {
        return base ? static_cast<const char*>(base) + size_t(q0) * per * (rb / 8) : nullptr;
    }

    //! my answer for the queries [q0, q0 + nq) as records.  A rank without particles has nothing to read: its empty range
    //! leaves every row unfilled without touching the arrays or the tree
    int knnLocal(KnnState& s, uint32_t q0, uint32_t nq)
    {
        return knnLocalRecords(ctx_, rb, s.x, s.y, s.z, s.si, s.ei, view_.box, s.t.child_offsets, s.t.internal_to_leaf,
                               s.t.layout, s.t.centers, s.t.sizes, knnAt(s.queryCenters, q0, 3), knnAt(s.queryRmax, q0, 1), nq,
                               s.k, s.idBase, s.send);
    }

    //! everybody's rows of the chunk: recv[p][q][0 .. k)
    int knnGather(KnnState& s, uint32_t nq)
    {
        if (P_ == 1) return CSTONE_OK;
        return callComm(comm_.all_gather(comm_.user, s.send, s.recv, size_t(nq) * s.k * sizeof(KnnRecord)), "all_gather (knn rows)");
    }

    //! the k best of the P rows of every query of the chunk, into the caller's arrays
    int knnMerge(KnnState& s, uint32_t q0, uint32_t nq)
    {
        void* d2 = s.dist2 ? static_cast<char*>(s.dist2) + size_t(q0) * s.k * (rb / 8) : nullptr;
        return knnMergeRecords(ctx_, rb, s.recv, P_, knnAt(s.queryRmax, q0, 1), nq, s.k, s.ids + size_t(q0) * s.k, d2,
                               s.counts ? s.counts + q0 : nullptr);
    }

    cstone_hip_ctx* ctx_;
    int curve_, rank_, P_;
    uint32_t bucket_, bucketFocus_;
    cstone_box box_;
    cstone_hip_comm_ops comm_;
    float haloExt_  = 1.0f;
    float theta_    = 0.5f;
    int sortMode_   = CSTONE_SORT_INCREMENTAL;
    bool speculativeBox_ = std::getenv("CSTONE_NO_SPECULATIVE_BOX") == nullptr;
    bool measureFirst_   = false; // the last box was not the one before it: measure the extents before encoding
    int boxRedos_        = 0;     // syncs whose speculative keys were thrown away because the box had changed
    bool useLet_    = std::getenv("CSTONE_MR_OWNER_SIDE") == nullptr; // halos through the locally essential tree (default)
    std::unique_ptr<FocusLet<K, T>> let_;
    const K* resortTree_ = nullptr; // the leaves of my own key range (and their number) the next sync's re-sort starts from
    int resortLeaves_    = 0;
    bool firstCall_ = true;
    bool ctxGone_   = false; // the destructor runs behind the context's destruction (cstone_hip_domain_mr_destroy)
    bool toggled_   = false; // this sync has switched to the other output buffer set already
    int pending_    = 0; // status of this rank inside sync(): 0, or the error code the peers have to learn about
    uint32_t statusW32_ = 0; // staging of the status word that rides on the box counts (an asynchronous copy reads it)
    std::string pendingMsg_;
    bool timing_    = std::getenv("CSTONE_MR_TIMING") != nullptr;
    bool noMargin_  = std::getenv("CSTONE_MR_NO_MARGIN") != nullptr; // tests: no room left for halos, the block is moved
    bool peerLoop_  = std::getenv("CSTONE_MR_PEER_LOOP") != nullptr; // tests: take the > 32 ranks path (one traversal per peer)
    int syncs_      = 0;
    bool adapted_   = false; // adaptH ran since the last sync (one call per sync; every sync clears it)
    int viewSync_   = -1;    // the sync view_ was made by; differs from syncs_ after an abandoned sync (friendsOfFriends)
    std::map<std::string, double> phase_;
    std::chrono::steady_clock::time_point t0_;
    std::vector<K> assignment_;
    cstone_hip_domain_mr_view view_{};

    DevBuf scal_;
    DevBuf keys_, order_, keysAlt_, orderAlt_, sortTmp_;
    DevBuf gTree_, gCounts_, gLocalCounts_;
    int gCap_ = 0, gLeaves_ = 0;
    bool gTreeSame_ = false; // the global leaf array is that of the previous sync
    GlobalTreeHost<K> gHost_;           // host copies of the global tree and its all-reduced counts (assign()), and the
                                        // pinned block where the read-backs of a sync arrive
    bool gLeavesOnHost_  = false;       // gHost_.leaves is what gTree_ holds (the host made this sync's update step)
    bool hostGlobalStep_ = std::getenv("CSTONE_MR_DEVICE_GLOBAL_STEP") == nullptr; // (tests: the device-side step)
    bool speculateCuts_  = std::getenv("CSTONE_MR_NO_SPECULATIVE_CUTS") == nullptr;  // (tests: always ask after assign())
    int cutRedos_        = 0; // syncs whose assignment changed: cut points asked for twice
    float centerDriftTol_      = 1.05f; // Domain::centerDriftTol_ (R/domain/domain.hpp:665)
    bool haveExpansionCenters_ = false; // the last sync was a syncGrav (or updateExpansionCenters followed it)
    DevBuf gravGroups_;                 // u32[gravNumGroups_ + 1]: target groups of computeGravity over the assigned range
    uint32_t gravNumGroups_ = 0;
    int gravGroupsSync_     = -1;       // ... computed for this sync
    bool overlapPlace_   = std::getenv("CSTONE_MR_NO_PLACE_OVERLAP") == nullptr; // x, y, z placed on the second stream
    bool placeForked_    = false; // ... and not joined yet
    DevBuf fTree_, fCounts_, fTmp_;
    int fCap_ = 0, fLeaves_ = 0;
    DevBuf fPrefixes_, fChild_, fParents_, fLevelRange_, fItl_, fLti_;
    DevBuf leaving_, sendRows_, recvRows_, rcol_[4], rcolS_[4], rk_, ro_, posA_, posB_, moveTmp_;
    DevBuf propRecv_[MAX_PROPS], propRecvS_[MAX_PROPS];
    uint64_t prevLo_ = 0, prevHi_ = 0;
    LeafResort<K> resort_;
    int resortBackoff_ = 0, resorts_ = 0;
    uint32_t lastMovers_ = 0;
    uint64_t layoutParticles_ = 0; // particles and box layout_ was made for
    cstone_box layoutBox_{};
    std::vector<K> coverHost_; // leaf keys inserted at the range boundaries, staged for the copy to the device
    int coverDeepest_ = 0;     // level of the deepest of them
    int treeSteps_    = 0;     // single update steps of the focus tree so far (0: the tree was just built from scratch)
    // tree over all local particles incl. halos (octree()), built on request
    DevBuf nsTree_, nsCounts_, nsLayout_, nsPrefixes_, nsChild_, nsParents_, nsLevelRange_, nsItl_, nsLti_, nsCenters_,
        nsSizes_;
    int nsCap_ = 0, nsLeaves_ = 0, nsSync_ = -1;
    // particle routes of the last sync (reapplySync): input size, kept / received / sent counts, start of the kept range
    uint64_t rsN_ = 0, rsNa_ = 0, rsNb_ = 0, rsSend_ = 0, rsMoved_ = 0, rsKeptOffset_ = 0;
    std::vector<uint64_t> rsSendCounts_, rsRecvCounts_;
    int prevMaxLeafLevel_ = -1; // deepest level of this rank's tree at the previous sync
    NodeIdx* hostLevelRange_ = nullptr; // pinned: the level ranges of the last tree, read at the start of the next sync
    bool levelRangePending_  = false;
    // halo exchange pattern of the last sync (exchangeHalos)
    std::vector<uint64_t> haloSend_, haloRecv_;
    uint64_t haloRecvLo_ = 0, haloRecvHi_ = 0, haloAssigned_ = 0, haloSel_ = 0, haloAnyLast_ = 0;
    DevBuf layout_, radii_, boxes_, boxFlags_, myBoxes_, allBoxes_, oflags_, cnt_, sel_;
    // friendsOfFriends(): component ids, labels and sizes before they are handed out, scalars, the size protocol's slices
    DevBuf fofComp_, fofLabels_, fofSizes_, fofScal_, fofWork_, fofRecv_;
    // fofCatalog(): the id ranges of the last friendsOfFriends() and the sync they belong to; the sender's slices, its
    // partials, the owner's slices
    std::vector<uint64_t> fofOffset_;
    int fofOffsetSync_ = -1;
    DevBuf catWork_, catPart_, catRecv_, catScal_;
    DevBuf sphereBuf_; // the operand of the all-reduce of sphereProfiles: {counts as doubles, sums}
    DevBuf knnBuf_;    // knn(): my rows of a chunk of queries, then the rows of every rank
    uint32_t knnChunks_      = 0; // of the last knn(): all_gather rounds made, bytes its receive buffer took
    uint64_t knnGatherBytes_ = 0;
    Out out_[2];
    int cur_ = 0;
};

} // namespace

} // namespace cship

using namespace cship;

struct cstone_hip_domain_mr
{
    cstone_hip_ctx* ctx;
    std::unique_ptr<MrBase> impl;
};

extern "C"
{

int cstone_hip_domain_mr_create(cstone_hip_ctx* ctx, cstone_hip_domain_mr** out, int curve, int key_bits, int real_bits,
                                int rank, int num_ranks, uint32_t bucket_size, uint32_t bucket_size_focus,
                                const cstone_box* box_host, const cstone_hip_comm_ops* comm)
{
    if (!ctx || !out || !box_host || !comm) return fail(ctx, CSTONE_E_ARG, "domain_mr_create: null argument");
    if (num_ranks < 1 || rank < 0 || rank >= num_ranks) return fail(ctx, CSTONE_E_ARG, "domain_mr_create: bad rank");
    // the small per-rank tables of a sync (cut points, send counts) live in fixed slots of one scalar block
    if (num_ranks > 96) return fail(ctx, CSTONE_E_ARG, "domain_mr_create: at most 96 ranks in this version");
    if (num_ranks > 1 && (!comm->all_reduce || !comm->all_gather || !comm->all_to_all_v))
        return fail(ctx, CSTONE_E_ARG, "domain_mr_create: missing collective");
    if (curve != CSTONE_MORTON && curve != CSTONE_HILBERT) return fail(ctx, CSTONE_E_ARG, "domain_mr_create: bad curve");
    // Domain ctor (R/domain/domain.hpp:95-113)
    if (bucket_size < bucket_size_focus)
        return fail(ctx, CSTONE_E_ARG, "The bucket size of the global tree must not be smaller than the bucket size of "
                                       "the focused tree");
    auto* d = new cstone_hip_domain_mr{ctx, nullptr};
    if (key_bits == 64 && real_bits == 64)
        d->impl = std::make_unique<MultiRankDomain<uint64_t, double>>(ctx, curve, rank, num_ranks, bucket_size,
                                                                      bucket_size_focus, *box_host, *comm);
    else if (key_bits == 64 && real_bits == 32)
        d->impl = std::make_unique<MultiRankDomain<uint64_t, float>>(ctx, curve, rank, num_ranks, bucket_size,
                                                                     bucket_size_focus, *box_host, *comm);
    else if (key_bits == 32 && real_bits == 64)
        d->impl = std::make_unique<MultiRankDomain<uint32_t, double>>(ctx, curve, rank, num_ranks, bucket_size,
                                                                      bucket_size_focus, *box_host, *comm);
    else if (key_bits == 32 && real_bits == 32)
        d->impl = std::make_unique<MultiRankDomain<uint32_t, float>>(ctx, curve, rank, num_ranks, bucket_size,
                                                                     bucket_size_focus, *box_host, *comm);
    else
    {
        delete d;
        return fail(ctx, CSTONE_E_ARG, "domain_mr_create: unsupported type combination");
    }
    *out = d;
    return CSTONE_OK;
}

int cstone_hip_domain_mr_destroy(cstone_hip_domain_mr* dom)
{
    if (!dom) return CSTONE_E_ARG;
    const bool alive = ctxAlive(dom->ctx); // (see cstone_hip_domain_destroy)
    if (alive) (void)hipStreamSynchronize(dom->ctx->stream);
    else (void)hipDeviceSynchronize();
    dom->impl->contextGone(!alive);
    delete dom;
    return alive ? CSTONE_OK : CSTONE_E_ARG;
}

int cstone_hip_domain_mr_sync_props(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z,
                                    const void* h, size_t n, const void* const* props, const int* prop_bytes,
                                    int num_props)
{
    if (!dom) return CSTONE_E_ARG;
    if (n && (!x || !y || !z || !h)) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync: null array");
    if (num_props && (!props || !prop_bytes)) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync: null property list");
    return dom->impl->sync(x, y, z, h, n, props, prop_bytes, num_props, nullptr);
}

int cstone_hip_domain_mr_sync_keys(cstone_hip_domain_mr* dom, const void* keys, const void* x, const void* y,
                                   const void* z, const void* h, size_t n, const void* const* props,
                                   const int* prop_bytes, int num_props)
{
    if (!dom) return CSTONE_E_ARG;
    if (n && (!x || !y || !z || !h)) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync: null array");
    if (num_props && (!props || !prop_bytes)) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync: null property list");
    return dom->impl->sync(x, y, z, h, n, props, prop_bytes, num_props, keys);
}

int cstone_hip_domain_mr_sync_grav(cstone_hip_domain_mr* dom, const void* keys, const void* x, const void* y,
                                   const void* z, const void* h, const void* m, int mass_bits, size_t n,
                                   const void* const* props, const int* prop_bytes, int num_props)
{
    if (!dom) return CSTONE_E_ARG;
    if (n && (!x || !y || !z || !h || !m)) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync_grav: null array");
    if (num_props && (!props || !prop_bytes)) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync_grav: null property list");
    if (mass_bits != 32 && mass_bits != 64) return fail(dom->ctx, CSTONE_E_ARG, "domain_mr_sync_grav: mass_bits %d", mass_bits);
    return dom->impl->sync(x, y, z, h, n, props, prop_bytes, num_props, keys, m, mass_bits);
}

int cstone_hip_domain_mr_update_expansion_centers(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z,
                                                  const void* m, int mass_bits)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->updateExpansionCenters(x, y, z, m, mass_bits);
}

int cstone_hip_domain_mr_compute_gravity(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z,
                                         const void* m, int mass_bits, int order, double G, double eps2, void* ax,
                                         void* ay, void* az, void* phi)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->computeGravity(x, y, z, m, nullptr, mass_bits, order, G, eps2, ax, ay, az, phi);
}

int cstone_hip_domain_mr_compute_gravity_h(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z,
                                           const void* m, const void* h, int mass_bits, int order, double G,
                                           double eps2, void* ax, void* ay, void* az, void* phi)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->computeGravity(x, y, z, m, h, mass_bits, order, G, eps2, ax, ay, az, phi);
}

int cstone_hip_domain_mr_adapt_h(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z, void* h,
                                 uint32_t ng0, uint32_t tol, uint32_t max_iter, float grow_limit, uint32_t* counts,
                                 uint32_t* status)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->adaptH(x, y, z, h, ng0, tol, max_iter, grow_limit, counts, status);
}

int cstone_hip_domain_mr_fof(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z, double linking_length,
                             uint32_t max_rounds, uint64_t* labels, uint64_t* group_sizes, uint64_t* num_groups,
                             uint32_t* rounds)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->friendsOfFriends(x, y, z, linking_length, max_rounds, labels, group_sizes, num_groups, rounds);
}

int cstone_hip_domain_mr_fof_catalog(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z, const void* m,
                                     int mass_bits, const void* vx, const void* vy, const void* vz, const uint64_t* labels,
                                     uint64_t min_members, size_t capacity, uint64_t* group_labels, uint64_t* group_sizes,
                                     void* mass, void* center, void* velocity, void* radius, uint32_t* flags,
                                     uint32_t* num_groups_host)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->fofCatalog(x, y, z, m, mass_bits, vx, vy, vz, labels, min_members, capacity, group_labels, group_sizes,
                                 mass, center, velocity, radius, flags, num_groups_host);
}

int cstone_hip_domain_mr_sphere_profiles(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z,
                                         const void* w, int mass_bits, const void* query_centers, const void* query_scale,
                                         uint32_t num_queries, const double* edges_host, int num_bins, uint64_t* counts,
                                         double* sums, uint32_t* flags)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->sphereProfiles(x, y, z, w, mass_bits, query_centers, query_scale, num_queries, edges_host, num_bins,
                                     counts, sums, flags);
}

int cstone_hip_domain_mr_pair_counts(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z, const void* w,
                                     int w_bits, const double* edges_host, int num_bins, uint64_t* counts, double* sums,
                                     uint64_t* stats_host)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->pairCounts(false, x, y, z, w, w_bits, nullptr, nullptr, 0, edges_host, num_bins, counts, sums, stats_host);
}

int cstone_hip_domain_mr_pair_counts_cross(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z,
                                           const void* w, int w_bits, const void* query_centers, const void* query_w,
                                           uint32_t num_queries, const double* edges_host, int num_bins, uint64_t* counts,
                                           double* sums, uint64_t* stats_host)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->pairCounts(true, x, y, z, w, w_bits, query_centers, query_w, num_queries, edges_host, num_bins, counts,
                                 sums, stats_host);
}

int cstone_hip_domain_mr_knn(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z, const void* query_centers,
                             const void* query_rmax, uint32_t num_queries, uint32_t k, uint64_t* ids, void* dist2,
                             uint32_t* counts)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->knn(x, y, z, query_centers, query_rmax, num_queries, k, ids, dist2, counts);
}

int cstone_hip_domain_mr_knn_last(cstone_hip_domain_mr* dom, uint32_t* num_chunks, uint64_t* gather_bytes)
{
    if (!dom) return CSTONE_E_ARG;
    dom->impl->knnLast(num_chunks, gather_bytes);
    return CSTONE_OK;
}

int cstone_hip_domain_mr_multipoles_get(cstone_hip_domain_mr* dom, const void** multipoles, int32_t* num_nodes)
{
    if (!dom || !multipoles || !num_nodes) return CSTONE_E_ARG;
    return dom->impl->multipoles(multipoles, num_nodes);
}

int cstone_hip_domain_mr_octupoles_get(cstone_hip_domain_mr* dom, const void** octupoles, int32_t* num_nodes)
{
    if (!dom || !octupoles || !num_nodes) return CSTONE_E_ARG;
    return dom->impl->octupoles(octupoles, num_nodes);
}

int cstone_hip_domain_mr_sync(cstone_hip_domain_mr* dom, const void* x, const void* y, const void* z, const void* h,
                              size_t n)
{
    return cstone_hip_domain_mr_sync_props(dom, x, y, z, h, n, nullptr, nullptr, 0);
}

int cstone_hip_domain_mr_view_get(cstone_hip_domain_mr* dom, cstone_hip_domain_mr_view* out)
{
    if (!dom || !out) return CSTONE_E_ARG;
    return dom->impl->view(out);
}

int cstone_hip_domain_mr_exchange_halos(cstone_hip_domain_mr* dom, void* array, int elem_bytes)
{
    if (!dom || !array) return CSTONE_E_ARG;
    return dom->impl->exchangeHalos(array, elem_bytes);
}

int cstone_hip_domain_mr_octree_get(cstone_hip_domain_mr* dom, cstone_hip_domain_mr_octree* out)
{
    if (!dom || !out) return CSTONE_E_ARG;
    return dom->impl->octree(out);
}

int cstone_hip_domain_mr_reapply_sync(cstone_hip_domain_mr* dom, const void* in, size_t n, int elem_bytes, void* out)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->reapplySync(in, n, elem_bytes, out);
}

int cstone_hip_domain_mr_set_halo_mode(cstone_hip_domain_mr* dom, int mode)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->setHaloMode(mode);
}

int cstone_hip_domain_mr_set_theta(cstone_hip_domain_mr* dom, float theta)
{
    if (!dom) return CSTONE_E_ARG;
    return dom->impl->setTheta(theta);
}

int cstone_hip_domain_mr_set_sort_mode(cstone_hip_domain_mr* dom, int mode)
{
    if (!dom || mode < CSTONE_SORT_INCREMENTAL || mode > CSTONE_SORT_ALL_DIGITS) return CSTONE_E_ARG;
    dom->impl->setSortMode(mode);
    return CSTONE_OK;
}

int cstone_hip_domain_mr_set_halo_factor(cstone_hip_domain_mr* dom, float factor)
{
    if (!dom || !(factor > 0.0f)) return CSTONE_E_ARG;
    dom->impl->setHaloFactor(factor);
    return CSTONE_OK;
}

} // extern "C"
