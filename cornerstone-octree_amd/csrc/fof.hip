// Friends-of-friends groups on gfx950: particles closer than a linking length b are friends, groups are the connected
// components of that relation.  The rule is stated in include/cstone_hip.h, cstone_hip_friends_of_friends: i and j of the
// target range are linked iff cstone_hip_find_neighbors at ext = 1 reports j for i OR i for j when h = T(0.5) * T(b) -- the
// same walk (cstone_hip::traverseNeighborsH), the same d^2, the same strict <, compiled with -ffp-contract=off like
// neighbors.hip.  The pair test is symmetric (b below half of every periodic edge is enforced), the walk is not quite: a
// pair within rounding of b across a cell face can be pruned by the node test from one side and reported from the other
// (tests/test_face_pairs.py).  So every lane unites its target with EVERY reported j of the range, not only with the
// smaller ones: the relation is the symmetric closure of the walk's and does not depend on how the particles are numbered.
// Wherever no such pair is pruned from both sides this is the brute force over all pairs in the coordinate type, and any
// union-find reproduces the labels with ==.
//
// The forest is the label array itself (union_find.hpp: parent[v] <= v, parent[v] in v's component).  Four passes:
//   init     labels[k] = first + k
//   link     the layout of findNeighborsKernel -- one wave per 64 consecutive targets, four waves per block, the LDS stack
//            of cstone_hip_device.hpp -- with a functor that unites i and j instead of storing j.  Lock-free: one
//            compare-and-swap per union hooks the larger root under the smaller.  Reads of parent are relaxed agent-scope
//            atomic loads (they bypass the CU's L1, and the compiler cannot keep them in a register); what they return may
//            still be STALE, which is harmless: any value parent[v] ever held is a smaller vertex of v's component, so the
//            chain still descends, and a root that is none any more makes the compare-and-swap (done at the memory side,
//            on the true value) fail and return the true parent, from which the search goes on.  A lane keeps the root of
//            i in a register between neighbours and shortens i's chain to it once, after its walk.  No lane waits for
//            another lane: every loop ends by itself (strictly decreasing chains, a retry cap on top).
//   flatten  behind the link kernel's end: labels[k] = root(k), the minimum of k's component; counts the roots.
//   sizes    integer atomicAdd at the roots, one per run of equal labels in a wave, then sizes[k] = count[labels[k]].
// All atomics are on integers and every result is a function of the components alone: the same input gives the same bits
// in every run.  The catalogue (cstone_hip_fof_catalog) is a stable radix sort of (label, index), head flags, two scans
// and a compaction.
//
// Groups across ranks (cstone_hip_domain_mr_fof, domain_mr.hip) take these labels as the components
// of everything present on a rank and lower 64-bit global labels to the minimum of each component, round after round:
// cstone_hip_fof_lower_labels below -- all ones, one 64-bit atomic minimum per run of equal components of a wave, a
// broadcast pass that counts what dropped.  The device steps of the group sizes across ranks (fof_mr.hpp) are here too.
#include <algorithm>

#include "cstone_hip_device.hpp"
#include "ctx.hpp"
#include "fof_mr.hpp"
#include "scan.hpp"
#include "union_find.hpp"

namespace cship
{

namespace
{

constexpr int FOF_BLOCK = 256;
constexpr int FOF_WAVES = FOF_BLOCK / 64;
constexpr int FOF_ERR_RETRY_CAP = 16; // bit of the sticky error word: a union gave up at ufRetryCap

//! the operations of union_find.hpp on the label array of the range [first, first + n): vertex v lives at p[v - first]
struct DeviceParents
{
    uint32_t* p;
    uint32_t first;
    __device__ uint32_t load(uint32_t v) const
    {
        return __hip_atomic_load(p + (v - first), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ uint32_t cas(uint32_t v, uint32_t expect, uint32_t set) const { return atomicCAS(p + (v - first), expect, set); }
};

__global__ __launch_bounds__(256) void fofInitKernel(uint32_t* __restrict__ labels, uint32_t first, uint32_t n)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) labels[k] = first + k;
}

template<class T>
__global__ __launch_bounds__(FOF_BLOCK) void fofLinkKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                           const T* __restrict__ z, uint32_t first, uint32_t last, T hi,
                                                           cstone_hip::DeviceBox<T> box, cstone_hip::OctreeNsView<T> tree,
                                                           uint32_t* parent, int* __restrict__ errors)
{
    __shared__ cstone_hip::TraversalStack stacks[FOF_WAVES];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    const uint32_t chunk = first + (blockIdx.x * FOF_WAVES + wave) * 64u;
    if (chunk >= last) return;
    const bool valid = chunk + lane < last;
    const uint32_t i = valid ? chunk + lane : last - 1;

    const DeviceParents ops{parent, first};
    uint32_t root = i; // the root of i's tree as last seen: every find of this lane starts there, not at i
    bool gaveUp   = false;
    // every reported j of the range, whichever of i and j is larger: the walk of j may have pruned i's leaf by a rounding
    // of its node test (above), and ufUnite hooks the larger root under the smaller whatever the order.  A pair that both
    // walks report is united twice; the second union finds equal roots and writes nothing.  j outside [first, last) is
    // not a target: it links nothing and has no entry in parent.
    auto link = [&](uint32_t j, T, T, T, T)
    {
        if (j >= first && j < last) root = ufUnite(ops, root, j, ufRetryCap, &gaveUp);
    };
    (void)cstone_hip::traverseNeighborsH(valid, i, x, y, z, hi, tree, box, 1.0f, stacks[wave], errors, link);
    if (valid) ufCompress(ops, i, root);
    if (gaveUp) atomicOr(errors, FOF_ERR_RETRY_CAP);
}

/*! labels[k] = root(k).  Runs behind the end of the link kernel: no root changes any more.  A thread may read parent[k]
 *  while k's own thread replaces it by root(k); both values lie on k's chain to the same root. */
__global__ __launch_bounds__(256) void fofFlattenKernel(uint32_t* labels, uint32_t first, uint32_t n,
                                                        uint32_t* __restrict__ numRoots)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const DeviceParents ops{labels, first};
    uint32_t r = 0;
    if (k < n)
    {
        r = ufFind(ops, first + k);
        __hip_atomic_store(labels + k, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (numRoots)
    {
        const uint64_t roots = __ballot(k < n && r == first + k);
        if ((threadIdx.x & 63u) == 0 && roots) atomicAdd(numRoots, uint32_t(__popcll(roots)));
    }
}

/*! count[label - first] += members.  Particles of a group are mostly consecutive (SFC order), so a wave holds few distinct
 *  labels: one atomicAdd per distinct label of the wave, with the number of lanes that carry it (at most 64 rounds) */
__global__ __launch_bounds__(256) void fofCountKernel(const uint32_t* __restrict__ labels, uint32_t first, uint32_t n,
                                                      uint32_t* __restrict__ count)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t lab  = k < n ? labels[k] : 0u;
    uint64_t todo       = __ballot(k < n);
    while (todo)
    {
        const int leader    = __ffsll((long long)todo) - 1;
        const uint32_t head = uint32_t(__shfl(int(lab), leader));
        const uint64_t same = __ballot(k < n && lab == head) & todo;
        if (int(lane) == leader) atomicAdd(count + (head - first), uint32_t(__popcll(same)));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void fofBroadcastKernel(const uint32_t* __restrict__ labels, uint32_t first, uint32_t n,
                                                          const uint32_t* __restrict__ count, uint32_t* __restrict__ sizes)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) sizes[k] = count[labels[k] - first];
}

// ---- the catalogue: (label, index) sorted by label; runs of equal labels are the groups ------------------------------

__global__ __launch_bounds__(256) void fofHeadsKernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ heads)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) heads[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1u : 0u;
}

//! runStart[r] = position of the head of run r (runId: inclusive scan of the head flags), runStart[numRuns] = n
__global__ __launch_bounds__(256) void fofRunStartsKernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ runId,
                                                          uint32_t n, uint32_t* __restrict__ runStart)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    if (k == 0 || keys[k] != keys[k - 1]) runStart[runId[k] - 1] = k;
    if (k == n - 1) runStart[runId[k]] = n;
}

//! keep[r] = run r has at least minMembers members; kept[r] = its length if so, else 0.  r < numRuns = runId[n - 1]
__global__ __launch_bounds__(256) void fofKeepKernel(const uint32_t* __restrict__ runStart, const uint32_t* __restrict__ runId,
                                                     uint32_t n, uint32_t minMembers, uint32_t* __restrict__ keep,
                                                     uint32_t* __restrict__ kept)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t len = r < runId[n - 1] ? runStart[r + 1] - runStart[r] : 0u;
    keep[r]            = len >= minMembers ? 1u : 0u; // (minMembers >= 1: an empty slot is never kept)
    kept[r]            = len >= minMembers ? len : 0u;
}

/*! one thread per sorted pair k of run r = runId[k] - 1: if the run is kept, its member goes to members[offset of the run
 *  + position in the run]; the head of the run writes the group's offset, the last pair the closing offset.  outIdx,
 *  outOff: exclusive scans of keep and kept; totals: {number of groups, number of members listed}.  Nothing is written
 *  when the offsets do not fit (the host reports it). */
__global__ __launch_bounds__(256) void fofFillKernel(const uint32_t* __restrict__ values, const uint32_t* __restrict__ runId,
                                                     const uint32_t* __restrict__ runStart, const uint32_t* __restrict__ keep,
                                                     const uint32_t* __restrict__ outIdx, const uint32_t* __restrict__ outOff,
                                                     const uint32_t* __restrict__ totals, uint32_t n, uint32_t capacity,
                                                     uint32_t* __restrict__ groupOffsets, uint32_t* __restrict__ members)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint32_t numGroups = totals[0];
    if (numGroups >= capacity) return; // numGroups + 1 entries are needed
    if (k == n - 1) groupOffsets[numGroups] = totals[1];
    const uint32_t r = runId[k] - 1;
    if (!keep[r]) return;
    const uint32_t pos = k - runStart[r];
    if (pos == 0) groupOffsets[outIdx[r]] = outOff[r];
    members[outOff[r] + pos] = values[k];
}

// ---- joining groups across ranks: the lowering step (cstone_hip_fof_lower_labels) and the group sizes (fof_mr.hpp) -----

constexpr int FOF_ERR_COMPONENT = 32; // bit of the sticky error word: a component id or a label outside its range

__global__ __launch_bounds__(256) void fofFillOnesKernel(uint64_t* __restrict__ words, uint32_t n)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) words[k] = ~uint64_t(0);
}

//! a 64-bit value from lane (own lane ^ mask): two 32-bit shuffles, both halves travel
__device__ inline uint64_t shflXor64(uint64_t v, int mask)
{
    const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(v)), mask));
    const uint32_t hi = uint32_t(__shfl_xor(int(uint32_t(v >> 32)), mask));
    return (uint64_t(hi) << 32) | lo;
}

/*! minOf[c] = min(minOf[c], labels[k]) over the k with component[k] == c.  The pattern of fofCountKernel: one 64-bit
 *  atomic minimum per distinct component of a wave, by the first lane that carries it, with the minimum over the lanes
 *  that share it (a butterfly in which the other lanes hold all ones; skipped for a component with one lane).  `same` is a
 *  ballot, so every branch on it is uniform over the wave. */
__global__ __launch_bounds__(256) void fofLowerMinKernel(const uint32_t* __restrict__ component, uint32_t n,
                                                         const uint64_t* __restrict__ labels, uint64_t* __restrict__ minOf,
                                                         int* __restrict__ errors)
{
    const uint32_t k    = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t comp = k < n ? component[k] : 0u;
    const bool ok       = k < n && comp < n; // (a component id beyond n has no word in minOf: reported, never written)
    if (k < n && !ok) atomicOr(errors, FOF_ERR_COMPONENT);
    const uint64_t lab = ok ? labels[k] : ~uint64_t(0);
    uint64_t todo      = __ballot(ok);
    while (todo)
    {
        const int leader    = __ffsll((long long)todo) - 1;
        const uint32_t head = uint32_t(__shfl(int(comp), leader));
        const uint64_t same = __ballot(ok && comp == head) & todo;
        uint64_t low        = lab;
        if (same & (same - 1)) // more than one lane
        {
            low = ((same >> lane) & 1u) ? lab : ~uint64_t(0);
            for (int offset = 32; offset; offset >>= 1)
            {
                const uint64_t other = shflXor64(low, offset);
                low                  = other < low ? other : low;
            }
        }
        if (int(lane) == leader) (void)__hip_atomic_fetch_min(minOf + head, low, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        todo &= ~same;
    }
}

//! labels[k] = minOf[component[k]]; *changed += the k of [first, last) whose label dropped (one atomicAdd per wave)
__global__ __launch_bounds__(256) void fofLowerBroadcastKernel(const uint32_t* __restrict__ component, uint32_t n,
                                                               uint32_t first, uint32_t last,
                                                               const uint64_t* __restrict__ minOf, uint64_t* __restrict__ labels,
                                                               uint32_t* __restrict__ changed)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool dropped     = false;
    if (k < n)
    {
        const uint32_t comp = component[k];
        if (comp < n)
        {
            const uint64_t low = minOf[comp];
            if (low < labels[k])
            {
                labels[k] = low;
                dropped   = true;
            }
        }
    }
    const uint64_t votes = __ballot(dropped && k >= first && k < last);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(changed, uint32_t(__popcll(votes)));
}

//! *numOwn += the k < n with labels[k] == firstId + k: the groups whose lowest member is one of these particles
__global__ __launch_bounds__(256) void fofCountOwnKernel(const uint64_t* __restrict__ labels, uint32_t n, uint64_t firstId,
                                                         uint32_t* __restrict__ numOwn)
{
    const uint32_t k     = blockIdx.x * 256u + threadIdx.x;
    const uint64_t votes = __ballot(k < n && labels[k] == firstId + k);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(numOwn, uint32_t(__popcll(votes)));
}

__global__ __launch_bounds__(256) void fofPairFlagsKernel(const uint32_t* __restrict__ count, uint32_t n,
                                                          uint32_t* __restrict__ flags)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < n) flags[c] = count[c] ? 1u : 0u;
}

//! one (label, component) pair per component with a counted member; pos: exclusive scan of the flags
__global__ __launch_bounds__(256) void fofEmitPairsKernel(const uint32_t* __restrict__ count, const uint32_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ labels, uint32_t n,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ values)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n || !count[c]) return;
    keys[pos[c]]   = labels[c]; // (a component id is the index of one of its members)
    values[pos[c]] = c;
}

__global__ __launch_bounds__(256) void fofPackPairsKernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ values,
                                                          const uint32_t* __restrict__ count, uint32_t numPairs,
                                                          FofPair* __restrict__ pairs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < numPairs) pairs[i] = FofPair{keys[i], uint64_t(count[values[i]])};
}

//! the owner's side: totals[label - firstId] += count for every received pair (a label that is not mine is reported)
__global__ __launch_bounds__(256) void fofAddTotalsKernel(const FofPair* __restrict__ pairs, uint32_t numPairs, uint64_t firstId,
                                                          uint32_t numOwn, unsigned long long* __restrict__ totals,
                                                          int* __restrict__ errors)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= numPairs) return;
    const uint64_t slot = pairs[i].label - firstId;
    if (slot < numOwn) atomicAdd(totals + slot, (unsigned long long)pairs[i].count);
    else atomicOr(errors, FOF_ERR_COMPONENT);
}

__global__ __launch_bounds__(256) void fofAnswerKernel(const FofPair* __restrict__ pairs, uint32_t numPairs, uint64_t firstId,
                                                       uint32_t numOwn, const unsigned long long* __restrict__ totals,
                                                       uint64_t* __restrict__ answers)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= numPairs) return;
    const uint64_t slot = pairs[i].label - firstId;
    answers[i]          = slot < numOwn ? uint64_t(totals[slot]) : 0u;
}

__global__ __launch_bounds__(256) void fofScatterTotalsKernel(const uint32_t* __restrict__ values,
                                                              const uint64_t* __restrict__ answers, uint32_t numPairs,
                                                              uint64_t* __restrict__ componentTotals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < numPairs) componentTotals[values[i]] = answers[i];
}

//! sizes[k] = componentTotals[component[k]] for k in [first, last)
__global__ __launch_bounds__(256) void fofSizesOfComponentsKernel(const uint32_t* __restrict__ component, uint32_t first,
                                                                  uint32_t last, const uint64_t* __restrict__ componentTotals,
                                                                  uint64_t* __restrict__ sizes)
{
    const uint32_t k = first + blockIdx.x * 256u + threadIdx.x;
    if (k < last) sizes[k] = componentTotals[component[k]];
}

//! *out = min(*out, bits of radii[leaf]) over the leaves of [first, last) that hold particles (radii are >= 0: the bit
//! patterns order like the values)
__global__ __launch_bounds__(256) void fofMinRadiusKernel(const float* __restrict__ radii, const uint32_t* __restrict__ counts,
                                                          int first, int last, uint32_t* __restrict__ out)
{
    const int leaf = first + int(blockIdx.x * 256u + threadIdx.x);
    uint32_t bits  = 0x7f800000u; // +inf
    if (leaf < last && counts[leaf]) bits = __float_as_uint(radii[leaf]);
    for (int offset = 32; offset; offset >>= 1)
        bits = min(bits, uint32_t(__shfl_xor(int(bits), offset)));
    if ((threadIdx.x & 63u) == 0 && bits != 0x7f800000u) atomicMin(out, bits);
}

__global__ void fofClampFlagKernel(uint32_t* word) { *word = *word ? 1u : 0u; }

template<class T>
void launchLink(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, uint32_t first, uint32_t last,
                const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf, const uint32_t* layout,
                const void* centers, const void* sizes, double linkingLength, uint32_t* labels)
{
    cstone_hip::OctreeNsView<T> tree{childOffsets, internalToLeaf, layout, (const T*)centers, (const T*)sizes};
    const T hi = T(0.5) * T(linkingLength);
    hipLaunchKernelGGL((fofLinkKernel<T>), gridFor(size_t(last - first), FOF_BLOCK), FOF_BLOCK, 0, ctx->stream, (const T*)x,
                       (const T*)y, (const T*)z, first, last, hi, cstone_hip::makeDeviceBox<T>(box), tree, labels,
                       ctx->devScalars + 63);
}

} // namespace

void fofMinRadius(cstone_hip_ctx* ctx, const float* radii, const uint32_t* counts, int first, int last, uint32_t* outBits)
{
    if (last > first)
        hipLaunchKernelGGL(fofMinRadiusKernel, gridFor(size_t(last - first), 256), 256, 0, ctx->stream, radii, counts, first,
                           last, outBits);
}

void fofClampFlag(cstone_hip_ctx* ctx, uint32_t* word) { hipLaunchKernelGGL(fofClampFlagKernel, 1, 1, 0, ctx->stream, word); }

void fofCountOwn(cstone_hip_ctx* ctx, const uint64_t* labels, uint32_t n, uint64_t firstId, uint32_t* numOwn)
{
    if (n) hipLaunchKernelGGL(fofCountOwnKernel, gridFor(n, 256), 256, 0, ctx->stream, labels, n, firstId, numOwn);
}

int fofComponentPairs(cstone_hip_ctx* ctx, const uint32_t* component, uint32_t n, uint32_t first, uint32_t last,
                      const uint64_t* labels, uint32_t* count, uint64_t* keys, uint32_t* values, uint32_t* numPairsHost)
{
    *numPairsHost = 0;
    if (n == 0 || last <= first) return CSTONE_OK;
    const size_t words = alignUp(size_t(n) * sizeof(uint32_t));
    CS_TRY(arenaReserve(ctx, 2 * words + scanArenaBytes(n) + 1024));
    uint32_t* flags = static_cast<uint32_t*>(arenaTake(ctx, words));
    uint32_t* pos   = static_cast<uint32_t*>(arenaTake(ctx, words));
    uint32_t* total = static_cast<uint32_t*>(arenaTake(ctx, 256));
    const unsigned grid = gridFor(n, 256);
    int rc              = CSTONE_OK;
    if (hipError_t e = hipMemsetAsync(count, 0, size_t(n) * sizeof(uint32_t), ctx->stream); e != hipSuccess)
        rc = fail(ctx, CSTONE_E_HIP, "fof group sizes: %s", hipGetErrorString(e));
    if (rc == CSTONE_OK)
    {
        // (the counting pass of the single-rank call, on the window: count[component[k]] for first <= k < last)
        hipLaunchKernelGGL(fofCountKernel, gridFor(last - first, 256), 256, 0, ctx->stream, component + first, 0u, last - first,
                           count);
        hipLaunchKernelGGL(fofPairFlagsKernel, grid, 256, 0, ctx->stream, count, n, flags);
        rc = scanU32(ctx, flags, pos, n, 0u, false, total);
    }
    if (rc == CSTONE_OK)
    {
        hipLaunchKernelGGL(fofEmitPairsKernel, grid, 256, 0, ctx->stream, count, pos, labels, n, keys, values);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            rc = fail(ctx, CSTONE_E_HIP, "fof group sizes: %s", hipGetErrorString(e));
    }
    if (rc == CSTONE_OK) rc = copyToHost(ctx, numPairsHost, total, sizeof(uint32_t));
    arenaReset(ctx);
    return rc;
}

void fofPackPairs(cstone_hip_ctx* ctx, const uint64_t* keys, const uint32_t* values, const uint32_t* count,
                  uint32_t numPairs, FofPair* pairs)
{
    if (numPairs)
        hipLaunchKernelGGL(fofPackPairsKernel, gridFor(numPairs, 256), 256, 0, ctx->stream, keys, values, count, numPairs, pairs);
}

int fofOwnerTotals(cstone_hip_ctx* ctx, const FofPair* pairs, uint32_t numPairs, uint64_t firstId, uint32_t numOwn,
                   uint64_t* totals, uint64_t* answers)
{
    if (numOwn) CS_HIP(ctx, hipMemsetAsync(totals, 0, size_t(numOwn) * sizeof(uint64_t), ctx->stream));
    if (!numPairs) return CSTONE_OK;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t));
    auto* t = reinterpret_cast<unsigned long long*>(totals);
    hipLaunchKernelGGL(fofAddTotalsKernel, gridFor(numPairs, 256), 256, 0, ctx->stream, pairs, numPairs, firstId, numOwn, t,
                       ctx->devScalars + 63);
    hipLaunchKernelGGL(fofAnswerKernel, gridFor(numPairs, 256), 256, 0, ctx->stream, pairs, numPairs, firstId, numOwn, t,
                       answers);
    return CSTONE_OK;
}

void fofSizesFromAnswers(cstone_hip_ctx* ctx, const uint32_t* values, const uint64_t* answers, uint32_t numPairs,
                         const uint32_t* component, uint32_t first, uint32_t last, uint64_t* componentTotals, uint64_t* sizes)
{
    if (numPairs)
        hipLaunchKernelGGL(fofScatterTotalsKernel, gridFor(numPairs, 256), 256, 0, ctx->stream, values, answers, numPairs,
                           componentTotals);
    if (last > first)
        hipLaunchKernelGGL(fofSizesOfComponentsKernel, gridFor(last - first, 256), 256, 0, ctx->stream, component, first, last,
                           componentTotals, sizes);
}

} // namespace cship

using namespace cship;

extern "C" int cstone_hip_fof_lower_labels(cstone_hip_ctx* ctx, const uint32_t* component, uint32_t n, uint32_t first,
                                           uint32_t last, uint64_t* labels, uint32_t* changed)
{
    if (!ctx || !component || !labels || !changed || last < first || last > n)
        return fail(ctx, CSTONE_E_ARG, "fof_lower_labels: bad argument");
    if (n == 0) return CSTONE_OK;
    CS_TRY(arenaReserve(ctx, alignUp(size_t(n) * sizeof(uint64_t)) + 256));
    uint64_t* minOf     = static_cast<uint64_t*>(arenaTake(ctx, alignUp(size_t(n) * sizeof(uint64_t))));
    const unsigned grid = gridFor(n, 256);
    hipLaunchKernelGGL(fofFillOnesKernel, grid, 256, 0, ctx->stream, minOf, n);
    hipLaunchKernelGGL(fofLowerMinKernel, grid, 256, 0, ctx->stream, component, n, labels, minOf, ctx->devScalars + 63);
    hipLaunchKernelGGL(fofLowerBroadcastKernel, grid, 256, 0, ctx->stream, component, n, first, last, minOf, labels, changed);
    arenaReset(ctx);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(ctx, CSTONE_E_HIP, "fof_lower_labels: %s", hipGetErrorString(e));
    return CSTONE_OK;
}

extern "C" int cstone_hip_friends_of_friends(cstone_hip_ctx* ctx, int real_bits, const void* x, const void* y, const void* z,
                                             uint32_t first, uint32_t last, const cstone_box* box_host,
                                             const int32_t* child_offsets, const int32_t* internal_to_leaf,
                                             const uint32_t* layout, const void* centers, const void* sizes,
                                             double linking_length, uint32_t* labels, uint32_t* group_sizes,
                                             uint32_t* num_groups)
{
    if (!ctx || !x || !y || !z || !box_host || !child_offsets || !internal_to_leaf || !layout || !centers || !sizes ||
        !labels || last < first)
        return fail(ctx, CSTONE_E_ARG, "friends_of_friends: bad argument");
    if (real_bits != 32 && real_bits != 64)
        return fail(ctx, CSTONE_E_ARG, "friends_of_friends: real_bits %d unsupported", real_bits);
    if (!(linking_length > 0.0)) // (a NaN fails the comparison)
        return fail(ctx, CSTONE_E_ARG, "friends_of_friends: linking length %g is not > 0", linking_length);
    for (int d = 0; d < 3; ++d)
    {
        // the relation is symmetric only while a pair has ONE periodic image within b
        const double len = box_host->lim[2 * d + 1] - box_host->lim[2 * d];
        if (box_host->bc[d] == 1 && !(linking_length < 0.5 * len))
            return fail(ctx, CSTONE_E_ARG, "friends_of_friends: linking length %g is not below half the periodic edge %g",
                        linking_length, len);
    }
    if (last == first) return CSTONE_OK;

    const uint32_t n    = last - first;
    const unsigned grid = gridFor(n, 256);
    uint32_t* count     = nullptr;
    uint32_t* numRoots  = nullptr;
    if (group_sizes || num_groups)
    {
        const size_t countBytes = group_sizes ? alignUp(size_t(n) * sizeof(uint32_t)) : 0;
        CS_TRY(arenaReserve(ctx, countBytes + 1024));
        numRoots = static_cast<uint32_t*>(arenaTake(ctx, 256));
        if (group_sizes) count = static_cast<uint32_t*>(arenaTake(ctx, countBytes));
        hipError_t e = hipMemsetAsync(numRoots, 0, sizeof(uint32_t), ctx->stream);
        if (e == hipSuccess && count) e = hipMemsetAsync(count, 0, size_t(n) * sizeof(uint32_t), ctx->stream);
        if (e != hipSuccess)
        {
            arenaReset(ctx);
            return fail(ctx, CSTONE_E_HIP, "friends_of_friends: %s", hipGetErrorString(e));
        }
    }
    hipLaunchKernelGGL(fofInitKernel, grid, 256, 0, ctx->stream, labels, first, n);
    {
        StageTimer timer(ctx, CSTONE_STAGE_FOF);
        if (real_bits == 32)
            launchLink<float>(ctx, x, y, z, first, last, *box_host, child_offsets, internal_to_leaf, layout, centers, sizes,
                              linking_length, labels);
        else
            launchLink<double>(ctx, x, y, z, first, last, *box_host, child_offsets, internal_to_leaf, layout, centers, sizes,
                               linking_length, labels);
    }
    hipLaunchKernelGGL(fofFlattenKernel, grid, 256, 0, ctx->stream, labels, first, n, num_groups ? numRoots : nullptr);
    if (group_sizes)
    {
        hipLaunchKernelGGL(fofCountKernel, grid, 256, 0, ctx->stream, labels, first, n, count);
        hipLaunchKernelGGL(fofBroadcastKernel, grid, 256, 0, ctx->stream, labels, first, n, count, group_sizes);
    }
    int rc = CSTONE_OK;
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        rc = fail(ctx, CSTONE_E_HIP, "friends_of_friends: %s", hipGetErrorString(e));
    // the only synchronisation of the call, and only when the number of groups is asked for
    if (rc == CSTONE_OK && num_groups) rc = copyToHost(ctx, num_groups, numRoots, sizeof(uint32_t));
    arenaReset(ctx);
    return rc;
}

extern "C" int cstone_hip_fof_catalog(cstone_hip_ctx* ctx, const uint32_t* labels, uint32_t first, uint32_t last,
                                      uint32_t min_members, uint32_t* group_offsets, size_t capacity, uint32_t* members,
                                      uint32_t* num_groups)
{
    if (!ctx || !labels || !group_offsets || !members || !num_groups || last < first)
        return fail(ctx, CSTONE_E_ARG, "fof_catalog: bad argument");
    const size_t n = size_t(last) - first;
    if (n >= (size_t(1) << 30)) return fail(ctx, CSTONE_E_ARG, "fof_catalog: %zu particles, the sort takes fewer than 2^30", n);
    if (min_members == 0) min_members = 1;
    if (n == 0)
    {
        *num_groups = 0;
        if (capacity < 1) return fail(ctx, CSTONE_E_CAPACITY, "fof_catalog: capacity 0");
        const uint32_t zero = 0;
        CS_HIP(ctx, hipMemcpyAsync(group_offsets, &zero, sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CSTONE_OK;
    }
    // slices: keys, values and their sort scratch; run ids; run starts (n + 1); keep, kept and their scans; two totals
    const size_t words = alignUp(n * sizeof(uint32_t)), words1 = alignUp((n + 1) * sizeof(uint32_t));
    const size_t tempBytes = cstone_hip_sort_pairs_temp_bytes(32, n);
    CS_TRY(arenaReserve(ctx, 9 * words + words1 + alignUp(tempBytes) + 3 * scanArenaBytes(n) + 4096));
    auto take      = [&](size_t bytes) { return static_cast<uint32_t*>(arenaTake(ctx, bytes)); };
    uint32_t *keys = take(words), *values = take(words), *keysAlt = take(words), *valuesAlt = take(words);
    void* temp     = arenaTake(ctx, alignUp(tempBytes) + 256);
    uint32_t *runId = take(words), *runStart = take(words1), *keep = take(words), *kept = take(words);
    uint32_t *outIdx = take(words), *outOff = take(words), *totals = take(256);
    const unsigned grid = gridFor(n, 256);
    int rc              = CSTONE_OK;
    hipError_t e = hipMemcpyAsync(keys, labels, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, CSTONE_E_HIP, "fof_catalog: %s", hipGetErrorString(e));
    if (rc == CSTONE_OK) rc = cstone_hip_sequence_u32(ctx, values, n, first);
    // the radix sort is stable: the members of a group stay in ascending order
    if (rc == CSTONE_OK) rc = cstone_hip_sort_pairs(ctx, 32, keys, values, n, keysAlt, valuesAlt, temp, tempBytes);
    if (rc == CSTONE_OK)
    {
        uint32_t* heads = keysAlt; // free again
        hipLaunchKernelGGL(fofHeadsKernel, grid, 256, 0, ctx->stream, keys, uint32_t(n), heads);
        rc = scanU32(ctx, heads, runId, n, 0u, true);
    }
    if (rc == CSTONE_OK)
    {
        hipLaunchKernelGGL(fofRunStartsKernel, grid, 256, 0, ctx->stream, keys, runId, uint32_t(n), runStart);
        hipLaunchKernelGGL(fofKeepKernel, grid, 256, 0, ctx->stream, runStart, runId, uint32_t(n), min_members, keep, kept);
        rc = scanU32(ctx, keep, outIdx, n, 0u, false, totals);
    }
    if (rc == CSTONE_OK) rc = scanU32(ctx, kept, outOff, n, 0u, false, totals + 1);
    if (rc == CSTONE_OK)
    {
        hipLaunchKernelGGL(fofFillKernel, grid, 256, 0, ctx->stream, values, runId, runStart, keep, outIdx, outOff, totals,
                           uint32_t(n), uint32_t(std::min<size_t>(capacity, 0xffffffffu)), group_offsets, members);
        if (hipError_t le = hipGetLastError(); le != hipSuccess)
            rc = fail(ctx, CSTONE_E_HIP, "fof_catalog: %s", hipGetErrorString(le));
    }
    if (rc == CSTONE_OK) rc = copyToHost(ctx, num_groups, totals, sizeof(uint32_t));
    arenaReset(ctx);
    CS_TRY(rc);
    if (size_t(*num_groups) + 1 > capacity)
        return fail(ctx, CSTONE_E_CAPACITY, "fof_catalog: %u groups need %u entries, capacity %zu", *num_groups,
                    *num_groups + 1, capacity);
    return CSTONE_OK;
}
