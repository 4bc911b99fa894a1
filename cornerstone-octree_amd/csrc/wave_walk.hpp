// The batched octree walk of ONE WAVE, shared by the kernels whose particle test is the authority and whose node test
// only prunes: sphereProfilesKernel (sphere.hip), knnKernel (knn.hip) and pairCountsKernel (pair_counts.hip).
// findHalosKernel (halos.hip) is a different walk: several waves per block, a lane mask per node, its own stack bound.
//
// One step: up to 8 nodes leave the LDS stack, lane l tests child l & 7 of node l >> 3, a ballot says which open children
// are leaves and which go back on the stack.  The opened leaves hand their layout ranges to the caller in lane order;
// ranges that touch (the children of one node are consecutive in SFC order) are handed over as one.  No lane mask
// travels with a node: the wave walks for one query, or for one group of targets.
//
// The stack.  Popping 8 nodes and pushing up to 64 children is a depth-first walk in batches, and it needs more room than
// the 160 entries of the one-node-at-a-time walks: a sphere that covers four full levels already has 176 entries pending.
// Bound: call what one step pushes a batch (at most 64 nodes) and label it with 1 + the lowest level among the nodes the
// step popped.  A step pops from the top: it consumes whole batches and at most a part of one further batch B; every node
// it pops has a level >= label(B), so its own batch, put above what is left of B, carries a label above B's.  So the
// labels of the live batches ascend strictly from the bottom of the stack to its top; they lie in 1 .. 20 (a node of the
// deepest level, 21, is a leaf and has no children; the root is no batch), hence never more than 1 + 20 * 64 entries --
// whatever the node test lets through, also when it lets everything through, and whatever the order inside a batch.
// WALK_STACK covers that; an overflow would still be caught and ORs 4 into the sticky error word like every walk here.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "cstone_hip_device.hpp"

namespace cship
{

constexpr int WALK_STACK = 64 * 21;

static_assert(CSTONE_PAIR_MAX_BINS == CSTONE_SPHERE_MAX_BINS, "one edges struct, and pairEdgesOk goes through sphereEdgesOk");

//! the bin edges of a call as a kernel argument
template<class T>
struct WalkEdges
{
    T e[CSTONE_SPHERE_MAX_BINS + 1]; // T(edges[b]), converted on the host
};

//! per axis |folded offset of node n's centre from c| - half size of n: how far c lies outside the node's box
template<class T>
__device__ __forceinline__ void walkNodeGap(const cstone_hip::OctreeNsView<T>& tree, const cstone_hip::DeviceBox<T>& box, int32_t n,
                                            T cx, T cy, T cz, T& dx, T& dy, T& dz)
{
    dx = tree.centers[3 * n] - cx, dy = tree.centers[3 * n + 1] - cy, dz = tree.centers[3 * n + 2] - cz;
    dx = cstone_hip::detail::foldAxis<T>(dx, box.len[0], box.inv[0], box.bc[0] == 1);
    dy = cstone_hip::detail::foldAxis<T>(dy, box.len[1], box.inv[1], box.bc[1] == 1);
    dz = cstone_hip::detail::foldAxis<T>(dz, box.len[2], box.inv[2], box.bc[2] == 1);
    dx = fabs(dx) - tree.sizes[3 * n], dy = fabs(dy) - tree.sizes[3 * n + 1], dz = fabs(dz) - tree.sizes[3 * n + 2];
}
template<class T>
__device__ __forceinline__ T walkClampedNorm2(T dx, T dy, T dz)
{
    dx = dx > T(0) ? dx : T(0), dy = dy > T(0) ? dy : T(0), dz = dz > T(0) ? dz : T(0);
    return dx * dx + dy * dy + dz * dz;
}
//! the squared distance of the point c to the box of node n
template<class T>
__device__ __forceinline__ T walkNodeDist2(const cstone_hip::OctreeNsView<T>& tree, const cstone_hip::DeviceBox<T>& box, int32_t n,
                                           T cx, T cy, T cz)
{
    T dx, dy, dz;
    walkNodeGap(tree, box, n, cx, cy, cz, dx, dy, dz);
    return walkClampedNorm2(dx, dy, dz);
}
//! the squared distance of the box with centre c and half extents h to the box of node n
template<class T>
__device__ __forceinline__ T walkNodeDist2(const cstone_hip::OctreeNsView<T>& tree, const cstone_hip::DeviceBox<T>& box, int32_t n,
                                           T cx, T cy, T cz, T hx, T hy, T hz)
{
    T dx, dy, dz;
    walkNodeGap(tree, box, n, cx, cy, cz, dx, dy, dz);
    return walkClampedNorm2(dx - hx, dy - hy, dz - hz);
}

/*! COLLECTIVE: the walk below the root if fromRoot says that the root is open and internal (wave-uniform), else nothing.
 *    open(child) -> bool      the node test, evaluated only by the lanes whose slot holds a node.  A NaN must open.
 *    leaves(begin, end)       wave-uniform: the particles of opened leaves, touching ranges merged
 *    still() -> bool          asked of the open internal children after the leaves of the step: push it?
 *    place(dst, push, pm, numPush, child)   writes the numPush children with push set (ballot pm) to dst[0 .. numPush);
 *                             the next step pops from the END of dst
 *  stack: WALK_STACK entries in LDS, the caller's.  LDS accesses of one wave are in program order. */
template<class T, class Open, class Leaves, class Still, class Place>
__device__ __forceinline__ void walkBelowRoot(const cstone_hip::OctreeNsView<T>& tree, int32_t* stack, unsigned lane, int* errors,
                                              bool fromRoot, Open&& open, Leaves&& leaves, Still&& still, Place&& place)
{
    int top = 0;
    if (fromRoot)
    {
        if (lane == 0) stack[0] = 0;
        top = 1;
    }
    while (top > 0)
    {
        const int take = min(top, 8);
        const int slot = int(lane >> 3);
        int32_t child  = 0;
        bool go = false, isLeaf = false;
        uint32_t jb = 0, je = 0;
        if (slot < take)
        {
            const int32_t par = stack[top - 1 - slot];
            child             = tree.childOffsets[par] + int32_t(lane & 7u);
            go                = open(child);
            if (go && tree.childOffsets[child] == 0)
            {
                isLeaf             = true;
                const int32_t leaf = tree.internalToLeaf[child];
                jb = tree.layout[leaf], je = tree.layout[leaf + 1];
            }
        }
        top -= take;
        // the opened leaves in lane order; ranges that touch are read as one
        uint64_t lm = __ballot(go && isLeaf);
        uint32_t rb = 0, re = 0;
        while (lm)
        {
            const int src = __ffsll((unsigned long long)lm) - 1;
            lm &= lm - 1;
            const uint32_t b = uint32_t(__builtin_amdgcn_readlane(int(jb), src));
            const uint32_t e = uint32_t(__builtin_amdgcn_readlane(int(je), src));
            if (b == re) { re = e; }
            else
            {
                if (re > rb) leaves(rb, re);
                rb = b, re = e;
            }
        }
        if (re > rb) leaves(rb, re);

        const bool push   = go && !isLeaf && still();
        const uint64_t pm = __ballot(push);
        const int numPush = __popcll(pm);
        if (top + numPush > WALK_STACK)
        {
            if (lane == 0) atomicOr(errors, 4);
            return;
        }
        place(stack + top, push, pm, numPush, child);
        top += numPush;
    }
}

/*! COLLECTIVE: the whole walk: nothing if the root is closed, its range if it is a leaf, else the walk below it with the
 *  default hooks: every open internal child is pushed, compacted in lane order.  (A leaf root falls through to the loop under
 *  the flag, as the hand-written loops had it: with a return there and the stack set up unconditionally the pair-count
 *  kernels spilt more SGPRs and one of their timings rose by 0.9 %; DESIGN.md, "The batched walk".) */
template<class T, class Open, class Leaves>
__device__ __forceinline__ void walkFromRoot(const cstone_hip::OctreeNsView<T>& tree, int32_t* stack, unsigned lane, int* errors,
                                             Open&& open, Leaves&& leaves)
{
    if (!open(0)) return;
    const bool internal = tree.childOffsets[0] != 0;
    if (!internal)
    {
        const int32_t leaf = tree.internalToLeaf[0];
        leaves(tree.layout[leaf], tree.layout[leaf + 1]);
    }
    walkBelowRoot(
        tree, stack, lane, errors, internal, open, leaves, [] { return true; },
        [lane](int32_t* dst, bool push, uint64_t pm, int, int32_t child)
        {
            if (push) dst[__popcll(pm & ((1ull << lane) - 1ull))] = child;
        });
}

/*! COLLECTIVE: the per-lane accumulators cnt[b][64] (and acc[b][64] with HAS_W) added over the 64 lanes of every bin by a
 *  butterfly (lane ^ 32, 16, ... 1: a fixed tree, and a + b is commutative, so every lane holds the same bits); lane b
 *  keeps bin b */
template<bool HAS_W>
__device__ __forceinline__ void walkBinTotals(const uint32_t* cnt, const double* acc, int nb, unsigned lane,
                                              unsigned long long& myCount, double& mySum)
{
    myCount = 0, mySum = 0.0;
    for (int b = 0; b < nb; ++b)
    {
        unsigned long long c = cnt[b * 64 + lane];
        double a             = HAS_W ? acc[b * 64 + lane] : 0.0;
        for (int offset = 32; offset; offset >>= 1)
        {
            c += __shfl_xor(c, offset);
            if (HAS_W) a += __shfl_xor(a, offset);
        }
        if (int(lane) == b) myCount = c, mySum = a;
    }
}

} // namespace cship
