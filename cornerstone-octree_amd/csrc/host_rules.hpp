// The host-side RULES the single-rank and the multi-rank Domain orchestration share (domain.hip, domain_mr.hip): plain
// C++ that includes nothing from HIP, so that a stand-alone program built with the host compiler can check it.  What
// needs a context or device buffers is in host_tree.hpp, which includes this file.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "cstone_hip.h"

namespace cship
{

//! octree levels of a key type (maxLevel<K>() of device_keys.hpp, R/tree/definitions.h:46-72), for host code without HIP
template<class K>
constexpr unsigned hostMaxLevel() { return 8 * sizeof(K) / 3; }

//! true if no limit of the two boxes differs
inline bool sameLimits(const cstone_box& a, const cstone_box& b) { return std::equal(a.lim, a.lim + 6, b.lim); }

/*! The box of a sync (makeGlobalBox + limitBoxShrinking, R/sfc/box.hpp:415-431, evaluated in T like the reference) from
 *  the box of the previous sync and the extents fitted to the particles, {min, max} per axis.  Periodic axes keep their
 *  limits whatever `fitted` holds for them; the first call takes the fitted extents as they are. */
template<class T>
cstone_box limitBoxShrinking(const cstone_box& prev, const double* fitted, bool firstCall)
{
    cstone_box next = prev;
    const T shrink  = T(0.05);
    for (int d = 0; d < 3; ++d)
    {
        const bool pbc   = prev.bc[d] == 1;
        const double fLo = pbc ? prev.lim[2 * d] : fitted[2 * d], fHi = pbc ? prev.lim[2 * d + 1] : fitted[2 * d + 1];
        if (firstCall) { next.lim[2 * d] = fLo, next.lim[2 * d + 1] = fHi; }
        else
        {
            const T lo = T(prev.lim[2 * d]), hi = T(prev.lim[2 * d + 1]);
            const T len = hi - lo;
            const T a = lo + shrink * len, b = hi - shrink * len;
            next.lim[2 * d]     = std::min(T(fLo), a);
            next.lim[2 * d + 1] = std::max(T(fHi), b);
        }
    }
    return next;
}

//! deepest non-empty level of a level-range array (hostMaxLevel<K>() + 2 entries) of a linked octree
template<class K, class Range>
int deepestLevel(const Range& levelRange)
{
    int deepest = 0;
    for (int l = 0; l <= int(hostMaxLevel<K>()); ++l)
        if (levelRange[l + 1] > levelRange[l]) deepest = l;
    return deepest;
}

/*! How many low digit passes a radix sort may skip.  Two particles whose keys agree in the digits above the deepest leaf
 *  level (+ margin) of the previous focus tree sit in the same leaf cell: such runs hold at most a bucket of particles and
 *  are ordered by a fix-up pass instead (sort.hip, fixupRunsKernel).  One level below the deepest leaves a run holds about
 *  bucket / 8 particles; larger buckets get more margin (the fix-up handles runs of up to 192). */
template<class K>
int partialSortStartPass(int deepestLeafLevel, uint32_t bucketFocus)
{
    const int margin  = 1 + (bucketFocus > 128) + (bucketFocus > 1024);
    const int lowBits = 3 * int(hostMaxLevel<K>()) - 3 * (deepestLeafLevel + margin);
    return std::max(0, lowBits / 8) & ~1;
}

//! what the re-sort reports in its flag word (resort.hpp): bits 0..2 are reasons to give up, bit 3 is advice to sortLeaves
constexpr int RESORT_GIVE_UP = 7, RESORT_LARGE_QUIET_TILES = 8;
//! syncs that go straight to the radix sort after a re-sort that was not accepted
constexpr int RESORT_BACKOFF_SYNCS = 4;
//! a re-sort is carried out if nothing overflowed and at most an eighth of the particles changed their leaf
inline bool resortAccepted(int flags, uint32_t movers, size_t n) { return (flags & RESORT_GIVE_UP) == 0 && movers <= n / 8; }

// what the client chose (cstone_hip_domain_set_sort_mode); the environment variables of the experiments override it.
// Read at every call: the tests switch them between syncs.
inline bool mayResort(int sortMode)
{
    return sortMode == CSTONE_SORT_INCREMENTAL && std::getenv("CSTONE_NO_RESORT") == nullptr &&
           std::getenv("CSTONE_FULL_SORT") == nullptr;
}
inline bool allDigits(int sortMode) { return sortMode == CSTONE_SORT_ALL_DIGITS || std::getenv("CSTONE_FULL_SORT") != nullptr; }

/*! Who sends what to whom in the particle exchange of a multi-rank sync, from the cut points of the assignment in this
 *  rank's sorted keys (P + 1) and the all-gathered rows of everybody's send counts (P rows of P + 1 words, word P = the
 *  status of that rank; not read for P = 1).  Every rank derives the same failedRank / badRank from the same rows. */
struct ExchangePlan
{
    std::vector<uint64_t> sendCounts, matrix; // what I send to rank p; matrix[src * P + dst]
    int failedRank = -1;                      // first rank whose status word is set (nothing below is filled then)
    int badRank    = -1;                      // first rank left without particles or with 2^30 or more ...
    uint64_t badArriving = 0;                 // ... and how many arrive there
    uint64_t movedAny = 0, mSend = 0, na = 0, nb = 0; // particles moving anywhere; that I send, keep and receive
};
inline ExchangePlan exchangePlan(int rank, int P, const std::vector<uint64_t>& cut, const std::vector<uint64_t>& rows)
{
    ExchangePlan e;
    e.sendCounts.resize(P), e.matrix.assign(size_t(P) * P, 0);
    for (int p = 0; p < P; ++p)
        e.sendCounts[p] = cut[p + 1] - cut[p];
    if (P == 1) e.matrix[0] = e.sendCounts[0];
    for (int p = 0; p < P && P > 1; ++p)
    {
        if (rows[size_t(p) * (P + 1) + P] != 0) { e.failedRank = p; return e; }
        std::copy_n(rows.begin() + size_t(p) * (P + 1), P, e.matrix.begin() + size_t(p) * P);
    }
    for (int q = 0; q < P; ++q)
    {
        uint64_t arriving = 0;
        for (int p = 0; p < P; ++p)
            arriving += e.matrix[size_t(p) * P + q];
        if (arriving == 0 || arriving >= (uint64_t(1) << 30)) { e.badRank = q, e.badArriving = arriving; return e; }
    }
    for (int p = 0; p < P; ++p)
    {
        for (int q = 0; q < P; ++q)
            if (p != q) e.movedAny += e.matrix[size_t(p) * P + q];
        if (p != rank) e.mSend += e.sendCounts[p], e.nb += e.matrix[size_t(p) * P + rank];
    }
    e.na = e.sendCounts[rank];
    return e;
}

/*! The result arrays of a multi-rank sync: the nm assigned particles are written once, at slot M of arrays of cap
 *  elements, with room on both sides for the halos, whose number is only known later: twice those of the previous sync
 *  (a quarter of nm on the first call) and a page.  M is a multiple of 4 elements: the assigned range the client passes
 *  back as the next input then starts on a 16-byte boundary, which the next sync's vector loads need. */
struct ResultMargins { uint64_t M, cap; };
inline ResultMargins resultMargins(uint64_t nm, uint64_t prevLo, uint64_t prevHi, bool firstCall, bool margins)
{
    if (!margins) return {0, nm};
    const uint64_t first = firstCall ? nm / 4 : 0;
    const uint64_t M     = (std::max(2 * prevLo + 4096, first) + 3) & ~uint64_t(3);
    return {M, M + nm + std::max(2 * prevHi + 4096, first)};
}
//! ... once nlo halos below and nhi above are known: the arrays handed out start at off; where the margins were too small
//! the block must move to slot M2 (again a multiple of 4) of arrays of cap2 elements
struct BlockWithHalos { bool move; uint64_t M2, cap2, off; };
inline BlockWithHalos blockWithHalos(uint64_t M, uint64_t cap, uint64_t nm, uint64_t nlo, uint64_t nhi)
{
    if (nlo <= M && M + nm + nhi <= cap) return {false, M, cap, M - nlo};
    const uint64_t M2 = (nlo + 3) & ~uint64_t(3);
    return {true, M2, M2 + nm + nhi, M2 - nlo};
}

/*! One update step of the (small, replicated) GLOBAL tree on the host: the decision of nodeOp (tree.hip,
 *  R/tree/csarray.hpp:270-310) and the expansion of rebalanceKernel (R/tree/csarray.hpp:360-385), restated for the host
 *  copies of the leaf array and the all-reduced counts that the last sync read back anyway.  The device then only counts
 *  (and reduces): the read-back between decision and rebalance of cstone_hip_update_octree disappears from a steady-state
 *  sync.  Returns true if every node op is "keep" (the leaf array is unchanged). */
template<class K>
bool globalTreeStepHost(const std::vector<K>& tree, const std::vector<uint32_t>& counts, uint32_t bucket,
                        std::vector<K>& newTree)
{
    const int numNodes = int(counts.size());
    constexpr unsigned top = hostMaxLevel<K>();
    auto span = [](unsigned level) { return K(1) << (3u * (top - level)); };
    auto levelOf = [&](K s) // level of a node of key span s (a power of 8)
    {
        unsigned level = top;
        while (level > 0 && span(level) < s)
            --level;
        return level;
    };
    std::vector<uint32_t> ops(size_t(numNodes) + 1, 0);
    bool keepAll = true;
    for (int i = 0; i < numNodes; ++i)
    {
        const K start        = tree[i];
        const unsigned level = levelOf(K(tree[i + 1] - start));
        uint32_t op          = 1;
        bool merged          = false;
        if (level > 0)
        {
            const int sib = int((start >> (3u * (top - level))) & 7u);
            if (sib > 0)
            {
                const int first = i - sib;
                if (first >= 0 && first + 8 <= numNodes && tree[first + 8] == K(tree[first] + span(level - 1)))
                {
                    uint64_t parent = 0;
                    for (int k = 0; k < 8; ++k)
                        parent += counts[first + k];
                    merged = parent <= uint64_t(bucket);
                }
            }
        }
        if (merged) { op = 0; }
        else
        {
            const uint32_t c = counts[i];
            if (c > bucket * 512u && level + 3 < top) op = 4096;
            else if (c > bucket * 64u && level + 2 < top) op = 512;
            else if (c > bucket * 8u && level + 1 < top) op = 64;
            else if (c > bucket && level < top) op = 8;
        }
        ops[i]  = op;
        keepAll = keepAll && op == 1;
    }
    if (keepAll) return true;
    newTree.clear();
    for (int i = 0; i < numNodes; ++i)
    {
        const uint32_t cnt = ops[i];
        if (cnt == 0) continue;
        const K start        = tree[i];
        const unsigned level = levelOf(K(tree[i + 1] - start));
        unsigned down = 0; // cnt in {1, 8, 64, 512, 4096}: 0..4 levels down
        for (uint32_t c = cnt; c > 1; c /= 8)
            ++down;
        const K step = span(level + down);
        for (uint32_t j = 0; j < cnt; ++j)
            newTree.push_back(K(start + K(j) * step));
    }
    newTree.push_back(tree[numNodes]);
    return false;
}

} // namespace cship
