// Lock-free union-find on an array of parents, for the friends-of-friends group finder (fof.hip).  Plain C++ that includes
// nothing from HIP and is templated on the atomic operations, so that the SAME text runs in the link kernel (agent-scope
// atomics on the label array) and in a stand-alone host program with std::atomic (tests/union_find_check.cpp), where
// threads, sanitizers and an injected failing compare-and-swap can get at it.
//
// The forest.  parent[v] is a vertex; a vertex with parent[v] == v is a root.  Invariant, from the initial parent[v] = v
// to the end:   parent[v] <= v,   and parent[v] lies in the connected component of v   (component of the graph whose
// edges have been handed to ufUnite so far).  Every chain v, parent[v], parent[parent[v]] ... therefore strictly decreases
// until it stops at a root, so ufFind ends, and a root is the smallest vertex of its tree.  The only write that changes a
// root is the compare-and-swap of ufUnite, which hooks the LARGER of two roots under the smaller; a vertex that has
// stopped being a root never becomes one again.  When all unions are done the trees are the components, and every root
// is the minimum of its component: the label that ufFind returns does not depend on the order the unions were made in.
//
// Ops:   uint32_t load(uint32_t v) const                          -- parent[v], a real (relaxed atomic) load
//        uint32_t cas(uint32_t v, uint32_t expect, uint32_t set)  -- compare-and-swap on parent[v], returns what it found
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define CSTONE_UF_FN __host__ __device__ inline
#else
#define CSTONE_UF_FN inline
#endif

namespace cship
{

/*! failed compare-and-swaps that ONE ufUnite puts up with.  Under the invariant a failed one returns a value below the
 *  root it was tried on, so their number is bounded by the vertex index without any cap and is a handful in practice (one
 *  per race lost); the cap bounds the loop for memory that breaks the invariant, where it would be a spin otherwise. */
constexpr uint32_t ufRetryCap = 1u << 20;

/*! the root of v's tree.  A stale read is harmless: every value parent[v] has ever held is a vertex of v's component
 *  that is <= v, so an outdated chain still descends and still ends inside the component, at a vertex that was a root
 *  when it was read.  p > v cannot be read under the invariant; it ends the walk like a root does. */
template<class Ops>
CSTONE_UF_FN uint32_t ufFind(const Ops& ops, uint32_t v)
{
    for (;;)
    {
        const uint32_t p = ops.load(v);
        if (p >= v) return v;
        v = p;
    }
}

/*! joins the trees of a and b and returns the root of the joined tree as this thread knows it (a vertex that was the
 *  root when it was last read: the caller may keep it to start its next find from).  Lock-free: find both roots, hook the
 *  larger under the smaller with one compare-and-swap that expects it to be a root still.  A stale root -- read before
 *  another thread hooked it -- only makes the compare-and-swap fail: it returns the true parent, which is smaller, and
 *  the search goes on from there; the smaller root may be stale too, and hooking under a vertex that is no root any more
 *  keeps the invariant just the same.  Every failure lowers the larger of the two roots, so the loop ends; retryCap
 *  bounds it even for a compare-and-swap that fails without such a value.  *gaveUp is set (never cleared) when the cap
 *  was reached: the two trees may then still be separate. */
template<class Ops>
CSTONE_UF_FN uint32_t ufUnite(const Ops& ops, uint32_t a, uint32_t b, uint32_t retryCap, bool* gaveUp)
{
    uint32_t ra = ufFind(ops, a), rb = ufFind(ops, b);
    for (uint32_t failures = 0; ra != rb;)
    {
        const uint32_t hi = ra < rb ? rb : ra, lo = ra < rb ? ra : rb;
        const uint32_t seen = ops.cas(hi, hi, lo);
        if (seen == hi) return lo;
        if (++failures >= retryCap)
        {
            *gaveUp = true;
            return lo;
        }
        // hi has been hooked meanwhile: its parent is smaller.  (seen > hi breaks the invariant: try again, up to the cap)
        ra = seen < hi ? ufFind(ops, seen) : hi;
        rb = lo;
    }
    return ra;
}

/*! shortens v's chain to r, a vertex found from v's chain (ufFind, ufUnite), with ONE attempt: r <= v and r is in v's
 *  component, so the write keeps the invariant; if it fails, somebody else has shortened the chain.  v is not a root when
 *  r < v, so this never competes with the hook of ufUnite for the meaning of "root". */
template<class Ops>
CSTONE_UF_FN void ufCompress(const Ops& ops, uint32_t v, uint32_t r)
{
    const uint32_t p = ops.load(v);
    if (r < p && p <= v) (void)ops.cas(v, p, r);
}

} // namespace cship
