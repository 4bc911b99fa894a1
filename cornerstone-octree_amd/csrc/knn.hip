// Exact k nearest neighbours of ARBITRARY points on the octree for gfx950.  The rule is stated in include/cstone_hip.h,
// cstone_hip_knn: the brute force over all (query, particle) pairs with the offset, the fold and d2 of the sphere queries,
// the candidates ordered by (d2, index).  The tree only prunes.
//
// Shape: ONE WAVE PER QUERY, one wave per workgroup, the walk of sphereProfilesKernel (sphere.hip): up to 8 nodes leave the
// LDS stack per step, lane l tests child l & 7 of node l >> 3, the opened leaves are read 64 particles at a time (lane l
// loads particle base + l, coalesced) and every lane forms the KEY of its own particle.
//
// Key.  (bits of d2, j).  d2 is a sum of squares, so it is >= +0 or a NaN, and the bit patterns of the non-negative reals
// ascend with them as unsigned integers: the order of the rule, (d2, j) lexicographic, is the order of the keys -- one u64
// in f32, a u64 and a u32 in f64.  Keys of different particles differ (j does).
//   NONE    = all ones: a lane without a particle, the excluded index.  Above every other key.
//   LIMIT   = (bits of r2, 0), r2 = r_q * r_q or +inf: a candidate has d2 < r2, hence a key BELOW LIMIT whatever its j;
//             any other particle has d2 >= r2 or a NaN d2 (bits above those of +inf, with or without the sign), hence a
//             key >= LIMIT.  "key < LIMIT" IS the candidate test.  r2 = 0 or NaN: LIMIT = (0, 0), nothing is below it.
//
// The k-best list.  64 R keys in registers, R = ceil(k / 64) rounded up to 1, 2 or 4: register r of lane l is element
// 64 r + l, ascending, filled with LIMIT at the start.  tau = element k - 1: the k-th best key so far, LIMIT while fewer
// than k candidates are held.  A chunk of 64 keys contributes only if a ballot of key < tau is non-empty -- after the first
// few leaves almost none does.  One that does is sorted by the network of resort.hip (waveSort64: 21 compare-exchange
// steps over DPP and v_permlane16/32_swap, here on keys of 2 or 3 words; wave_lanes.hpp), then merged: the top register
// takes the minimum against the MIRRORED chunk (lane ^ 63) -- the chunk padded with NONE to 64 R keys and reversed meets
// the list only there --, which leaves the 64 R smallest keys of list and chunk as a bitonic sequence; half-cleaners at
// distances 128, 64 (between registers) and 32 .. 1 (within) sort it.  k in 65 .. 256 stays in registers too: 4 x 3 words
// at most, and the merge then needs no LDS traffic at all; the kernels take 30 .. 53 VGPRs.
// Elements k .. 64 R - 1 are kept but never written out.  Nothing here depends on the order the chunks arrive in: the
// list is always the 64 R smallest keys below LIMIT seen so far, and every particle is seen at most once.
//
// Order of the walk.  tau must come down before pruning can work, so the walk first descends to ONE leaf, level by level
// into the child whose box is nearest to the query (ties: the first child), and merges it.  The batched walk follows and
// leaves that leaf out (a particle fed twice would be held twice).  What a step pushes is sorted by node distance with
// the same network, nearest on top, so that the 8 nodes of the next step are the nearest of the batch.  The order changes
// how many particles are tested, never the result.
//
// Pruning.  A node may be skipped only if no particle in it can have a key below tau, i.e. only if every particle in it
// has d2 > t2 or (d2 == t2 and j above tau's) where t2 is the d2 of tau.  The margin of sphere.hip carries over with
// e = fl(sqrt(t2)) in the place of e_NB: per axis the node's clamped offset as computed is at most the particle's
// + 45 u L (u = eps / 2; the roundings of the two folds, of the key normalisation and of centre and size: all ABSOLUTE,
// derived at sphereProfilesKernel), over three axes < 64 eps L; the squares, the sums, the comparison and here the square root
// (one more relative rounding: a particle with d2 <= t2 has sqrt(d2) <= e (1 + u)) are covered by 1 + 16 eps.  Hence
//     skip iff  dist2_node > (fl(sqrt(t2)) * (1 + 16 eps) + 64 eps L)^2.
// A node at distance exactly sqrt(t2) is OPENED: a particle in it at exactly that distance with an index below tau's
// displaces tau, and with the margin the strict comparison is far from deciding that case anyway.  t2 = +inf (LIMIT of a
// query without radius, list not full) gives an infinite threshold: every node is opened.  !(>): a NaN anywhere opens
// the node and the particle test decides.  tau only descends, so a test against an older tau only opens too much.
//
// The walk, its stack and the stack's bound are those of wave_walk.hpp; the bound does not look at the order inside a batch.
//
// LDS per wave: the stack, 5 376 bytes.  No atomics except that error word.
#include <cmath>
#include <cstring>
#include <limits>

#include "cstone_hip_device.hpp"
#include "ctx.hpp"
#include "knn.hpp"
#include "wave_lanes.hpp"
#include "wave_walk.hpp"

namespace cship
{

namespace
{

template<class T>
struct KnnKey
{
    using Bits = std::conditional_t<sizeof(T) == 4, uint32_t, uint64_t>;
    Bits d;     // bit pattern of d2
    uint32_t j; // particle index (a node index where nodes are sorted)
};

template<class T>
__device__ __forceinline__ typename KnnKey<T>::Bits knnBits(T v)
{
    if constexpr (sizeof(T) == 4) return __float_as_uint(v);
    else
        return uint64_t(__double_as_longlong(v));
}
template<class T>
__device__ __forceinline__ T knnReal(typename KnnKey<T>::Bits b)
{
    if constexpr (sizeof(T) == 4) return __uint_as_float(b);
    else
        return __longlong_as_double((long long)(b));
}
template<class T>
__device__ __forceinline__ bool knnLess(const KnnKey<T>& a, const KnnKey<T>& b)
{
    if constexpr (sizeof(T) == 4) return ((uint64_t(a.d) << 32) | a.j) < ((uint64_t(b.d) << 32) | b.j);
    else
        return a.d < b.d || (a.d == b.d && a.j < b.j);
}
//! the key of lane ^ X
template<int X, class T>
__device__ __forceinline__ KnnKey<T> knnPartner(const KnnKey<T>& k, unsigned lane)
{
    KnnKey<T> o;
    if constexpr (sizeof(T) == 4) o.d = laneXor<X>(k.d, lane);
    else
        o.d = uint64_t(laneXor<X>(uint32_t(k.d), lane)) | (uint64_t(laneXor<X>(uint32_t(k.d >> 32), lane)) << 32);
    o.j = laneXor<X>(k.j, lane);
    return o;
}
//! the key of lane src (wave-uniform)
template<class T>
__device__ __forceinline__ KnnKey<T> knnReadLane(const KnnKey<T>& k, int src)
{
    KnnKey<T> o;
    if constexpr (sizeof(T) == 4) o.d = uint32_t(__builtin_amdgcn_readlane(int(k.d), src));
    else
        o.d = uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(k.d)), src))) |
              (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(k.d >> 32)), src))) << 32);
    o.j = uint32_t(__builtin_amdgcn_readlane(int(k.j), src));
    return o;
}

//! compare-exchange with the lane at distance X; the lane whose bit LOWBIT is clear keeps the smaller key
template<int X, unsigned LOWBIT, class T>
__device__ __forceinline__ void knnExchange(KnnKey<T>& v, unsigned lane)
{
    const KnnKey<T> o = knnPartner<X>(v, lane);
    const bool take   = (lane & LOWBIT) ? knnLess(v, o) : knnLess(o, v);
    if (take) v = o;
}
template<int J, class T>
__device__ __forceinline__ void knnHalfClean(KnnKey<T>& v, unsigned lane)
{
    if constexpr (J >= 1)
    {
        knnExchange<J, unsigned(J)>(v, lane);
        knnHalfClean<J / 2>(v, lane);
    }
}
//! ascending sort of the 64 keys of a wave: waveSort64 of resort.hip on keys
template<class T>
__device__ __forceinline__ void knnSort64(KnnKey<T>& v, unsigned lane)
{
    knnExchange<1, 1u>(v, lane);
    knnExchange<3, 2u>(v, lane), knnHalfClean<1>(v, lane);
    knnExchange<7, 4u>(v, lane), knnHalfClean<2>(v, lane);
    knnExchange<15, 8u>(v, lane), knnHalfClean<4>(v, lane);
    knnExchange<31, 16u>(v, lane), knnHalfClean<8>(v, lane);
    knnExchange<63, 32u>(v, lane), knnHalfClean<16>(v, lane);
}
//! registers a (the lower) and b of every lane: a keeps the smaller key
template<class T>
__device__ __forceinline__ void knnOrder(KnnKey<T>& a, KnnKey<T>& b)
{
    if (knnLess(b, a))
    {
        const KnnKey<T> t = a;
        a = b, b = t;
    }
}

//! the k-best list of one wave (see the head of the file)
template<class T, int R>
struct KnnList
{
    using Key = KnnKey<T>;
    Key v[R];
    Key tau;
    unsigned lane;
    int kr, kl; // element k - 1 is register kr of lane kl

    __device__ __forceinline__ void init(const Key& limit, uint32_t k, unsigned lane_)
    {
        lane = lane_;
        kr = int((k - 1) >> 6), kl = int((k - 1) & 63u);
#pragma unroll
        for (int r = 0; r < R; ++r)
            v[r] = limit;
        tau = limit;
    }
    //! COLLECTIVE: 64 keys, one per lane (NONE where a lane has none).  true iff the list changed
    __device__ __forceinline__ bool feed(Key c)
    {
        const bool below = knnLess(c, tau);
        if (__ballot(below) == 0) return false;
        if (!below) c.d = ~typename Key::Bits(0), c.j = ~0u;
        knnSort64(c, lane);
        const Key m = knnPartner<63>(c, lane);
        if (knnLess(m, v[R - 1])) v[R - 1] = m;
        if constexpr (R == 4) knnOrder(v[0], v[2]), knnOrder(v[1], v[3]);
        if constexpr (R >= 2) knnOrder(v[0], v[1]);
        if constexpr (R == 4) knnOrder(v[2], v[3]);
#pragma unroll
        for (int r = 0; r < R; ++r)
            knnHalfClean<32>(v[r], lane);
        Key t = v[0];
#pragma unroll
        for (int r = 1; r < R; ++r)
            if (kr == r) t = v[r];
        tau = knnReadLane(t, kl);
        return true;
    }
};

// ---- where a finished list goes: slot(q, k, e, filled, key) for every e < k, then count(q, m)

//! cstone_hip_knn: absolute particle indices
template<class T>
struct KnnOutIndices
{
    uint32_t* neighbors;
    T* dist2;
    uint32_t* counts;
    __device__ __forceinline__ void slot(size_t q, uint32_t k, uint32_t e, bool filled, const KnnKey<T>& key) const
    {
        neighbors[q * k + e] = filled ? key.j : 0xFFFFFFFFu;
        if (dist2) dist2[q * k + e] = filled ? knnReal<T>(key.d) : std::numeric_limits<T>::infinity();
    }
    __device__ __forceinline__ void count(size_t q, uint32_t m) const
    {
        if (counts) counts[q] = m;
    }
};
//! the local search of cstone_hip_domain_mr_knn: records {d2 bits widened, global id}, all ones where unfilled
template<class T>
struct KnnOutRecords
{
    KnnRecord* records;
    uint64_t idBase; // global id of particle `first`
    uint32_t first;
    __device__ __forceinline__ void slot(size_t q, uint32_t k, uint32_t e, bool filled, const KnnKey<T>& key) const
    {
        KnnRecord r{~0ull, ~0ull};
        if (filled) r.d2 = uint64_t(key.d), r.id = idBase + (key.j - first);
        records[q * k + e] = r;
    }
    __device__ __forceinline__ void count(size_t, uint32_t) const {}
};
//! the merge of cstone_hip_domain_mr_knn: key.j = p * k + s names slot s of rank p's row, which holds the id
template<class T>
struct KnnOutMerged
{
    const KnnRecord* rows; // [numRanks][numQueries][k]
    uint32_t numQueries;
    uint64_t* ids;
    T* dist2;
    uint32_t* counts;
    __device__ __forceinline__ void slot(size_t q, uint32_t k, uint32_t e, bool filled, const KnnKey<T>& key) const
    {
        uint64_t id = ~0ull;
        if (filled) id = rows[(size_t(key.j / k) * numQueries + q) * k + key.j % k].id;
        ids[q * k + e] = id;
        if (dist2) dist2[q * k + e] = filled ? knnReal<T>(key.d) : std::numeric_limits<T>::infinity();
    }
    __device__ __forceinline__ void count(size_t q, uint32_t m) const
    {
        if (counts) counts[q] = m;
    }
};

//! the row of query q from the list: slots below k that hold a key below LIMIT are filled, the others unfilled
template<class T, int R, class Out>
__device__ __forceinline__ void knnWriteRow(const KnnList<T, R>& list, const KnnKey<T>& limit, size_t q, uint32_t k, const Out& out)
{
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
    {
        const uint32_t e  = 64u * r + list.lane;
        const bool filled = e < k && knnLess(list.v[r], limit);
        m += uint32_t(__popcll(__ballot(filled)));
        if (e < k) out.slot(q, k, e, filled, list.v[r]);
    }
    if (list.lane == 0) out.count(q, m);
}

template<class T>
__device__ __forceinline__ KnnKey<T> knnLimit(const T* __restrict__ rmax, size_t q)
{
    T r2 = std::numeric_limits<T>::infinity();
    if (rmax)
    {
        const T r = rmax[q];
        r2        = r * r;
    }
    KnnKey<T> limit;
    limit.d = r2 > T(0) ? knnBits<T>(r2) : 0; // (a NaN fails the comparison)
    limit.j = 0;
    return limit;
}

template<class T, int R, class Out>
__global__ __launch_bounds__(64) void knnKernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                uint32_t first, uint32_t last, cstone_hip::DeviceBox<T> box,
                                                cstone_hip::OctreeNsView<T> tree, const T* __restrict__ qc,
                                                const T* __restrict__ rmax, const uint32_t* __restrict__ qself, uint32_t k,
                                                T absMargin, Out out, int* __restrict__ errors)
{
    using Key = KnnKey<T>;
    __shared__ int32_t stack[WALK_STACK];

    const unsigned lane = threadIdx.x;
    const size_t q      = blockIdx.x;
    const T cx = qc[3 * q], cy = qc[3 * q + 1], cz = qc[3 * q + 2];
    const uint32_t self = qself ? qself[q] : 0xFFFFFFFFu;
    const bool px = box.bc[0] == 1, py = box.bc[1] == 1, pz = box.bc[2] == 1;

    const Key limit = knnLimit<T>(rmax, q);
    KnnList<T, R> list;
    list.init(limit, k, lane);

    const T eps = sizeof(T) == 4 ? T(1.1920928955078125e-07) : T(2.220446049250313e-16);
    T thr2;
    auto setThreshold = [&]()
    {
        const T thr = sqrt(knnReal<T>(list.tau.d)) * (T(1) + T(16) * eps) + absMargin;
        thr2        = thr * thr;
    };
    setThreshold();
    auto nodeD2 = [&](int32_t n) -> T { return walkNodeDist2(tree, box, n, cx, cy, cz); };
    // particles [jb, je) (wave-uniform), clipped to the range: the particle test, the authority
    auto scan = [&](uint32_t jb, uint32_t je)
    {
        jb = max(jb, first), je = min(je, last);
        bool changed = false;
        for (uint32_t base = jb; base < je; base += 64)
        {
            const uint32_t j = base + lane;
            Key c;
            c.d = ~typename Key::Bits(0), c.j = ~0u;
            if (j < je && j != self)
            {
                T dx = x[j] - cx, dy = y[j] - cy, dz = z[j] - cz;
                dx = cstone_hip::detail::foldAxis<T>(dx, box.len[0], box.inv[0], px);
                dy = cstone_hip::detail::foldAxis<T>(dy, box.len[1], box.inv[1], py);
                dz = cstone_hip::detail::foldAxis<T>(dz, box.len[2], box.inv[2], pz);
                const T d2 = dx * dx + dy * dy + dz * dz;
                c.d = knnBits<T>(d2), c.j = j;
            }
            changed |= list.feed(c);
        }
        if (changed) setThreshold();
    };

    // LIMIT = (0, 0): no candidate can exist
    const bool live = last > first && limit.d != 0;
    if (live)
    {
        // the leaf nearest to the query first
        int32_t seed = 0;
        while (tree.childOffsets[seed] != 0)
        {
            const int32_t child = tree.childOffsets[seed] + int32_t(lane & 7u);
            T d                 = nodeD2(child);
            int32_t at          = child;
#pragma unroll
            for (int offset = 4; offset; offset >>= 1)
            {
                const T od        = __shfl_xor(d, offset);
                const int32_t oat = __shfl_xor(at, offset);
                if (od < d || (od == d && oat < at)) d = od, at = oat;
            }
            seed = __builtin_amdgcn_readfirstlane(at);
        }
        {
            const int32_t leaf = tree.internalToLeaf[seed];
            scan(tree.layout[leaf], tree.layout[leaf + 1]);
        }

        T nd = T(0); // the distance of the child this lane tested last
        auto open = [&](int32_t child) -> bool
        {
            nd = nodeD2(child);
            return !(nd > thr2) && child != seed;
        };
        // what the leaves of a step brought tau down to may close nodes that were open a moment ago
        auto still = [&]() -> bool { return !(nd > thr2); };
        // nearest on top: sorted ascending by (distance, node), written downwards from the new top
        auto place = [&](int32_t* dst, bool push, uint64_t, int numPush, int32_t child)
        {
            if (numPush > 1)
            {
                Key n;
                n.d = push ? knnBits<T>(nd) : ~typename Key::Bits(0);
                n.j = push ? uint32_t(child) : ~0u;
                knnSort64(n, lane);
                if (int(lane) < numPush) dst[numPush - 1 - int(lane)] = int32_t(n.j);
            }
            else if (push) { dst[0] = child; }
        };
        walkBelowRoot(tree, stack, lane, errors, seed != 0, open, scan, still, place);
    }
    knnWriteRow(list, limit, q, k, out);
}

/*! The merge of cstone_hip_domain_mr_knn: one wave per query feeds the same list from the gathered rows instead of from
 *  leaves.  rows[p][q][0 .. k) is rank p's answer for query q, ascending by (d2, id), all ones where unfilled.  The ranks'
 *  id ranges ascend with p, so (d2, p, slot) orders the records as (d2, id) does: the key's second word is p * k + slot,
 *  and the id is read back from the record at the end.  LIMIT is the search's, so that unfilled slots are told apart the
 *  same way; every record is a candidate already. */
template<class T, int R>
__global__ __launch_bounds__(64) void knnMergeKernel(const KnnRecord* __restrict__ rows, int numRanks, uint32_t numQueries,
                                                     const T* __restrict__ rmax, uint32_t k, KnnOutMerged<T> out)
{
    using Key           = KnnKey<T>;
    const unsigned lane = threadIdx.x;
    const size_t q      = blockIdx.x;
    const Key limit     = knnLimit<T>(rmax, q);
    KnnList<T, R> list;
    list.init(limit, k, lane);
    for (int p = 0; p < numRanks; ++p)
    {
        const KnnRecord* row = rows + (size_t(p) * numQueries + q) * k;
        for (uint32_t base = 0; base < k; base += 64)
        {
            const uint32_t e = base + lane;
            Key c;
            c.d = ~typename Key::Bits(0), c.j = ~0u;
            if (e < k)
            {
                const uint64_t d = row[e].d2;
                if (d != ~0ull) c.d = typename Key::Bits(d), c.j = uint32_t(p) * k + e;
            }
            list.feed(c);
        }
    }
    knnWriteRow(list, limit, q, k, out);
}

template<class T, int R, class Out>
int launchKnnOut(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, uint32_t first, uint32_t last,
                 const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf, const uint32_t* layout,
                 const void* centers, const void* sizes, const void* qc, const void* rmax, const uint32_t* qself,
                 uint32_t numQueries, uint32_t k, const Out& out)
{
    cstone_hip::OctreeNsView<T> tree{childOffsets, internalToLeaf, layout, (const T*)centers, (const T*)sizes};
    hipLaunchKernelGGL((knnKernel<T, R, Out>), numQueries, 64, 0, ctx->stream, (const T*)x, (const T*)y, (const T*)z, first,
                       last, cstone_hip::makeDeviceBox<T>(box), tree, (const T*)qc, (const T*)rmax, qself, k,
                       nodeAbsMargin<T>(box, 64), out, ctx->devScalars + 63);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(ctx, CSTONE_E_HIP, "knn: %s", hipGetErrorString(e));
    return CSTONE_OK;
}

//! the instantiation for k
template<class T, class Out, class... Args>
int launchKnnFor(uint32_t k, Args... args)
{
    const int regs = knnListRegisters(k);
    return regs == 1 ? launchKnnOut<T, 1, Out>(args...) : regs == 2 ? launchKnnOut<T, 2, Out>(args...) : launchKnnOut<T, 4, Out>(args...);
}

template<class T, int R>
int launchKnnMerge(cstone_hip_ctx* ctx, const KnnRecord* rows, int numRanks, const void* rmax, uint32_t numQueries, uint32_t k,
                   uint64_t* ids, void* dist2, uint32_t* counts)
{
    hipLaunchKernelGGL((knnMergeKernel<T, R>), numQueries, 64, 0, ctx->stream, rows, numRanks, numQueries, (const T*)rmax, k,
                       KnnOutMerged<T>{rows, numQueries, ids, (T*)dist2, counts});
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(ctx, CSTONE_E_HIP, "knn merge: %s", hipGetErrorString(e));
    return CSTONE_OK;
}

} // namespace

int knnLocalRecords(cstone_hip_ctx* ctx, int realBits, const void* x, const void* y, const void* z, uint32_t first,
                    uint32_t last, const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf,
                    const uint32_t* layout, const void* centers, const void* sizes, const void* queryCenters,
                    const void* queryRmax, uint32_t numQueries, uint32_t k, uint64_t idBase, KnnRecord* records)
{
    if (numQueries == 0) return CSTONE_OK;
    if (realBits == 32)
        return launchKnnFor<float, KnnOutRecords<float>>(k, ctx, x, y, z, first, last, box, childOffsets, internalToLeaf, layout,
                                                         centers, sizes, queryCenters, queryRmax, (const uint32_t*)nullptr,
                                                         numQueries, k, KnnOutRecords<float>{records, idBase, first});
    return launchKnnFor<double, KnnOutRecords<double>>(k, ctx, x, y, z, first, last, box, childOffsets, internalToLeaf, layout,
                                                       centers, sizes, queryCenters, queryRmax, (const uint32_t*)nullptr,
                                                       numQueries, k, KnnOutRecords<double>{records, idBase, first});
}

int knnMergeRecords(cstone_hip_ctx* ctx, int realBits, const KnnRecord* rows, int numRanks, const void* queryRmax,
                    uint32_t numQueries, uint32_t k, uint64_t* ids, void* dist2, uint32_t* counts)
{
    if (numQueries == 0) return CSTONE_OK;
    const int regs = knnListRegisters(k);
#define CSTONE_KNN_MERGE(T, R) launchKnnMerge<T, R>(ctx, rows, numRanks, queryRmax, numQueries, k, ids, dist2, counts)
    if (realBits == 32) return regs == 1 ? CSTONE_KNN_MERGE(float, 1) : regs == 2 ? CSTONE_KNN_MERGE(float, 2) : CSTONE_KNN_MERGE(float, 4);
    return regs == 1 ? CSTONE_KNN_MERGE(double, 1) : regs == 2 ? CSTONE_KNN_MERGE(double, 2) : CSTONE_KNN_MERGE(double, 4);
#undef CSTONE_KNN_MERGE
}

} // namespace cship

using namespace cship;

extern "C" int cstone_hip_knn(cstone_hip_ctx* ctx, int real_bits, const void* x, const void* y, const void* z, uint32_t first,
                              uint32_t last, const cstone_box* box_host, const int32_t* child_offsets,
                              const int32_t* internal_to_leaf, const uint32_t* layout, const void* centers,
                              const void* sizes, const void* query_centers, const void* query_rmax,
                              const uint32_t* query_self, uint32_t num_queries, uint32_t k, uint32_t* neighbors, void* dist2,
                              uint32_t* counts)
{
    if (!ctx) return CSTONE_E_ARG;
    const bool pointers = x && y && z && box_host && child_offsets && internal_to_leaf && layout && centers && sizes &&
                          query_centers && neighbors;
    if (const char* why = knnRefusal(real_bits, k, first, last, num_queries, pointers))
        return fail(ctx, CSTONE_E_ARG, "knn: %s", why);
    if (num_queries == 0) return CSTONE_OK;

    if (real_bits == 32)
        return launchKnnFor<float, KnnOutIndices<float>>(k, ctx, x, y, z, first, last, *box_host, child_offsets, internal_to_leaf,
                                                         layout, centers, sizes, query_centers, query_rmax, query_self,
                                                         num_queries, k, KnnOutIndices<float>{neighbors, (float*)dist2, counts});
    return launchKnnFor<double, KnnOutIndices<double>>(k, ctx, x, y, z, first, last, *box_host, child_offsets, internal_to_leaf,
                                                       layout, centers, sizes, query_centers, query_rmax, query_self,
                                                       num_queries, k, KnnOutIndices<double>{neighbors, (double*)dist2, counts});
}

extern "C" uint32_t cstone_hip_knn_mr_chunk_queries(uint32_t num_queries, uint32_t k, int num_ranks, uint64_t cap_bytes)
{
    return knnChunkQueries(num_queries, k, num_ranks, cap_bytes);
}
