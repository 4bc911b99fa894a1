// Pair counts in radial bins on the octree for gfx950: DD(r), the histogram behind the two-point correlation function.  The
// rule is stated in include/cstone_hip.h, cstone_hip_pair_counts: the brute force over all ordered (target, source) pairs
// with the offset, the fold and d2 in the coordinate type, half-open bins on the squared edges, sums in double.  The tree
// only prunes.
//
// Shape: ONE WAVE PER 64 CONSECUTIVE TARGETS, one wave per workgroup -- the third kind of walk here.  The neighbour walk
// (cstone_hip_device.hpp) shares a traversal among 64 targets too, but its node test decides what is reported; the sphere
// walk (sphere.hip) lets the pair test decide, but pays one traversal per query.  This one shares the traversal AND leaves
// the decision to the pair test.
//   box          the wave forms the exact bounding box of its targets by wave reductions (lanes past the end of the range
//                repeat the wave's last target); centre and half size are rounded from it, which the margin allows for.
//                Where the 64 targets are spread over far more than the bins reach, the wave walks once per group of 32, 16,
//                ... 1 lanes instead, each with its own box (the same butterfly gives the groups' bounds): the largest group
//                size whose boxes all have a half extent of at most 2 e_NB.  Without this one wave of the outskirts of a
//                Plummer sphere, whose box holds the core, tests every particle of the core for all its lanes.
//   node tests   64 at a time, as sphereProfilesKernel does: up to 8 nodes leave the stack, lane l tests child l & 7 of node
//                l >> 3 against the group's box inflated by e_NB, a ballot says which children are leaves and which go back
//                on the stack.  No lane mask travels with a node: a node is open for the whole group or for nobody.
//   leaves       ranges of opened leaves that touch are merged, clipped to [first, last) and read 64 particles at a time:
//                lane l loads x, y, z, w of particle base + l (coalesced); the loop over k hands particle k round by
//                v_readlane and every lane tests it against ITS OWN target.  Most tested particles lie outside every bin,
//                so one compare against e2_0 and e2_NB comes first; who passes finds the bin by a binary search over e2 in
//                LDS (log2 NB steps) and adds to its own accumulator cnt[b][l] (acc[b][l] with weights) in LDS.
//                cnt[b][l] lies b * 256 + l * 4 bytes into its array, acc[b][l] b * 512 + l * 8: whatever b each lane picks,
//                the lanes of an access group hit distinct banks.  No atomics.
//   weights      HAS_W is a template argument: the unweighted kernel carries no double accumulators, 256 NB bytes of LDS
//                per wave instead of 768 NB.
//   rows         a workgroup takes the waves g, g + G, g + 2 G, ... of targets (G = gridDim.x, a function of the ranges
//                alone) and keeps its accumulators across them.  At the end the 64 lanes of every bin are added by a
//                butterfly (lane ^ 32, 16, ... 1: a fixed tree, a + b is commutative, every lane holds the same bits) and
//                the workgroup writes ONE partial row to the context's workspace.
//   finish       pairCountsFinishKernel, one workgroup per bin: thread t adds the rows t, t + 256, ... in ascending order,
//                the 256 partial results are added by a fixed tree in LDS.  With G a function of the ranges, the order of
//                every sum is fixed by the octree, the ranges and this shape; no floating-point atomics anywhere, and no
//                integer ones either (the sticky error word aside).
//
// The walk, its stack and the stack's bound are those of wave_walk.hpp; the bound holds whatever the node test lets through,
// also when it lets everything through (an open box with e_NB beyond its diagonal).
//
// LDS per wave: 256 NB (768 NB with weights) + 66 reals (e2) + 5 376 (stack): 21.5 KiB at NB = 64 without weights, 54 KiB
// with them.
#include <cmath>
#include <cstring>

#include "cstone_hip_device.hpp"
#include "ctx.hpp"
#include "node_margin.hpp"
#include "pair_counts.hpp"
#include "sphere.hpp"
#include "wave_walk.hpp"

namespace cship
{

namespace
{

constexpr int PAIR_E2_PAD = CSTONE_PAIR_MAX_BINS + 2; // e2[0 .. NB], padded to an even count: the stack stays 8-aligned
//! partial rows of a call at most (workgroups of the walk); more only where a lane's 32-bit count could wrap otherwise
constexpr uint32_t PAIR_ROWS = 8192;

template<class T>
constexpr size_t pairLdsBytes(int nb, bool hasW)
{
    return size_t(nb) * 64 * (sizeof(uint32_t) + (hasW ? sizeof(double) : 0)) + PAIR_E2_PAD * sizeof(T) +
           WALK_STACK * sizeof(int32_t);
}

/*! The margin of the node test, and why its absolute term is nodeAbsMargin(box, 256).  A node may be skipped only if NO
 *  particle p in it passes the pair test d2 < e2_NB of ANY of the wave's targets t.  Per axis a, with u = eps / 2 the unit roundoff of T and L the largest of |lo_a|, |hi_a| and
 *  len_a over the axes:
 *
 *    In exact arithmetic the folded offset has the magnitude g(d) = distance of d to the nearest multiple of len, and g is
 *    1-Lipschitz.  With c_n, s_n the node's centre and half size and c_b, s_b those of the targets' box,
 *    p - t = (c_n - c_b) + (p - c_n) - (t - c_b), so  g(p - t) >= g(c_n - c_b) - s_n - s_b  -- whichever images the two
 *    folds pick.  What the kernel computes differs from that by ABSOLUTE errors, and here BOTH boxes bring cancellation:
 *      - the pair's offset d = fl(p - t) is off by u |d| <= 2 u L; d * inv carries 3 relative roundings, so rint may pick
 *        the neighbouring image only when d is within 6 u L of half a box length, where both images have magnitudes
 *        within 12 u L of each other; len * k is exact for the k that occur, the subtraction adds u L: < 16 u L.  The
 *        same for the offset of the two centres: 32 u L together (as in sphere.hip).
 *      - the particle is "in" the node by its SFC key, while the node's centre and half size are rounded from the grid:
 *        it can lie outside [c_n - s_n, c_n + s_n] by < 12 u L (sphere.hip).
 *      - the targets' box: lo and hi are exact (a minimum and a maximum), s_b = fl((hi - lo) / 2) is off by u (hi - lo)
 *        <= 2 u L (the halving is exact), c_b = fl(lo + s_b) by another 2 u L: a target can lie outside
 *        [c_b - s_b, c_b + s_b] by < 6 u L.
 *      - (|d_centres| - s_n) - s_b: two more roundings, 2 u L.
 *    So  max(|d_centres| - s_n - s_b, 0) <= |d_pair| + 52 u L  per axis as computed.  Targets that are no particles (the
 *    cross counts) may lie up to two box lengths outside a periodic box, where |t| <= 3 L and the terms that scale with the
 *    targets' magnitude (the two offsets and the box: 38 u L of the 52) triple: 128 u L.  The kernel allows twice that,
 *    256 u L = 128 eps L per axis.  Over three axes the boxes' distance exceeds the pair's sqrt(d2) by at most
 *    sqrt(3) * 128 eps L < 256 eps L, and the squares, sums and the comparison with e2_NB = fl(e_NB * e_NB) add a few
 *    RELATIVE roundings on both sides, covered by the factor 1 + 16 eps.
 *    Hence:  skip iff  dist2_boxes > (e_NB * (1 + 16 eps) + 256 eps L)^2.
 *
 *  The relative term alone covers nothing when e_NB is a few ulps of the coordinates: tests/test_pair_counts.py (cell
 *  faces) counts the pairs a relative-only margin loses.
 *
 *  Sources: x, y, z, w over [first, last).  Targets: tx, ty, tz, tw over [tFirst, tLast) -- the same arrays for the auto
 *  counts (EXCL: a target is no partner of itself, BY INDEX), the sorted queries for the cross counts.  tw == nullptr with
 *  HAS_W: every target weighs 1. */
template<class T, class W, bool HAS_W, bool EXCL>
__global__ __launch_bounds__(64) void pairCountsKernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                       const W* __restrict__ w, uint32_t first, uint32_t last,
                                                       const T* __restrict__ tx, const T* __restrict__ ty,
                                                       const T* __restrict__ tz, const W* __restrict__ tw, uint32_t tFirst,
                                                       uint32_t tLast, cstone_hip::DeviceBox<T> box,
                                                       cstone_hip::OctreeNsView<T> tree, WalkEdges<T> edges, int nb,
                                                       T absMargin, uint32_t numWaves,
                                                       unsigned long long* __restrict__ rowCounts,
                                                       double* __restrict__ rowSums, unsigned long long* __restrict__ rowTests,
                                                       int* __restrict__ errors)
{
    extern __shared__ double pairLds[];
    double* acc    = pairLds;                                                      // [nb][64], HAS_W only
    uint32_t* cnt  = reinterpret_cast<uint32_t*>(pairLds + (HAS_W ? nb * 64 : 0)); // [nb][64]
    T* e2          = reinterpret_cast<T*>(cnt + nb * 64);                          // [nb + 1]
    int32_t* stack = reinterpret_cast<int32_t*>(e2 + PAIR_E2_PAD);

    const unsigned lane = threadIdx.x;
    const bool px = box.bc[0] == 1, py = box.bc[1] == 1, pz = box.bc[2] == 1;

    for (int b = int(lane); b <= nb; b += 64)
        e2[b] = edges.e[b] * edges.e[b];
    for (int b = 0; b < nb; ++b)
    {
        cnt[b * 64 + lane] = 0u;
        if (HAS_W) acc[b * 64 + lane] = 0.0;
    }
    __syncthreads();

    // the node test (its margin: above the kernel).  !(>): a NaN anywhere opens the node, the pair test then decides
    const T eps  = sizeof(T) == 4 ? T(1.1920928955078125e-07) : T(2.220446049250313e-16);
    const T thr  = edges.e[nb] * (T(1) + T(16) * eps) + absMargin;
    const T thr2 = thr * thr;
    const T e2lo = e2[0], e2hi = e2[nb];
    const T spread = T(2) * edges.e[nb]; // the half extent up to which targets share a box
    const int topStep = nb > 1 ? 1 << (31 - __clz(nb - 1)) : 0; // the largest power of two below nb

    unsigned long long tests = 0; // wave-uniform: distance tests issued for targets that exist

    for (uint32_t wave = blockIdx.x; wave < numWaves; wave += gridDim.x)
    {
        const uint32_t i0     = tFirst + wave * 64u; // < tLast: the wave's first target exists
        const uint32_t nValid = min(64u, tLast - i0);
        const bool valid      = lane < nValid;
        const uint32_t i      = i0 + (valid ? lane : nValid - 1u); // lanes past the end repeat the last target
        const T xi = tx[i], yi = ty[i], zi = tz[i];
        double wi = 1.0;
        if (HAS_W && tw) wi = double(tw[i]);

        // The targets' boxes: exact bounds by a butterfly.  After the step with offset o every lane holds the bounds of its
        // aligned group of 2 o lanes.  The wave walks once per group of gs lanes, gs the largest power of two whose groups
        // all have a half extent of at most 2 e_NB: 64 where the targets are as dense as the bins are wide -- one shared
        // traversal --, fewer where 64 consecutive targets are spread over far more than the bins reach (the outskirts of a
        // clustered cloud, bins much narrower than the particle spacing), where one box would open leaves that no target
        // needs, for all 64.  gs = 1 always qualifies.
        T lox = xi, loy = yi, loz = zi, hix = xi, hiy = yi, hiz = zi;
        T gLox = xi, gLoy = yi, gLoz = zi, gHix = xi, gHiy = yi, gHiz = zi;
        uint32_t gs = 1;
        for (int offset = 1; offset < 64; offset <<= 1)
        {
            T o;
            o = __shfl_xor(lox, offset), lox = o < lox ? o : lox;
            o = __shfl_xor(loy, offset), loy = o < loy ? o : loy;
            o = __shfl_xor(loz, offset), loz = o < loz ? o : loz;
            o = __shfl_xor(hix, offset), hix = o > hix ? o : hix;
            o = __shfl_xor(hiy, offset), hiy = o > hiy ? o : hiy;
            o = __shfl_xor(hiz, offset), hiz = o > hiz ? o : hiz;
            const T ex = hix - lox, ey = hiy - loy, ez = hiz - loz;
            const T e  = ex > ey ? (ex > ez ? ex : ez) : (ey > ez ? ey : ez);
            if (__ballot(e * T(0.5) > spread) != 0) break; // (a NaN extent does not split: its box opens every node)
            gs = 2u * uint32_t(offset);
            gLox = lox, gLoy = loy, gLoz = loz, gHix = hix, gHiy = hiy, gHiz = hiz;
        }

      for (uint32_t g0 = 0; g0 < nValid; g0 += gs)
      {
        // centre and half size of the group's box, rounded from its exact bounds (the margin allows for that)
        using cstone_hip::detail::readLane;
        const T blx = readLane(gLox, g0), bly = readLane(gLoy, g0), blz = readLane(gLoz, g0);
        const T hsx = (readLane(gHix, g0) - blx) * T(0.5), hsy = (readLane(gHiy, g0) - bly) * T(0.5),
                hsz = (readLane(gHiz, g0) - blz) * T(0.5);
        const T bcx = blx + hsx, bcy = bly + hsy, bcz = blz + hsz;
        const bool mine      = valid && lane >= g0 && lane < g0 + gs;
        const uint32_t nMine = min(gs, nValid - g0);

        auto near = [&](int32_t n) -> bool { return !(walkNodeDist2(tree, box, n, bcx, bcy, bcz, hsx, hsy, hsz) > thr2); };
        // particles [jb, je) (wave-uniform), clipped to the range: the pair test, the authority
        auto bin = [&](uint32_t jb, uint32_t je)
        {
            jb = max(jb, first), je = min(je, last);
            for (uint32_t base = jb; base < je; base += 64)
            {
                const uint32_t num = min(64u, je - base);
                T xl = T(0), yl = T(0), zl = T(0);
                double wl = 0.0;
                if (lane < num)
                {
                    xl = x[base + lane], yl = y[base + lane], zl = z[base + lane];
                    if (HAS_W) wl = double(w[base + lane]);
                }
                tests += (unsigned long long)num * nMine;
                for (uint32_t k = 0; k < num; ++k)
                {
                    const uint32_t j = base + k;
                    T dx = cstone_hip::detail::readLane(xl, k) - xi, dy = cstone_hip::detail::readLane(yl, k) - yi,
                      dz = cstone_hip::detail::readLane(zl, k) - zi;
                    double wj = 0.0;
                    if (HAS_W) wj = cstone_hip::detail::readLane(wl, k);
                    dx = cstone_hip::detail::foldAxis<T>(dx, box.len[0], box.inv[0], px);
                    dy = cstone_hip::detail::foldAxis<T>(dy, box.len[1], box.inv[1], py);
                    dz = cstone_hip::detail::foldAxis<T>(dz, box.len[2], box.inv[2], pz);
                    const T d2 = dx * dx + dy * dy + dz * dz;
                    if (mine && (!EXCL || j != i) && e2lo <= d2 && d2 < e2hi)
                    {
                        // the largest b < nb with e2[b] <= d2 (e2 does not descend, e2[0] <= d2 < e2[nb])
                        int b = 0;
                        for (int step = topStep; step; step >>= 1)
                        {
                            const int t = b + step;
                            if (t < nb && e2[t] <= d2) b = t;
                        }
                        const int slot = b * 64 + int(lane);
                        cnt[slot] += 1u;
                        if (HAS_W) acc[slot] += wi * wj;
                    }
                }
            }
        };

        walkFromRoot(tree, stack, lane, errors, near, bin);
      }
    }
    __syncthreads();

    unsigned long long myCount;
    double mySum;
    walkBinTotals<HAS_W>(cnt, acc, nb, lane, myCount, mySum);
    if (int(lane) < nb)
    {
        rowCounts[size_t(blockIdx.x) * nb + lane] = myCount;
        if (HAS_W) rowSums[size_t(blockIdx.x) * nb + lane] = mySum;
    }
    if (lane == 0) rowTests[blockIdx.x] = tests;
}

/*! The finish: workgroup b < nb adds column b of the partial rows -- thread t the rows t, t + 256, ... in ascending order,
 *  then the 256 partial results by a fixed tree --; workgroup nb adds the tests issued and all counts (the pairs binned)
 *  into stats[0 .. 2).  The order depends on numRows alone. */
__global__ __launch_bounds__(256) void pairCountsFinishKernel(const unsigned long long* __restrict__ rowCounts,
                                                              const double* __restrict__ rowSums,
                                                              const unsigned long long* __restrict__ rowTests, uint32_t numRows,
                                                              int nb, unsigned long long* __restrict__ counts,
                                                              double* __restrict__ sums, unsigned long long* __restrict__ stats)
{
    __shared__ unsigned long long cs[256], bs[256];
    __shared__ double ss[256];
    const unsigned t = threadIdx.x;
    const int b      = int(blockIdx.x);
    unsigned long long c = 0, binned = 0;
    double s = 0.0;
    if (b < nb)
    {
        for (uint32_t r = t; r < numRows; r += 256)
        {
            c += rowCounts[size_t(r) * nb + b];
            if (rowSums) s += rowSums[size_t(r) * nb + b];
        }
    }
    else
    {
        for (uint32_t r = t; r < numRows; r += 256)
            c += rowTests[r];
        for (size_t k = t; k < size_t(numRows) * nb; k += 256)
            binned += rowCounts[k];
    }
    cs[t] = c, bs[t] = binned, ss[t] = s;
    __syncthreads();
    for (unsigned half = 128; half; half >>= 1)
    {
        if (t < half) cs[t] += cs[t + half], bs[t] += bs[t + half], ss[t] += ss[t + half];
        __syncthreads();
    }
    if (t == 0)
    {
        if (b < nb)
        {
            counts[b] = cs[0];
            if (sums && rowSums) sums[b] = ss[0];
        }
        else
        {
            stats[0] = cs[0];
            stats[1] = bs[0];
        }
    }
}

//! AoS query centres to the three arrays the encode takes
template<class T>
__global__ __launch_bounds__(256) void pairSplitCentersKernel(const T* __restrict__ qc, uint32_t n, T* __restrict__ qx,
                                                              T* __restrict__ qy, T* __restrict__ qz)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    qx[q] = qc[3 * size_t(q)], qy[q] = qc[3 * size_t(q) + 1], qz[q] = qc[3 * size_t(q) + 2];
}

//! the queries in the order of their keys: centres and (optionally) weights
template<class T, class W>
__global__ __launch_bounds__(256) void pairGatherQueriesKernel(const T* __restrict__ qc, const W* __restrict__ qw,
                                                               const uint32_t* __restrict__ order, uint32_t n,
                                                               T* __restrict__ sx, T* __restrict__ sy, T* __restrict__ sz,
                                                               W* __restrict__ sw)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const size_t o = order[q];
    sx[q] = qc[3 * o], sy[q] = qc[3 * o + 1], sz[q] = qc[3 * o + 2];
    if (qw) sw[q] = qw[o];
}

//! what one walk needs of the context's workspace
struct PairRows
{
    unsigned long long* counts;
    double* sums;
    unsigned long long* tests;
    unsigned long long* stats;
};

//! workgroups of the walk: min(waves, PAIR_ROWS), more only where waves-per-workgroup x sources could wrap a lane's count
uint32_t pairNumRows(uint32_t numTargets, uint32_t numSources)
{
    const uint64_t waves = (uint64_t(numTargets) + 63) / 64;
    uint64_t rows        = std::min<uint64_t>(waves, PAIR_ROWS);
    if (rows == 0) return 0;
    const uint64_t perLane = std::max<uint64_t>(1, 0xFFFFFFFFull / std::max<uint64_t>(numSources, 1)); // waves a lane may take
    rows                   = std::max(rows, (waves + perLane - 1) / perLane);
    return uint32_t(std::min(rows, waves));
}

size_t pairRowsBytes(uint32_t rows, int nb)
{
    return 2 * alignUp(size_t(rows) * nb * 8) + alignUp(size_t(rows) * 8) + 256 + 1024;
}

PairRows takeRows(cstone_hip_ctx* ctx, uint32_t rows, int nb)
{
    PairRows r;
    r.counts = (unsigned long long*)arenaTake(ctx, size_t(rows) * nb * 8);
    r.sums   = (double*)arenaTake(ctx, size_t(rows) * nb * 8);
    r.tests  = (unsigned long long*)arenaTake(ctx, size_t(rows) * 8);
    r.stats  = (unsigned long long*)arenaTake(ctx, 16);
    return r;
}

template<class T, class W, bool HAS_W, bool EXCL>
int launchPairCounts(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* w, uint32_t first,
                     uint32_t last, const void* tx, const void* ty, const void* tz, const void* tw, uint32_t tFirst,
                     uint32_t tLast, const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf,
                     const uint32_t* layout, const void* centers, const void* sizes, const double* edgesHost, int nb,
                     uint32_t numRows, const PairRows& rows, uint64_t* counts, double* sums)
{
    cstone_hip::OctreeNsView<T> tree{childOffsets, internalToLeaf, layout, (const T*)centers, (const T*)sizes};
    WalkEdges<T> edges;
    std::memset(&edges, 0, sizeof edges);
    for (int b = 0; b <= nb; ++b)
        edges.e[b] = T(edgesHost[b]);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t));
    const uint32_t numWaves = (tLast - tFirst + 63u) / 64u;
    hipLaunchKernelGGL((pairCountsKernel<T, W, HAS_W, EXCL>), numRows, 64, pairLdsBytes<T>(nb, HAS_W), ctx->stream, (const T*)x,
                       (const T*)y, (const T*)z, (const W*)w, first, last, (const T*)tx, (const T*)ty, (const T*)tz,
                       (const W*)tw, tFirst, tLast, cstone_hip::makeDeviceBox<T>(box), tree, edges, nb, nodeAbsMargin<T>(box, 256),
                       numWaves, rows.counts, rows.sums, rows.tests, ctx->devScalars + 63);
    hipLaunchKernelGGL(pairCountsFinishKernel, nb + 1, 256, 0, ctx->stream, rows.counts, HAS_W ? rows.sums : nullptr, rows.tests,
                       numRows, nb, reinterpret_cast<unsigned long long*>(counts), sums, rows.stats);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(ctx, CSTONE_E_HIP, "pair_counts: %s", hipGetErrorString(e));
    return CSTONE_OK;
}

template<bool EXCL>
int dispatchPairCounts(cstone_hip_ctx* ctx, int realBits, int wBits, const void* x, const void* y, const void* z, const void* w,
                       uint32_t first, uint32_t last, const void* tx, const void* ty, const void* tz, const void* tw,
                       uint32_t tFirst, uint32_t tLast, const cstone_box& box, const int32_t* childOffsets,
                       const int32_t* internalToLeaf, const uint32_t* layout, const void* centers, const void* sizes,
                       const double* edgesHost, int nb, uint32_t numRows, const PairRows& rows, uint64_t* counts, double* sums)
{
#define CSTONE_PAIR_LAUNCH(T, W, HAS_W)                                                                                \
    launchPairCounts<T, W, HAS_W, EXCL>(ctx, x, y, z, w, first, last, tx, ty, tz, tw, tFirst, tLast, box, childOffsets,  \
                                        internalToLeaf, layout, centers, sizes, edgesHost, nb, numRows, rows, counts, sums)
    if (realBits == 32)
    {
        if (!w) return CSTONE_PAIR_LAUNCH(float, float, false);
        return wBits == 32 ? CSTONE_PAIR_LAUNCH(float, float, true) : CSTONE_PAIR_LAUNCH(float, double, true);
    }
    if (!w) return CSTONE_PAIR_LAUNCH(double, float, false);
    return wBits == 32 ? CSTONE_PAIR_LAUNCH(double, float, true) : CSTONE_PAIR_LAUNCH(double, double, true);
#undef CSTONE_PAIR_LAUNCH
}

//! empty targets: zeroed outputs
int pairZero(cstone_hip_ctx* ctx, int nb, uint64_t* counts, double* sums, uint64_t* statsHost)
{
    CS_HIP(ctx, hipMemsetAsync(counts, 0, size_t(nb) * 8, ctx->stream));
    if (sums) CS_HIP(ctx, hipMemsetAsync(sums, 0, size_t(nb) * 8, ctx->stream));
    if (statsHost)
    {
        CS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        statsHost[0] = statsHost[1] = 0;
    }
    return CSTONE_OK;
}

} // namespace

const char* pairCountsRefusal(int realBits, int wBits, bool wGiven, const cstone_box* box, const double* edges, int numBins)
{
    if (realBits != 32 && realBits != 64) return "real_bits unsupported";
    if (wGiven && wBits != 32 && wBits != 64) return "w_bits unsupported";
    if (numBins < 1 || numBins > CSTONE_PAIR_MAX_BINS || !sphereEdgesOk(edges, numBins))
        return "1 .. 64 bins with finite, non-negative, strictly ascending edges are taken";
    if (!box) return "null box";
    for (int d = 0; d < 3; ++d)
    {
        // one periodic image within the outer edge, as friends_of_friends asks of its linking length
        const double len = box->lim[2 * d + 1] - box->lim[2 * d];
        if (box->bc[d] == 1 && !(edges[numBins] < 0.5 * len)) return "the outer edge is not below half a periodic edge of the box";
    }
    return nullptr;
}

} // namespace cship

using namespace cship;

extern "C" int cstone_hip_pair_counts(cstone_hip_ctx* ctx, int real_bits, int w_bits, const void* x, const void* y,
                                      const void* z, const void* w, uint32_t first, uint32_t last, uint32_t t_first,
                                      uint32_t t_last, const cstone_box* box_host, const int32_t* child_offsets,
                                      const int32_t* internal_to_leaf, const uint32_t* layout, const void* centers,
                                      const void* sizes, const double* edges_host, int num_bins, uint64_t* counts,
                                      double* sums, uint64_t* stats_host)
{
    if (!ctx) return CSTONE_E_ARG;
    if (const char* why = pairCountsRefusal(real_bits, w_bits, w != nullptr, box_host, edges_host, num_bins))
        return fail(ctx, CSTONE_E_ARG, "pair_counts: %s", why);
    if (last < first || t_last < t_first || t_first < first || t_last > last)
        return fail(ctx, CSTONE_E_ARG, "pair_counts: [t_first, t_last) must be a range inside the range [first, last)");
    if (!counts || (w && !sums)) return fail(ctx, CSTONE_E_ARG, "pair_counts: null output");
    if (t_last == t_first) return pairZero(ctx, num_bins, counts, w ? sums : nullptr, stats_host);
    if (!x || !y || !z || !child_offsets || !internal_to_leaf || !layout || !centers || !sizes)
        return fail(ctx, CSTONE_E_ARG, "pair_counts: null pointer");

    const uint32_t numRows = pairNumRows(t_last - t_first, last - first);
    CS_TRY(arenaReserve(ctx, pairRowsBytes(numRows, num_bins)));
    const PairRows rows = takeRows(ctx, numRows, num_bins);
    if (!rows.stats)
    {
        arenaReset(ctx);
        return fail(ctx, CSTONE_E_INTERNAL, "pair_counts: workspace");
    }
    int rc = dispatchPairCounts<true>(ctx, real_bits, w_bits, x, y, z, w, first, last, x, y, z, w, t_first, t_last, *box_host,
                                      child_offsets, internal_to_leaf, layout, centers, sizes, edges_host, num_bins, numRows, rows,
                                      counts, sums);
    if (rc == CSTONE_OK && stats_host) rc = copyToHost(ctx, stats_host, rows.stats, 16);
    arenaReset(ctx); // later launches reuse the slices behind these in stream order
    return rc;
}

extern "C" int cstone_hip_pair_counts_cross(cstone_hip_ctx* ctx, int real_bits, int w_bits, const void* x, const void* y,
                                            const void* z, const void* w, uint32_t first, uint32_t last,
                                            const cstone_box* box_host, const int32_t* child_offsets,
                                            const int32_t* internal_to_leaf, const uint32_t* layout, const void* centers,
                                            const void* sizes, const void* query_centers, const void* query_w,
                                            uint32_t num_queries, const double* edges_host, int num_bins, uint64_t* counts,
                                            double* sums, uint64_t* stats_host)
{
    if (!ctx) return CSTONE_E_ARG;
    if (const char* why = pairCountsRefusal(real_bits, w_bits, w != nullptr || query_w != nullptr, box_host, edges_host, num_bins))
        return fail(ctx, CSTONE_E_ARG, "pair_counts_cross: %s", why);
    if (last < first) return fail(ctx, CSTONE_E_ARG, "pair_counts_cross: last < first");
    if (query_w && !w) return fail(ctx, CSTONE_E_ARG, "pair_counts_cross: query_w without w");
    if (!counts || (w && !sums)) return fail(ctx, CSTONE_E_ARG, "pair_counts_cross: null output");
    if (num_queries == 0 || last == first)
    {
        if (num_queries && !query_centers) return fail(ctx, CSTONE_E_ARG, "pair_counts_cross: null pointer");
        return pairZero(ctx, num_bins, counts, w ? sums : nullptr, stats_host);
    }
    if (!x || !y || !z || !child_offsets || !internal_to_leaf || !layout || !centers || !sizes || !query_centers)
        return fail(ctx, CSTONE_E_ARG, "pair_counts_cross: null pointer");

    // the queries in SFC order (64-bit Hilbert keys in the particles' box; a centre outside an open box takes the key
    // the encode's clamping gives it: the order only serves the coherence of a wave's 64 targets)
    const size_t nq = num_queries, rbytes = size_t(real_bits / 8), wbytes = size_t(w_bits / 8);
    const size_t tempBytes = cstone_hip_sort_pairs_temp_bytes(64, nq);
    const uint32_t numRows = pairNumRows(num_queries, last - first);
    CS_TRY(arenaReserve(ctx, 6 * alignUp(nq * rbytes) + 2 * alignUp(nq * 8) + 2 * alignUp(nq * 4) + alignUp(tempBytes) +
                                 alignUp(nq * 8) + pairRowsBytes(numRows, num_bins) + 4096));
    void *qx = arenaTake(ctx, nq * rbytes), *qy = arenaTake(ctx, nq * rbytes), *qz = arenaTake(ctx, nq * rbytes);
    void *sx = arenaTake(ctx, nq * rbytes), *sy = arenaTake(ctx, nq * rbytes), *sz = arenaTake(ctx, nq * rbytes);
    void *keys = arenaTake(ctx, nq * 8), *keysAlt = arenaTake(ctx, nq * 8);
    auto* order    = (uint32_t*)arenaTake(ctx, nq * 4);
    auto* orderAlt = (uint32_t*)arenaTake(ctx, nq * 4);
    void* temp     = arenaTake(ctx, tempBytes);
    void* sw       = query_w ? arenaTake(ctx, nq * wbytes) : nullptr;
    const PairRows rows = takeRows(ctx, numRows, num_bins);
    if (!rows.stats || (query_w && !sw))
    {
        arenaReset(ctx);
        return fail(ctx, CSTONE_E_INTERNAL, "pair_counts_cross: workspace");
    }

    auto run = [&]() -> int
    {
        const unsigned grid = gridFor(nq, 256);
        if (real_bits == 32)
            hipLaunchKernelGGL(pairSplitCentersKernel<float>, grid, 256, 0, ctx->stream, (const float*)query_centers, num_queries,
                               (float*)qx, (float*)qy, (float*)qz);
        else
            hipLaunchKernelGGL(pairSplitCentersKernel<double>, grid, 256, 0, ctx->stream, (const double*)query_centers,
                               num_queries, (double*)qx, (double*)qy, (double*)qz);
        CS_HIP(ctx, hipMemsetAsync(keys, 0, nq * 8, ctx->stream)); // (the encode honours remove markers in the key array)
        CS_TRY(cstone_hip_compute_sfc_keys(ctx, CSTONE_HILBERT, 64, real_bits, qx, qy, qz, keys, nq, box_host));
        CS_TRY(cstone_hip_sort_keys_ordering(ctx, 64, keys, order, nq, keysAlt, orderAlt, temp, tempBytes));
#define CSTONE_PAIR_GATHER(T, W)                                                                                       \
    hipLaunchKernelGGL((pairGatherQueriesKernel<T, W>), grid, 256, 0, ctx->stream, (const T*)query_centers, (const W*)query_w, \
                       order, num_queries, (T*)sx, (T*)sy, (T*)sz, (W*)sw)
        if (real_bits == 32)
        {
            if (w_bits == 64 && query_w) CSTONE_PAIR_GATHER(float, double);
            else
                CSTONE_PAIR_GATHER(float, float);
        }
        else
        {
            if (w_bits == 64 && query_w) CSTONE_PAIR_GATHER(double, double);
            else
                CSTONE_PAIR_GATHER(double, float);
        }
#undef CSTONE_PAIR_GATHER
        CS_TRY(dispatchPairCounts<false>(ctx, real_bits, w_bits, x, y, z, w, first, last, sx, sy, sz, sw, 0, num_queries, *box_host,
                                         child_offsets, internal_to_leaf, layout, centers, sizes, edges_host, num_bins, numRows,
                                         rows, counts, sums));
        return stats_host ? copyToHost(ctx, stats_host, rows.stats, 16) : CSTONE_OK;
    };
    const int rc = run();
    arenaReset(ctx);
    return rc;
}

extern "C" int cstone_hip_xi_natural(const uint64_t* counts, const double* edges_host, int num_bins, double n_targets,
                                     double n_partners, double volume, double* xi_host)
{
    if (!counts || !xi_host || !sphereEdgesOk(edges_host, num_bins)) return CSTONE_E_ARG;
    const double fourPi3 = 4.0 * 3.14159265358979323846 / 3.0;
    for (int b = 0; b < num_bins; ++b)
    {
        const double e0 = edges_host[b], e1 = edges_host[b + 1];
        const double shell    = fourPi3 * (e1 * e1 * e1 - e0 * e0 * e0);
        const double expected = n_targets * n_partners * shell / volume;
        xi_host[b] = (shell > 0.0 && expected > 0.0) ? double(counts[b]) / expected - 1.0 : std::nan("");
    }
    return CSTONE_OK;
}
