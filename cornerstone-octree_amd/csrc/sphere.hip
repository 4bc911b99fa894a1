// Sphere queries on the octree for gfx950: everything within a few radii of ARBITRARY points, binned by distance.  The rule
// is stated in include/cstone_hip.h, cstone_hip_sphere_profiles: the brute force over all (query, particle) pairs with
// the offset, the fold and d2 in the coordinate type, half-open bins on the squared edges, sums in double.  The tree only
// prunes.
//
// Shape: ONE WAVE PER QUERY, one wave per workgroup.  A sphere about a group's centre holds 10^3 .. 10^6 particles, so the
// one-lane-per-target shape of the neighbour walk (cstone_hip_device.hpp) is the wrong one: here the centre and the edges
// are wave-uniform and the lanes share the work of one query.
//   node tests   64 at a time, as findHalosKernel does: up to 8 nodes leave the stack, lane l tests child l & 7 of node
//                l >> 3, a ballot says which children are leaves and which go back on the stack.  No lane mask travels
//                with a node -- there is one query per wave.
//   leaves       every lane of an opened leaf child loads its own layout range; ranges that touch (the children of one
//                node are consecutive in SFC order) are merged, clipped to [first, last) and read 64 particles at a time:
//                lane l loads x, y, z, w of particle base + l (coalesced), folds, squares, finds its bin by a binary search
//                over e2 in LDS (7 steps) and adds to ITS OWN accumulator acc[b][l], cnt[b][l] in LDS.  acc[b][l] lies
//                b * 512 + l * 8 bytes into the array: whatever b each lane picks, the lanes of an 8-byte access group hit
//                distinct banks.  No atomics of any kind.
//   end          the 64 lanes of every bin are added by a butterfly (lane ^ 32, 16, ... 1: a fixed tree, and a + b is
//                commutative, so every lane holds the same bits); lane b keeps bin b and the row is written coalesced.
// The order of every sum is fixed by the tree, the range and this shape; the launch shape is no argument of the call.
//
// The walk, its stack and the stack's bound are those of wave_walk.hpp.
//
// LDS per wave: 768 * NB (accumulators) + 66 reals (e2) + 5 376 (stack): 6.7 KiB at NB = 1, 55 KiB at NB = 64.
#include <cmath>
#include <cstring>

#include "cstone_hip_device.hpp"
#include "ctx.hpp"
#include "node_margin.hpp"
#include "sphere.hpp"
#include "wave_walk.hpp"

namespace cship
{

namespace
{

constexpr int SPHERE_E2_PAD = CSTONE_SPHERE_MAX_BINS + 2; // e2[0 .. NB], padded to an even count: the stack stays 8-aligned

struct SphereEdgesD
{
    double e[CSTONE_SPHERE_MAX_BINS + 1];
};

template<class T>
constexpr size_t sphereLdsBytes(int nb)
{
    return size_t(nb) * 64 * (sizeof(double) + sizeof(uint32_t)) + SPHERE_E2_PAD * sizeof(T) + WALK_STACK * sizeof(int32_t);
}

/*! The margin of the node test, and why its absolute term is nodeAbsMargin(box, 64).  A node may be skipped only if NO
 *  particle in it passes the particle test, d2 < e2_NB.  Per axis a, with u = eps / 2 the unit roundoff of T and L the largest of |lo_a|, |hi_a| and len_a over the axes:
 *
 *    In exact arithmetic the folded offset has the magnitude g(d) = distance of d to the nearest multiple of len, and g
 *    is 1-Lipschitz, so for a particle p inside the node's box  g(p - c_q) >= g(c_node - c_q) - size  -- whichever images
 *    the two folds pick.  What the kernel computes differs from that by ABSOLUTE errors, not relative ones:
 *      - d = fl(r - c_q) is off by u |d| <= 2 u L; d * inv carries 3 relative roundings (inv, the product), so rint may
 *        pick the neighbouring image only when d is within 6 u L of half a box length, where both images have magnitudes
 *        within 12 u L of each other; len * k is exact for the k that occur, the subtraction adds u L.  Together
 *        < 16 u L for the particle's offset and as much for the node's: 32 u L.
 *      - the particle is "in" the node by its SFC key, i.e. by fl((r - lo) * inv) scaled to the grid, while the node's
 *        centre and half size are themselves rounded from the grid: a particle can lie outside [c - size, c + size] by
 *        the roundings of the normalisation (3 u len) and of centre and size (a few u L each): < 12 u L.
 *      - |d_node| - size is one more rounding: u L.
 *    So  max(|d_node| - size, 0) <= |d_particle| + 45 u L  per axis as computed; the kernel allows 64 u L = 32 eps L.
 *    Over three axes the node's distance exceeds the particle's sqrt(d2) by at most sqrt(3) * 32 eps L < 64 eps L, and the
 *    squares, sums and the comparison with e2_NB = fl(e_NB * e_NB) add a few RELATIVE roundings on both sides, covered by
 *    the factor 1 + 16 eps.  Hence:  skip iff  dist2_node > (e_NB * (1 + 16 eps) + 64 eps L)^2.
 *
 *  The relative term alone covers nothing when e_NB is a few ulps of the coordinates: the cancellation in
 *  |c_node - c_q| - size is absolute.  tests/test_sphere_profiles.py (cell faces) has queries that a relative-only margin
 *  loses in f32.  The bound takes |c_q - r| <= 2 len on a periodic axis (centres in or near the box). */
template<class T, class W, bool HAS_W>
__global__ __launch_bounds__(64) void sphereProfilesKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                           const T* __restrict__ z, const W* __restrict__ w, uint32_t first,
                                                           uint32_t last, cstone_hip::DeviceBox<T> box,
                                                           cstone_hip::OctreeNsView<T> tree, const T* __restrict__ qc,
                                                           const T* __restrict__ qs, WalkEdges<T> edges, int nb,
                                                           T absMargin, unsigned long long* __restrict__ counts,
                                                           double* __restrict__ sums, uint32_t* __restrict__ flags,
                                                           int* __restrict__ errors)
{
    extern __shared__ double sphereLds[];
    double* acc    = sphereLds;                                   // [nb][64]
    uint32_t* cnt  = reinterpret_cast<uint32_t*>(acc + nb * 64);  // [nb][64]
    T* e2          = reinterpret_cast<T*>(cnt + nb * 64);         // [nb + 1]
    int32_t* stack = reinterpret_cast<int32_t*>(e2 + SPHERE_E2_PAD);

    const unsigned lane = threadIdx.x;
    const size_t q      = blockIdx.x;
    const T s           = qs ? qs[q] : T(1);
    const T cx = qc[3 * q], cy = qc[3 * q + 1], cz = qc[3 * q + 2];
    const bool px = box.bc[0] == 1, py = box.bc[1] == 1, pz = box.bc[2] == 1;

    for (int b = int(lane); b <= nb; b += 64)
    {
        const T e = s * edges.e[b];
        e2[b]     = e * e;
    }
    for (int b = 0; b < nb; ++b)
    {
        acc[b * 64 + lane] = 0.0;
        cnt[b * 64 + lane] = 0u;
    }
    const T eN      = s * edges.e[nb];
    const bool wide = (px && eN >= T(0.5) * box.len[0]) || (py && eN >= T(0.5) * box.len[1]) || (pz && eN >= T(0.5) * box.len[2]);
    // a scale of 0, a negative one or a NaN: no edge is above 0 and the row stays empty (the rule says so: the squares
    // of negative edges would ascend again)
    const bool live = !wide && eN > T(0) && last > first;
    __syncthreads();

    // the node test (its margin: above the kernel).  !(>): a NaN anywhere opens the node, the particle test then decides
    const T eps  = sizeof(T) == 4 ? T(1.1920928955078125e-07) : T(2.220446049250313e-16);
    const T thr  = eN * (T(1) + T(16) * eps) + absMargin;
    const T thr2 = thr * thr;
    auto near = [&](int32_t n) -> bool { return !(walkNodeDist2(tree, box, n, cx, cy, cz) > thr2); };
    // particles [jb, je) (wave-uniform), clipped to the range: the particle test, the authority
    auto bin = [&](uint32_t jb, uint32_t je)
    {
        jb = max(jb, first), je = min(je, last);
        for (uint32_t base = jb; base < je; base += 64)
        {
            const uint32_t j = base + lane;
            if (j < je)
            {
                T dx = x[j] - cx, dy = y[j] - cy, dz = z[j] - cz;
                dx = cstone_hip::detail::foldAxis<T>(dx, box.len[0], box.inv[0], px);
                dy = cstone_hip::detail::foldAxis<T>(dy, box.len[1], box.inv[1], py);
                dz = cstone_hip::detail::foldAxis<T>(dz, box.len[2], box.inv[2], pz);
                const T d2 = dx * dx + dy * dy + dz * dz;
                // number of edges with e2 <= d2 (e2 does not descend): bin = that number - 1
                int at = 0;
#pragma unroll
                for (int step = 64; step; step >>= 1)
                {
                    const int t = at + step;
                    if (t <= nb + 1 && e2[min(t - 1, nb)] <= d2) at = t;
                }
                if (at >= 1 && at <= nb)
                {
                    const int slot = (at - 1) * 64 + int(lane);
                    cnt[slot] += 1u;
                    if (HAS_W) acc[slot] += double(w[j]);
                }
            }
        }
    };

    if (live) walkFromRoot(tree, stack, lane, errors, near, bin);
    __syncthreads();

    unsigned long long myCount;
    double mySum;
    walkBinTotals<HAS_W>(cnt, acc, nb, lane, myCount, mySum);
    if (int(lane) < nb)
    {
        counts[q * nb + lane] = myCount;
        if (HAS_W) sums[q * nb + lane] = mySum;
    }
    if (lane == 0 && flags) flags[q] = wide ? CSTONE_SPHERE_TOO_WIDE : 0u;
}

//! the finish of include/cstone_hip.h, cstone_hip_spherical_overdensity: one lane per query, everything in double
template<class T>
__global__ __launch_bounds__(256) void sphericalOverdensityKernel(const T* __restrict__ qs, uint32_t numQueries, SphereEdgesD edges,
                                                                  int nb, const double* __restrict__ sums,
                                                                  const uint32_t* __restrict__ profileFlags, double rho,
                                                                  double* __restrict__ rDelta, double* __restrict__ mDelta,
                                                                  uint32_t* __restrict__ flags)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= numQueries) return;
    uint32_t flag = 0;
    double R = 0.0, M = 0.0;
    if (profileFlags && (profileFlags[q] & CSTONE_SPHERE_TOO_WIDE)) { flag = CSTONE_SPHERE_TOO_WIDE; }
    else
    {
        const double s        = double(qs ? qs[q] : T(1));
        const double fourPi3  = 4.0 * 3.14159265358979323846 / 3.0;
        const double* row     = sums + size_t(q) * nb;
        double Cprev = 0.0, Eprev = s * edges.e[0], fprev = 0.0;
        int bStar = 0;
        double C = 0.0, E = Eprev, f = 0.0;
        for (int b = 1; b <= nb; ++b)
        {
            C = Cprev + row[b - 1];
            E = s * edges.e[b];
            f = C - rho * (fourPi3 * (E * E * E));
            if (f < 0.0)
            {
                bStar = b;
                break;
            }
            Cprev = C, Eprev = E, fprev = f;
        }
        if (bStar == 0) { flag = CSTONE_SO_NOT_REACHED, R = E, M = C; }
        else if (bStar == 1) { flag = CSTONE_SO_UNRESOLVED; }
        else
        {
            const double t = fprev / (fprev - f);
            R              = Eprev + t * (E - Eprev);
            M              = Cprev + t * (C - Cprev);
        }
    }
    rDelta[q] = R;
    mDelta[q] = M;
    if (flags) flags[q] = flag;
}

__global__ __launch_bounds__(256) void spherePackKernel(const unsigned long long* __restrict__ counts,
                                                        const double* __restrict__ sums, size_t n, double* __restrict__ buf)
{
    const size_t k = size_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= n) return;
    buf[k] = double(counts[k]);
    if (sums) buf[n + k] = sums[k];
}

__global__ __launch_bounds__(256) void sphereUnpackKernel(const double* __restrict__ buf, size_t n,
                                                          unsigned long long* __restrict__ counts, double* __restrict__ sums)
{
    const size_t k = size_t(blockIdx.x) * 256u + threadIdx.x;
    if (k >= n) return;
    counts[k] = (unsigned long long)(buf[k]);
    if (sums) sums[k] = buf[n + k];
}

template<class T, class W, bool HAS_W>
int launchProfiles(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* w, uint32_t first,
                   uint32_t last, const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf,
                   const uint32_t* layout, const void* centers, const void* sizes, const void* qc, const void* qs,
                   uint32_t numQueries, const double* edgesHost, int nb, uint64_t* counts, double* sums, uint32_t* flags)
{
    cstone_hip::OctreeNsView<T> tree{childOffsets, internalToLeaf, layout, (const T*)centers, (const T*)sizes};
    WalkEdges<T> edges;
    std::memset(&edges, 0, sizeof edges);
    for (int b = 0; b <= nb; ++b)
        edges.e[b] = T(edgesHost[b]);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t));
    hipLaunchKernelGGL((sphereProfilesKernel<T, W, HAS_W>), numQueries, 64, sphereLdsBytes<T>(nb), ctx->stream, (const T*)x,
                       (const T*)y, (const T*)z, (const W*)w, first, last, cstone_hip::makeDeviceBox<T>(box), tree,
                       (const T*)qc, (const T*)qs, edges, nb, nodeAbsMargin<T>(box, 64),
                       reinterpret_cast<unsigned long long*>(counts), sums, flags, ctx->devScalars + 63);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(ctx, CSTONE_E_HIP, "sphere_profiles: %s", hipGetErrorString(e));
    return CSTONE_OK;
}

} // namespace

bool sphereEdgesOk(const double* edges, int numBins)
{
    if (!edges || numBins < 1 || numBins > CSTONE_SPHERE_MAX_BINS) return false;
    if (!std::isfinite(edges[0]) || edges[0] < 0.0) return false;
    for (int b = 1; b <= numBins; ++b)
        if (!std::isfinite(edges[b]) || !(edges[b] > edges[b - 1])) return false;
    return true;
}

void spherePackRows(cstone_hip_ctx* ctx, const uint64_t* counts, const double* sums, size_t n, double* buf)
{
    if (n)
        hipLaunchKernelGGL(spherePackKernel, gridFor(n, 256), 256, 0, ctx->stream,
                           reinterpret_cast<const unsigned long long*>(counts), sums, n, buf);
}

void sphereUnpackRows(cstone_hip_ctx* ctx, const double* buf, size_t n, uint64_t* counts, double* sums)
{
    if (n)
        hipLaunchKernelGGL(sphereUnpackKernel, gridFor(n, 256), 256, 0, ctx->stream, buf, n,
                           reinterpret_cast<unsigned long long*>(counts), sums);
}

} // namespace cship

using namespace cship;

extern "C" int cstone_hip_sphere_profiles(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                          const void* z, const void* w, uint32_t first, uint32_t last,
                                          const cstone_box* box_host, const int32_t* child_offsets,
                                          const int32_t* internal_to_leaf, const uint32_t* layout, const void* centers,
                                          const void* sizes, const void* query_centers, const void* query_scale,
                                          uint32_t num_queries, const double* edges_host, int num_bins, uint64_t* counts,
                                          double* sums, uint32_t* flags)
{
    if (!ctx) return CSTONE_E_ARG;
    if (real_bits != 32 && real_bits != 64) return fail(ctx, CSTONE_E_ARG, "sphere_profiles: real_bits %d unsupported", real_bits);
    if (w && mass_bits != 32 && mass_bits != 64)
        return fail(ctx, CSTONE_E_ARG, "sphere_profiles: mass_bits %d unsupported", mass_bits);
    if (last < first) return fail(ctx, CSTONE_E_ARG, "sphere_profiles: last < first");
    if (!sphereEdgesOk(edges_host, num_bins))
        return fail(ctx, CSTONE_E_ARG, "sphere_profiles: 1 .. %d bins with finite, non-negative, strictly ascending edges are taken",
                    CSTONE_SPHERE_MAX_BINS);
    if (num_queries == 0) return CSTONE_OK;
    if (!x || !y || !z || !box_host || !child_offsets || !internal_to_leaf || !layout || !centers || !sizes ||
        !query_centers || !counts || (w && !sums))
        return fail(ctx, CSTONE_E_ARG, "sphere_profiles: null pointer");

#define CSTONE_SPHERE_LAUNCH(T, W, HAS_W)                                                                              \
    launchProfiles<T, W, HAS_W>(ctx, x, y, z, w, first, last, *box_host, child_offsets, internal_to_leaf, layout, centers, \
                                sizes, query_centers, query_scale, num_queries, edges_host, num_bins, counts, sums, flags)
    if (real_bits == 32)
    {
        if (!w) return CSTONE_SPHERE_LAUNCH(float, float, false);
        return mass_bits == 32 ? CSTONE_SPHERE_LAUNCH(float, float, true) : CSTONE_SPHERE_LAUNCH(float, double, true);
    }
    if (!w) return CSTONE_SPHERE_LAUNCH(double, float, false);
    return mass_bits == 32 ? CSTONE_SPHERE_LAUNCH(double, float, true) : CSTONE_SPHERE_LAUNCH(double, double, true);
#undef CSTONE_SPHERE_LAUNCH
}

extern "C" int cstone_hip_spherical_overdensity(cstone_hip_ctx* ctx, int real_bits, const void* query_scale,
                                                uint32_t num_queries, const double* edges_host, int num_bins,
                                                const double* sums, const uint32_t* profile_flags, double rho_threshold,
                                                double* r_delta, double* m_delta, uint32_t* flags)
{
    if (!ctx) return CSTONE_E_ARG;
    if (real_bits != 32 && real_bits != 64)
        return fail(ctx, CSTONE_E_ARG, "spherical_overdensity: real_bits %d unsupported", real_bits);
    if (!sphereEdgesOk(edges_host, num_bins) || edges_host[0] != 0.0)
        return fail(ctx, CSTONE_E_ARG, "spherical_overdensity: 1 .. %d bins with finite, strictly ascending edges from 0 are taken",
                    CSTONE_SPHERE_MAX_BINS);
    if (!(rho_threshold > 0.0)) // (a NaN fails the comparison)
        return fail(ctx, CSTONE_E_ARG, "spherical_overdensity: threshold %g is not > 0", rho_threshold);
    if (num_queries == 0) return CSTONE_OK;
    if (!sums || !r_delta || !m_delta) return fail(ctx, CSTONE_E_ARG, "spherical_overdensity: null pointer");
    SphereEdgesD edges;
    std::memset(&edges, 0, sizeof edges);
    for (int b = 0; b <= num_bins; ++b)
        edges.e[b] = edges_host[b];
    const unsigned grid = gridFor(num_queries, 256);
    if (real_bits == 32)
        hipLaunchKernelGGL(sphericalOverdensityKernel<float>, grid, 256, 0, ctx->stream, (const float*)query_scale, num_queries,
                           edges, num_bins, sums, profile_flags, rho_threshold, r_delta, m_delta, flags);
    else
        hipLaunchKernelGGL(sphericalOverdensityKernel<double>, grid, 256, 0, ctx->stream, (const double*)query_scale,
                           num_queries, edges, num_bins, sums, profile_flags, rho_threshold, r_delta, m_delta, flags);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(ctx, CSTONE_E_HIP, "spherical_overdensity: %s", hipGetErrorString(e));
    return CSTONE_OK;
}
