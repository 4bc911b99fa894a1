// Adaptive smoothing lengths on gfx950: every target's h is iterated to a target neighbour count INSIDE one kernel.
// The loop an SPH client runs after Domain::sync -- count neighbours, correct h, count again -- costs one full walk of all
// particles per pass as a host loop; here a lane that is done drops out of its wave's walk and a wave that is done
// stops.  The rule belongs to this library (the reference has none) and is stated in include/cstone_hip.h,
// cstone_hip_adapt_smoothing_lengths: T arithmetic with + - * / and comparisons only, compiled with -ffp-contract=off
// like neighbors.hip, so a numpy restatement in the same dtype reproduces h, counts and status bit for bit.
//
// Layout: that of findNeighborsKernel (csrc/neighbors.hip) -- one wave per 64 consecutive targets, four waves per block,
// the LDS stack of cstone_hip_device.hpp, the walk of cstone_hip::traverseNeighborsH with the lane's h as a value.  Every
// lane keeps h, lo, hi, hcap, its count and its flags in registers; the wave repeats the walk while any lane is active;
// lanes that have stopped pass valid = false, so they are in no node mask and test no particle.  The loop exit is
// wave-uniform (__any).  h is updated in place: a target's walk reads only its own h (from a register), and only that
// target's lane writes it, once, after its last walk; x, y, z are read-only.  No atomics except the sticky error word.
#include <cmath>

#include "cstone_hip_device.hpp"
#include "ctx.hpp"
#include "device_keys.hpp"

namespace cship
{

namespace
{

constexpr int AH_BLOCK = 256;
constexpr int AH_WAVES = AH_BLOCK / 64;

/*! LISTS: after the iteration, one more walk of the whole wave at the final h stores the first ngmax neighbours of every
 *  target.  A walk cannot know that it is a target's last one before it has counted, and a list stored during an earlier
 *  walk with a larger count would leave entries beyond the final count, so the lists get a pass of their own. */
template<class T, bool LISTS>
__global__ __launch_bounds__(AH_BLOCK) void adaptSmoothingLengthsKernel(
    const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z, T* h, uint32_t first, uint32_t last,
    cstone_hip::DeviceBox<T> box, cstone_hip::OctreeNsView<T> tree, uint32_t ng0, uint32_t tol, uint32_t maxIter,
    float growLimit, uint32_t ngmax, uint32_t* __restrict__ neighbors, uint32_t* __restrict__ counts,
    uint32_t* __restrict__ status, int* __restrict__ errors)
{
    __shared__ cstone_hip::TraversalStack stacks[AH_WAVES];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    const uint32_t chunk = first + (blockIdx.x * AH_WAVES + wave) * 64u;
    if (chunk >= last) return;
    const bool valid   = chunk + lane < last;
    const uint32_t i   = valid ? chunk + lane : last - 1;
    const uint32_t tid = i - first;

    const T inf = T(INFINITY);
    T hc = h[i], lo = T(0), hi = inf;
    const T hcap = hc * T(growLimit);
    uint32_t nn = 0, walks = 0, flags = 0;
    bool active = valid;
    auto count  = [](uint32_t, T, T, T, T) {};

    // it is the same for every active lane: all lanes start at 0 and every turn of the loop is one walk of the wave
    for (uint32_t it = 0; __any(active); ++it)
    {
        const uint32_t found = cstone_hip::traverseNeighborsH(active, i, x, y, z, hc, tree, box, 1.0f, stacks[wave], errors, count);
        if (active)
        {
            nn = found;
            ++walks;
            const unsigned long long n64 = nn, g64 = ng0, t64 = tol;
            if (n64 + t64 >= g64 && n64 <= g64 + t64) { active = false; }
            else if (it == maxIter)
            {
                flags |= CSTONE_ADAPT_H_NOT_CONVERGED;
                active = false;
            }
            else
            {
                if (n64 + t64 < g64)
                {
                    lo = hc;
                    if (hc >= hcap)
                    {
                        flags |= CSTONE_ADAPT_H_CAPPED;
                        active = false;
                    }
                }
                else { hi = hc; }
                if (active)
                {
                    T q = T(ng0) / T(nn > 1u ? nn : 1u);
                    q   = q < T(0.125) ? T(0.125) : q;
                    q   = q > T(8) ? T(8) : q;
                    T t = (T(2) + q) / T(3); // two Newton steps towards cbrt(q) from 1
                    t   = (T(2) * t + q / (t * t)) / T(3);
                    T hp = hc * t;
                    hp   = hcap < hp ? hcap : hp;
                    if (hi < inf && !(lo < hp && hp < hi)) hp = T(0.5) * (lo + hi);
                    if (hp == hc)
                    {
                        flags |= CSTONE_ADAPT_H_STALLED;
                        active = false;
                    }
                    else { hc = hp; }
                }
            }
        }
    }

    if constexpr (LISTS)
    {
        uint32_t* out   = neighbors + size_t(tid) * ngmax;
        uint32_t stored = 0;
        auto keep       = [&](uint32_t j, T, T, T, T)
        {
            if (stored < ngmax) out[stored] = j;
            ++stored;
        };
        (void)cstone_hip::traverseNeighborsH(valid, i, x, y, z, hc, tree, box, 1.0f, stacks[wave], errors, keep);
    }
    if (valid)
    {
        h[i]        = hc;
        counts[tid] = nn;
        status[tid] = (walks < 255u ? walks : 255u) | flags;
    }
}

template<class T>
void launchAdapt(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, void* h, uint32_t first, uint32_t last,
                 const cstone_box& box, const int32_t* childOffsets, const int32_t* internalToLeaf,
                 const uint32_t* layout, const void* centers, const void* sizes, uint32_t ng0, uint32_t tol,
                 uint32_t maxIter, float growLimit, uint32_t ngmax, uint32_t* neighbors, uint32_t* counts,
                 uint32_t* status)
{
    cstone_hip::OctreeNsView<T> tree{childOffsets, internalToLeaf, layout, (const T*)centers, (const T*)sizes};
    const unsigned grid = gridFor(size_t(last - first), AH_BLOCK);
    int* errors         = ctx->devScalars + 63;
    if (ngmax)
        hipLaunchKernelGGL((adaptSmoothingLengthsKernel<T, true>), grid, AH_BLOCK, 0, ctx->stream, (const T*)x,
                           (const T*)y, (const T*)z, (T*)h, first, last, cstone_hip::makeDeviceBox<T>(box), tree, ng0, tol,
                           maxIter, growLimit, ngmax, neighbors, counts, status, errors);
    else
        hipLaunchKernelGGL((adaptSmoothingLengthsKernel<T, false>), grid, AH_BLOCK, 0, ctx->stream, (const T*)x,
                           (const T*)y, (const T*)z, (T*)h, first, last, cstone_hip::makeDeviceBox<T>(box), tree, ng0, tol,
                           maxIter, growLimit, ngmax, neighbors, counts, status, errors);
}

} // namespace

} // namespace cship

using namespace cship;

extern "C" int cstone_hip_adapt_smoothing_lengths(cstone_hip_ctx* ctx, int real_bits, const void* x, const void* y,
                                                  const void* z, void* h, uint32_t first, uint32_t last,
                                                  const cstone_box* box_host, const int32_t* child_offsets,
                                                  const int32_t* internal_to_leaf, const uint32_t* layout,
                                                  const void* centers, const void* sizes, uint32_t ng0, uint32_t tol,
                                                  uint32_t max_iter, float grow_limit, uint32_t ngmax,
                                                  uint32_t* neighbors, uint32_t* counts, uint32_t* status)
{
    if (!ctx || !x || !y || !z || !h || !box_host || !child_offsets || !internal_to_leaf || !layout || !centers ||
        !sizes || !counts || !status || (ngmax && !neighbors) || last < first)
        return fail(ctx, CSTONE_E_ARG, "adapt_smoothing_lengths: bad argument");
    if (real_bits != 32 && real_bits != 64)
        return fail(ctx, CSTONE_E_ARG, "adapt_smoothing_lengths: real_bits %d unsupported", real_bits);
    if (ng0 == 0) return fail(ctx, CSTONE_E_ARG, "adapt_smoothing_lengths: ng0 must be at least 1");
    if (!(grow_limit >= 1.0f)) // (a NaN fails the comparison)
        return fail(ctx, CSTONE_E_ARG, "adapt_smoothing_lengths: grow_limit %g is not >= 1", double(grow_limit));
    if (last == first) return CSTONE_OK;
    {
        StageTimer timer(ctx, CSTONE_STAGE_ADAPT_H);
        if (real_bits == 32)
            launchAdapt<float>(ctx, x, y, z, h, first, last, *box_host, child_offsets, internal_to_leaf, layout, centers,
                               sizes, ng0, tol, max_iter, grow_limit, ngmax, neighbors, counts, status);
        else
            launchAdapt<double>(ctx, x, y, z, h, first, last, *box_host, child_offsets, internal_to_leaf, layout, centers,
                                sizes, ng0, tol, max_iter, grow_limit, ngmax, neighbors, counts, status);
    }
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}
