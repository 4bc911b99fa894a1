// Barnes-Hut gravity on a linked octree that carries expansion centres (cstone_hip_domain_sync_grav /
// _update_expansion_centers, or any tree with centres and MAC radii in the same T[M][4] layout): the multipole upsweep
// and the group walk behind cstone_hip_upsweep_multipoles / cstone_hip_compute_gravity.  The reference leaves this step
// to its client (Ryoanji); the MAC is its evaluateMac (R/traversal/macs.hpp, the function above evaluateMacPbc).
//
// Multipoles: T[8] per node = (M, Qxx, Qxy, Qxz, Qyy, Qyz, Qzz, 0), traceless Cartesian quadrupole about the node's
// expansion centre.  Leaves from their particles (one thread per leaf), internal nodes one level at a time from the
// sum of their 8 children shifted to the parent's centre (parallel-axis term; the dipole about a centre of mass is 0).
//
// Walk: ONE wave per target group (up to 64 consecutive particles, one target per lane; longer groups are walked 64 at
// a time).  The MAC is taken against the box of the wave's targets, so every decision is wave-uniform: the node
// stack lives in LDS, node data (centre, MAC radius, multipole) comes through scalar loads, and a node is either
// applied as a multipole to all 64 lanes (M2P) or, for an opened leaf, its particles are fetched with one coalesced
// load per array and handed round with v_readlane (P2P), the inner loop touching no memory.
// Compiled with -ffp-contract=off like the rest of the library: the MAC arithmetic is the one the tests restate.
//
// On a locally essential tree (cstone_hip_compute_gravity_let, the LET flag of the walk) one more rule applies: a node
// that fails the MAC, has no children and has an EMPTY particle range is applied as a multipole.  Such a leaf belongs to
// another rank and is no halo: syncGrav left it without particles because every focus CELL of this rank passes the
// vector MAC against it (markMacs), and every real target lies in a focus cell, so its multipole is within the MAC's
// error bound for each target.  The walk only asks to open it because it tests the MAC against the bounding box of 64
// consecutive targets, and on a non-convex piece of the space-filling curve that box reaches outside the focus.
// Without the rule the leaf's mass would vanish from the sum.  node, child and the range are wave-uniform already, so
// the rule costs a scalar branch and no lane mask.
//
// Per-particle softening (the SOFT flag of the walk and of the direct sum, cstone_hip_compute_gravity_h): with
// H = h_i + h_j a pair closer than H (r2 = |d|^2 + eps2 < H^2) interacts like a point with a homogeneous sphere of radius
// H, force linear in d and phi = -G m (3 H^2 - r2) / (2 H^3), both continuous at r2 = H^2.  One sqrt and one division per
// pair as before; h == 0 everywhere gives the Plummer rule's bits.  M2P keeps eps2 only.
//
// Octupoles (order 3): a second T[8] per node = (Oxxx, Oxxy, Oxxz, Oxyy, Oxyz, Oyyy, Oyyz, 0), the seven independent
// components of the traceless symmetric rank-3 tensor O_abc = sum m (15 d_a d_b d_c - 3 |d|^2 (d_a delta_bc + d_b delta_ac
// + d_c delta_ab)) about the same centre; Oxzz, Oyzz, Ozzz follow from the trace and are never formed.  The upsweep of a
// level shifts the children's octupoles with their FINAL multipoles (M and Q enter the shift), so it runs after the
// multipole upsweep.  The walk takes the order as a template parameter; order 3 adds one contraction per M2P and changes
// no decision, so the counts are those of the other orders.
//
// Direct sum (cstone_hip_direct_gravity): one wave per 64 targets, the sources streamed through the same P2P tile, cut
// into segments over gridDim.y whose partial sums a second kernel adds in segment order (no atomics).
#include <algorithm>

#include "ctx.hpp"
#include "device_keys.hpp"

namespace cship
{

namespace
{

constexpr int GW_BLOCK = 256;
constexpr int GW_WAVES = GW_BLOCK / 64;
constexpr int GW_STACK = 160; // >= 7 * 21 + 1: the deepest a depth-first walk of an octree of 21 levels gets

__device__ __forceinline__ int32_t uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ float readLane(float v, int k)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ double readLane(double v, int k)
{
    long long b = __double_as_longlong(v);
    int lo      = __builtin_amdgcn_readlane(int(b), k);
    int hi      = __builtin_amdgcn_readlane(int(b >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

template<class T>
__device__ __forceinline__ T waveMin(T v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = min(v, __shfl_xor(v, o));
    return v;
}
template<class T>
__device__ __forceinline__ T waveMax(T v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, __shfl_xor(v, o));
    return v;
}

//! multipole of every leaf from its particles layout[leaf] .. layout[leaf + 1], stored at its node index
template<class T, class Tm>
__global__ __launch_bounds__(256) void leafMultipolesKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                            const T* __restrict__ z, const Tm* __restrict__ m,
                                                            const NodeIdx* __restrict__ leafToInternal, NodeIdx numLeaves,
                                                            const uint32_t* __restrict__ layout,
                                                            const T* __restrict__ centers, T* __restrict__ mp)
{
    const NodeIdx leaf = blockIdx.x * 256 + threadIdx.x;
    if (leaf >= numLeaves) return;
    const NodeIdx n = leafToInternal[leaf];
    const T cx = centers[4 * size_t(n)], cy = centers[4 * size_t(n) + 1], cz = centers[4 * size_t(n) + 2];
    T M = 0, qxx = 0, qxy = 0, qxz = 0, qyy = 0, qyz = 0, qzz = 0;
    for (uint32_t i = layout[leaf]; i < layout[leaf + 1]; ++i)
    {
        const T w  = T(m[i]);
        const T dx = x[i] - cx, dy = y[i] - cy, dz = z[i] - cz;
        const T r2 = dx * dx + dy * dy + dz * dz;
        M += w;
        qxx += w * (T(3) * dx * dx - r2);
        qxy += w * (T(3) * dx * dy);
        qxz += w * (T(3) * dx * dz);
        qyy += w * (T(3) * dy * dy - r2);
        qyz += w * (T(3) * dy * dz);
        qzz += w * (T(3) * dz * dz - r2);
    }
    T* out = mp + 8 * size_t(n);
    out[0] = M, out[1] = qxx, out[2] = qxy, out[3] = qxz, out[4] = qyy, out[5] = qyz, out[6] = qzz, out[7] = T(0);
}

//! one level of the upsweep: internal nodes [firstCell, lastCell) from their 8 children, shifted to the node's centre
template<class T>
__global__ __launch_bounds__(256) void upsweepMultipolesKernel(NodeIdx firstCell, NodeIdx lastCell,
                                                               const NodeIdx* __restrict__ childOffsets,
                                                               const T* __restrict__ centers, T* __restrict__ mp)
{
    const NodeIdx cell = firstCell + blockIdx.x * 256 + threadIdx.x;
    if (cell >= lastCell) return;
    const NodeIdx child = childOffsets[cell];
    if (!child) return;
    const T cx = centers[4 * size_t(cell)], cy = centers[4 * size_t(cell) + 1], cz = centers[4 * size_t(cell) + 2];
    T M = 0, qxx = 0, qxy = 0, qxz = 0, qyy = 0, qyz = 0, qzz = 0;
    for (int k = 0; k < 8; ++k)
    {
        const size_t c = size_t(child + k);
        const T* q     = mp + 8 * c;
        const T mc     = q[0];
        const T sx = centers[4 * c] - cx, sy = centers[4 * c + 1] - cy, sz = centers[4 * c + 2] - cz;
        const T s2 = sx * sx + sy * sy + sz * sz;
        M += mc;
        qxx += q[1] + mc * (T(3) * sx * sx - s2);
        qxy += q[2] + mc * (T(3) * sx * sy);
        qxz += q[3] + mc * (T(3) * sx * sz);
        qyy += q[4] + mc * (T(3) * sy * sy - s2);
        qyz += q[5] + mc * (T(3) * sy * sz);
        qzz += q[6] + mc * (T(3) * sz * sz - s2);
    }
    T* out = mp + 8 * size_t(cell);
    out[0] = M, out[1] = qxx, out[2] = qxy, out[3] = qxz, out[4] = qyy, out[5] = qyz, out[6] = qzz, out[7] = T(0);
}

//! octupole of every leaf from its particles, stored at its node index (layout as leafMultipolesKernel)
template<class T, class Tm>
__global__ __launch_bounds__(256) void leafOctupolesKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                           const T* __restrict__ z, const Tm* __restrict__ m,
                                                           const NodeIdx* __restrict__ leafToInternal, NodeIdx numLeaves,
                                                           const uint32_t* __restrict__ layout,
                                                           const T* __restrict__ centers, T* __restrict__ oc)
{
    const NodeIdx leaf = blockIdx.x * 256 + threadIdx.x;
    if (leaf >= numLeaves) return;
    const NodeIdx n = leafToInternal[leaf];
    const T cx = centers[4 * size_t(n)], cy = centers[4 * size_t(n) + 1], cz = centers[4 * size_t(n) + 2];
    T oxxx = 0, oxxy = 0, oxxz = 0, oxyy = 0, oxyz = 0, oyyy = 0, oyyz = 0;
    for (uint32_t i = layout[leaf]; i < layout[leaf + 1]; ++i)
    {
        const T w  = T(m[i]);
        const T dx = x[i] - cx, dy = y[i] - cy, dz = z[i] - cz;
        const T r2 = dx * dx + dy * dy + dz * dz;
        const T tx = T(3) * r2 * dx, ty = T(3) * r2 * dy, tz = T(3) * r2 * dz;
        oxxx += w * (T(15) * dx * dx * dx - T(3) * tx);
        oxxy += w * (T(15) * dx * dx * dy - ty);
        oxxz += w * (T(15) * dx * dx * dz - tz);
        oxyy += w * (T(15) * dx * dy * dy - tx);
        oxyz += w * (T(15) * dx * dy * dz);
        oyyy += w * (T(15) * dy * dy * dy - T(3) * ty);
        oyyz += w * (T(15) * dy * dy * dz - tz);
    }
    T* out = oc + 8 * size_t(n);
    out[0] = oxxx, out[1] = oxxy, out[2] = oxxz, out[3] = oxyy, out[4] = oxyz, out[5] = oyyy, out[6] = oyyz, out[7] = T(0);
}

/*! one level of the octupole upsweep: internal nodes [firstCell, lastCell) from their 8 children shifted by
 *  s = c_child - c_node: O' = O + 5 sym(s Q) - 2 sym(delta (Q s)) + M (15 s s s - 3 |s|^2 sym(s delta)); mp: the FINAL
 *  multipoles of the children's level */
template<class T>
__global__ __launch_bounds__(256) void upsweepOctupolesKernel(NodeIdx firstCell, NodeIdx lastCell,
                                                              const NodeIdx* __restrict__ childOffsets,
                                                              const T* __restrict__ centers, const T* __restrict__ mp,
                                                              T* __restrict__ oc)
{
    const NodeIdx cell = firstCell + blockIdx.x * 256 + threadIdx.x;
    if (cell >= lastCell) return;
    const NodeIdx child = childOffsets[cell];
    if (!child) return;
    const T cx = centers[4 * size_t(cell)], cy = centers[4 * size_t(cell) + 1], cz = centers[4 * size_t(cell) + 2];
    T oxxx = 0, oxxy = 0, oxxz = 0, oxyy = 0, oxyz = 0, oyyy = 0, oyyz = 0;
    for (int k = 0; k < 8; ++k)
    {
        const size_t c = size_t(child + k);
        const T* q     = mp + 8 * c;
        const T* o     = oc + 8 * c;
        const T mc     = q[0];
        const T qxx = q[1], qxy = q[2], qxz = q[3], qyy = q[4], qyz = q[5], qzz = q[6];
        const T sx = centers[4 * c] - cx, sy = centers[4 * c + 1] - cy, sz = centers[4 * c + 2] - cz;
        const T s2 = sx * sx + sy * sy + sz * sz;
        const T qsx = qxx * sx + qxy * sy + qxz * sz;
        const T qsy = qxy * sx + qyy * sy + qyz * sz;
        const T qsz = qxz * sx + qyz * sy + qzz * sz;
        const T tx = T(3) * s2 * sx, ty = T(3) * s2 * sy, tz = T(3) * s2 * sz;
        oxxx += o[0] + T(15) * sx * qxx - T(6) * qsx + mc * (T(15) * sx * sx * sx - T(3) * tx);
        oxxy += o[1] + T(5) * (T(2) * sx * qxy + sy * qxx) - T(2) * qsy + mc * (T(15) * sx * sx * sy - ty);
        oxxz += o[2] + T(5) * (T(2) * sx * qxz + sz * qxx) - T(2) * qsz + mc * (T(15) * sx * sx * sz - tz);
        oxyy += o[3] + T(5) * (sx * qyy + T(2) * sy * qxy) - T(2) * qsx + mc * (T(15) * sx * sy * sy - tx);
        oxyz += o[4] + T(5) * (sx * qyz + sy * qxz + sz * qxy) + mc * (T(15) * sx * sy * sz);
        oyyy += o[5] + T(15) * sy * qyy - T(6) * qsy + mc * (T(15) * sy * sy * sy - T(3) * ty);
        oyyz += o[6] + T(5) * (T(2) * sy * qyz + sz * qyy) - T(2) * qsz + mc * (T(15) * sy * sy * sz - tz);
    }
    T* out = oc + 8 * size_t(cell);
    out[0] = oxxx, out[1] = oxxy, out[2] = oxxz, out[3] = oxyy, out[4] = oxyz, out[5] = oyyy, out[6] = oyyz, out[7] = T(0);
}

/*! P2P of one tile: the cnt <= 64 sources that the lanes hold in (xl, yl, zl, ml[, hl]), source k being particle
 *  base + k, on the lane's target i; d = r_j - r_i, the target itself skipped.  The inner loop of the walk and of the
 *  direct sum: it touches no memory.  SOFT: the rule of the head of the file with H = hi + h_j */
template<bool SOFT, class T>
__device__ __forceinline__ void p2pTile(T xl, T yl, T zl, T ml, T hl, int cnt, uint32_t base, uint32_t i, T xi, T yi,
                                        T zi, T hi, T eps2, T& axi, T& ayi, T& azi, T& phii)
{
    for (int k = 0; k < cnt; ++k)
    {
        const T dx = readLane(xl, k) - xi, dy = readLane(yl, k) - yi, dz = readLane(zl, k) - zi;
        const T mj = readLane(ml, k);
        const T r2 = dx * dx + dy * dy + dz * dz + eps2;
        if constexpr (SOFT)
        {
            const T H      = hi + readLane(hl, k);
            const T H2     = H * H;
            const bool in  = r2 < H2;
            T rinv         = T(1) / sqrt(in ? H2 : r2);
            rinv           = (base + uint32_t(k) == i) ? T(0) : rinv;
            const T mr     = mj * rinv;
            const T mr3    = mr * rinv * rinv; // (the Plummer branch's order: h == 0 gives its bits)
            const T w      = in ? T(1.5) - T(0.5) * r2 * (rinv * rinv) : T(1);
            axi += mr3 * dx;
            ayi += mr3 * dy;
            azi += mr3 * dz;
            phii -= mr * w;
        }
        else
        {
            T rinv      = T(1) / sqrt(r2);
            rinv        = (base + uint32_t(k) == i) ? T(0) : rinv;
            const T mr  = mj * rinv;
            const T mr3 = mr * rinv * rinv;
            axi += mr3 * dx;
            ayi += mr3 * dy;
            azi += mr3 * dz;
            phii -= mr;
        }
    }
}

/*! The walk of one target group per wave (see the head of the file).  Outputs are indexed by i - first; lanes without a
 *  target (the tail of a group) take the group's first particle as a stand-in and write nothing.  SOFT: h, indexed like
 *  x (by particle, not by i - first), softens the P2P pairs; without it h is not read.  ORDER: 0 monopole, 2 adds the
 *  quadrupole, 3 the octupole as well (oc, read at order 3 only, through the scalar cache like mp). */
template<class T, class Tm, int ORDER, bool LET, bool SOFT>
__global__ __launch_bounds__(GW_BLOCK) void gravityWalkKernel(
    const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z, const Tm* __restrict__ m, uint32_t first,
    uint32_t last, const uint32_t* __restrict__ groups, uint32_t numGroups, const NodeIdx* __restrict__ childOffsets,
    const NodeIdx* __restrict__ internalToLeaf, const uint32_t* __restrict__ layout, const T* __restrict__ centers,
    const T* __restrict__ mp, T G, T eps2, T* __restrict__ ax, T* __restrict__ ay, T* __restrict__ az,
    T* __restrict__ phi, uint32_t* __restrict__ p2pCounts, uint32_t* __restrict__ m2pCounts,
    uint32_t* __restrict__ letCounts, int* __restrict__ errors, const T* __restrict__ h, const T* __restrict__ oc)
{
    __shared__ NodeIdx stacks[GW_WAVES][GW_STACK];
    const int lane = int(threadIdx.x & 63u), wave = int(threadIdx.x >> 6);
    NodeIdx* stack = stacks[wave];

    const uint32_t g = blockIdx.x * GW_WAVES + wave;
    if (g >= numGroups) return;
    const uint32_t gs = max(first, uint32_t(uniform(int32_t(groups[g]))));
    const uint32_t ge = min(last, uint32_t(uniform(int32_t(groups[g + 1]))));

    for (uint32_t chunk = gs; chunk < ge; chunk += 64)
    {
        const uint32_t cend = min(ge, chunk + 64u);
        const bool valid    = chunk + lane < cend;
        const uint32_t i    = valid ? chunk + lane : chunk;
        const T xi = x[i], yi = y[i], zi = z[i];
        T hi = T(0);
        if constexpr (SOFT) hi = h[i];

        // the box of the targets: centre (lo + hi) / 2, half-size (hi - lo) / 2 (identical in every lane)
        const T lox = waveMin(xi), loy = waveMin(yi), loz = waveMin(zi);
        const T hix = waveMax(xi), hiy = waveMax(yi), hiz = waveMax(zi);
        const T tcx = (lox + hix) * T(0.5), tcy = (loy + hiy) * T(0.5), tcz = (loz + hiz) * T(0.5);
        const T tsx = (hix - lox) * T(0.5), tsy = (hiy - loy) * T(0.5), tsz = (hiz - loz) * T(0.5);

        T axi = 0, ayi = 0, azi = 0, phii = 0;
        uint32_t nP2P = 0, nM2P = 0, nLet = 0;

        if (lane == 0) stack[0] = 0;
        int top = 1;
        while (top > 0)
        {
            --top;
            const NodeIdx node = uniform(stack[top]);
            const T* c         = centers + 4 * size_t(node);
            const T macSq      = c[3];
            if (macSq == T(0)) continue; // massless, empty node (set_mac leaves 0 exactly for those)
            const T cx = c[0], cy = c[1], cz = c[2];

            // evaluateMac: minimum distance of the target box to the expansion centre against the MAC radius
            T dX = fabs(tcx - cx) - tsx, dY = fabs(tcy - cy) - tsy, dZ = fabs(tcz - cz) - tsz;
            dX += fabs(dX), dY += fabs(dY), dZ += fabs(dZ);
            dX *= T(0.5), dY *= T(0.5), dZ *= T(0.5);
            const T R2      = dX * dX + (dY * dY + dZ * dZ); // right fold, as traverseNeighbors
            bool open = uniform(int(R2 < fabs(macSq))) != 0;

            NodeIdx child = 0;
            uint32_t jb = 0, je = 0;
            if (open)
            {
                child = uniform(childOffsets[node]);
                if (child == 0)
                {
                    const NodeIdx leaf = uniform(internalToLeaf[node]);
                    jb                 = uint32_t(uniform(int32_t(layout[leaf])));
                    je                 = uint32_t(uniform(int32_t(layout[leaf + 1])));
                    if constexpr (LET)
                    {
                        // a massive leaf whose particles are not here (see the head of the file): its multipole
                        if (jb == je)
                        {
                            open = false;
                            ++nLet;
                        }
                    }
                }
            }

            if (!open)
            {
                // M2P, d = r_i - c_n
                const T* q  = mp + 8 * size_t(node);
                const T M   = q[0];
                const T dx = xi - cx, dy = yi - cy, dz = zi - cz;
                const T r2   = dx * dx + dy * dy + dz * dz + eps2;
                const T rinv = T(1) / sqrt(r2);
                const T rinv2 = rinv * rinv;
                const T mr3   = M * rinv * rinv2;
                if constexpr (ORDER >= 2)
                {
                    const T qx  = q[1] * dx + q[2] * dy + q[3] * dz;
                    const T qy  = q[2] * dx + q[4] * dy + q[5] * dz;
                    const T qz  = q[3] * dx + q[5] * dy + q[6] * dz;
                    const T dqd = dx * qx + dy * qy + dz * qz;
                    const T r5  = rinv2 * rinv2 * rinv;
                    const T f   = mr3 + T(2.5) * dqd * r5 * rinv2;
                    axi += r5 * qx - f * dx;
                    ayi += r5 * qy - f * dy;
                    azi += r5 * qz - f * dz;
                    phii -= M * rinv + T(0.5) * dqd * r5;
                    if constexpr (ORDER == 3)
                    {
                        // u_a = O_abc d_b d_c with Oxzz, Oyzz, Ozzz eliminated by the trace; w = u.d
                        const T* o  = oc + 8 * size_t(node);
                        const T xx = dx * dx - dz * dz, yy = dy * dy - dz * dz;
                        const T xy = dx * dy, xz = dx * dz, yz = dy * dz;
                        const T ux = o[0] * xx + o[3] * yy + T(2) * (o[1] * xy + o[2] * xz + o[4] * yz);
                        const T uy = o[1] * xx + o[5] * yy + T(2) * (o[3] * xy + o[4] * xz + o[6] * yz);
                        const T uz = o[2] * xx + o[6] * yy + T(2) * (o[4] * xy - (o[0] + o[3]) * xz - (o[1] + o[5]) * yz);
                        const T w  = ux * dx + uy * dy + uz * dz;
                        const T r7 = r5 * rinv2;
                        const T hr = T(0.5) * r7;
                        const T g  = (T(7) / T(6)) * w * r7 * rinv2;
                        axi += hr * ux - g * dx;
                        ayi += hr * uy - g * dy;
                        azi += hr * uz - g * dz;
                        phii -= (T(1) / T(6)) * w * r7;
                    }
                }
                else
                {
                    axi -= mr3 * dx;
                    ayi -= mr3 * dy;
                    azi -= mr3 * dz;
                    phii -= M * rinv;
                }
                ++nM2P;
                continue;
            }

            if (child != 0)
            {
                if (top + 8 > GW_STACK)
                {
                    if (lane == 0) atomicOr(errors, 4); // traversal stack overflow: the call reports CSTONE_E_INTERNAL
                    break;
                }
                if (lane < 8) stack[top + lane] = child + 7 - lane; // child 0 is popped first
                top += 8;
                continue;
            }

            // P2P with every particle of the opened leaf, d = r_j - r_i, the target itself skipped
            for (uint32_t base = jb; base < je; base += 64)
            {
                const int cnt = int(min(64u, je - base));
                T xl = T(0), yl = T(0), zl = T(0), ml = T(0), hl = T(0);
                if (lane < cnt)
                {
                    xl = x[base + lane], yl = y[base + lane], zl = z[base + lane];
                    ml = T(m[base + lane]);
                    if constexpr (SOFT) hl = h[base + lane];
                }
                p2pTile<SOFT>(xl, yl, zl, ml, hl, cnt, base, i, xi, yi, zi, hi, eps2, axi, ayi, azi, phii);
            }
            nP2P += (je - jb) - ((i >= jb && i < je) ? 1u : 0u);
        }

        if (valid)
        {
            const uint32_t t = i - first;
            ax[t] = G * axi, ay[t] = G * ayi, az[t] = G * azi;
            if (phi) phi[t] = G * phii;
            if (p2pCounts) p2pCounts[t] = nP2P;
            if (m2pCounts) m2pCounts[t] = nM2P;
            if constexpr (LET)
            {
                if (letCounts) letCounts[t] = nLet;
            }
        }
    }
}

constexpr int DG_BLOCK = 256;
constexpr int DG_WAVES = DG_BLOCK / 64;

//! flag[0] = 1 if any of the target indices is not a particle
__global__ __launch_bounds__(256) void checkTargetsKernel(const uint32_t* __restrict__ targets, uint32_t numTargets,
                                                          uint32_t n, int* __restrict__ flag)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < numTargets && targets[k] >= n) *flag = 1;
}

/*! The direct sum: one wave per 64 targets (target position t: particle targets[t], or first + t without a list), one
 *  per lane; lanes behind the last target take the wave's first target as a stand-in and write nothing.  blockIdx.y
 *  is the segment of the sources: the ceil(n / 64) source tiles are cut into gridDim.y contiguous runs, and the wave
 *  streams the tiles of its run through p2pTile.  partial[(segment * numTargets + t) * 4 ..] = (ax, ay, az, phi) without G */
template<class T, class Tm, bool SOFT>
__global__ __launch_bounds__(DG_BLOCK) void directGravityKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                                const T* __restrict__ z, const Tm* __restrict__ m,
                                                                const T* __restrict__ h, uint32_t n, uint32_t first,
                                                                const uint32_t* __restrict__ targets,
                                                                uint32_t numTargets, T eps2, T* __restrict__ partial)
{
    const int lane = int(threadIdx.x & 63u), wave = int(threadIdx.x >> 6);
    const uint32_t t0 = (blockIdx.x * DG_WAVES + wave) * 64u;
    if (t0 >= numTargets) return;
    const bool valid = t0 + lane < numTargets;
    const uint32_t t = valid ? t0 + lane : t0;
    const uint32_t i = targets ? targets[t] : first + t;
    const T xi = x[i], yi = y[i], zi = z[i];
    T hi = T(0);
    if constexpr (SOFT) hi = h[i];

    const uint32_t seg = blockIdx.y, numSegments = gridDim.y;
    const uint32_t tiles = (n + 63u) / 64u; // (n <= 2^32 - 64: checked by the caller)
    const uint32_t tb = uint32_t(uint64_t(tiles) * seg / numSegments);
    const uint32_t te = uint32_t(uint64_t(tiles) * (seg + 1) / numSegments);

    T axi = 0, ayi = 0, azi = 0, phii = 0;
    for (uint32_t tile = tb; tile < te; ++tile)
    {
        const uint32_t base = tile * 64u;
        const int cnt       = int(min(64u, n - base));
        T xl = T(0), yl = T(0), zl = T(0), ml = T(0), hl = T(0);
        if (lane < cnt)
        {
            xl = x[base + lane], yl = y[base + lane], zl = z[base + lane];
            ml = T(m[base + lane]);
            if constexpr (SOFT) hl = h[base + lane];
        }
        p2pTile<SOFT>(xl, yl, zl, ml, hl, cnt, base, i, xi, yi, zi, hi, eps2, axi, ayi, azi, phii);
    }
    if (valid)
    {
        T* out = partial + (size_t(seg) * numTargets + t) * 4;
        out[0] = axi, out[1] = ayi, out[2] = azi, out[3] = phii;
    }
}

//! the partial sums of the segments added in segment order, times G
template<class T>
__global__ __launch_bounds__(256) void directGravityReduceKernel(const T* __restrict__ partial, uint32_t numTargets,
                                                                 uint32_t numSegments, T G, T* __restrict__ ax,
                                                                 T* __restrict__ ay, T* __restrict__ az,
                                                                 T* __restrict__ phi)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= numTargets) return;
    T a = 0, b = 0, c = 0, p = 0;
    for (uint32_t s = 0; s < numSegments; ++s)
    {
        const T* in = partial + (size_t(s) * numTargets + t) * 4;
        a += in[0], b += in[1], c += in[2], p += in[3];
    }
    ax[t] = G * a, ay[t] = G * b, az[t] = G * c;
    if (phi) phi[t] = G * p;
}

//! the internal nodes of every level, deepest first, from their children
template<class T>
int upsweepLevels(cstone_hip_ctx* ctx, int numLevels, const int32_t* levelRangeHost, const int32_t* childOffsets,
                  const void* centers, void* multipoles)
{
    for (int level = numLevels - 1; level >= 0; --level)
    {
        const int first = levelRangeHost[level], last = levelRangeHost[level + 1];
        if (last <= first) continue;
        hipLaunchKernelGGL(upsweepMultipolesKernel<T>, gridFor(size_t(last - first), 256), 256, 0, ctx->stream, first,
                           last, childOffsets, (const T*)centers, (T*)multipoles);
    }
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

template<class T, class Tm>
int upsweepMultipoles(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* m,
                      const int32_t* leafToInternal, int numLeaves, const uint32_t* layout, int numLevels,
                      const int32_t* levelRangeHost, const int32_t* childOffsets, const void* centers, void* multipoles)
{
    hipLaunchKernelGGL((leafMultipolesKernel<T, Tm>), gridFor(size_t(numLeaves), 256), 256, 0, ctx->stream,
                       (const T*)x, (const T*)y, (const T*)z, (const Tm*)m, leafToInternal, numLeaves, layout,
                       (const T*)centers, (T*)multipoles);
    return upsweepLevels<T>(ctx, numLevels, levelRangeHost, childOffsets, centers, multipoles);
}

//! the octupoles of the internal nodes of every level, deepest first; multipoles: already swept up
template<class T>
int upsweepOctupoleLevels(cstone_hip_ctx* ctx, int numLevels, const int32_t* levelRangeHost, const int32_t* childOffsets,
                          const void* centers, const void* multipoles, void* octupoles)
{
    for (int level = numLevels - 1; level >= 0; --level)
    {
        const int first = levelRangeHost[level], last = levelRangeHost[level + 1];
        if (last <= first) continue;
        hipLaunchKernelGGL(upsweepOctupolesKernel<T>, gridFor(size_t(last - first), 256), 256, 0, ctx->stream, first,
                           last, childOffsets, (const T*)centers, (const T*)multipoles, (T*)octupoles);
    }
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

template<class T, class Tm>
int upsweepOctupoles(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* m,
                     const int32_t* leafToInternal, int numLeaves, const uint32_t* layout, int numLevels,
                     const int32_t* levelRangeHost, const int32_t* childOffsets, const void* centers,
                     const void* multipoles, void* octupoles)
{
    hipLaunchKernelGGL((leafOctupolesKernel<T, Tm>), gridFor(size_t(numLeaves), 256), 256, 0, ctx->stream, (const T*)x,
                       (const T*)y, (const T*)z, (const Tm*)m, leafToInternal, numLeaves, layout, (const T*)centers,
                       (T*)octupoles);
    return upsweepOctupoleLevels<T>(ctx, numLevels, levelRangeHost, childOffsets, centers, multipoles, octupoles);
}

//! level_range_host must be num_levels + 1 ranges of [0, num_nodes)
bool badLevelRanges(int num_levels, const int32_t* level_range_host, int num_nodes)
{
    for (int level = 0; level < num_levels; ++level)
        if (level_range_host[level] < 0 || level_range_host[level + 1] < level_range_host[level] ||
            level_range_host[level + 1] > num_nodes)
            return true;
    return false;
}

template<class T, class Tm, int ORDER, bool LET, bool SOFT>
void launchWalk(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* m, const void* h,
                uint32_t first,
                uint32_t last, const uint32_t* groups, uint32_t numGroups, const int32_t* childOffsets,
                const int32_t* internalToLeaf, const uint32_t* layout, const void* centers, const void* multipoles,
                const void* octupoles, double G, double eps2, void* ax, void* ay, void* az, void* phi, uint32_t* p2p,
                uint32_t* m2p, uint32_t* letM2p)
{
    hipLaunchKernelGGL((gravityWalkKernel<T, Tm, ORDER, LET, SOFT>), gridFor(numGroups, GW_WAVES), GW_BLOCK, 0, ctx->stream,
                       (const T*)x, (const T*)y, (const T*)z, (const Tm*)m, first, last, groups, numGroups, childOffsets,
                       internalToLeaf, layout, (const T*)centers, (const T*)multipoles, T(G), T(eps2), (T*)ax, (T*)ay,
                       (T*)az, (T*)phi, p2p, m2p, letM2p, ctx->devScalars + 63, (const T*)h, (const T*)octupoles);
}

template<class T, class Tm>
int launchGravity(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* m, const void* h,
                  uint32_t first, uint32_t last, const uint32_t* groups, uint32_t numGroups, const int32_t* childOffsets,
                  const int32_t* internalToLeaf, const uint32_t* layout, const void* centers, const void* multipoles,
                  const void* octupoles, int order, bool let, double G, double eps2, void* ax, void* ay, void* az,
                  void* phi, uint32_t* p2p, uint32_t* m2p, uint32_t* letM2p)
{
#define CSTONE_WALK(ORDER, LET, SOFT)                                                                                  \
    launchWalk<T, Tm, ORDER, LET, SOFT>(ctx, x, y, z, m, h, first, last, groups, numGroups, childOffsets,               \
                                        internalToLeaf, layout, centers, multipoles, octupoles, G, eps2, ax, ay, az,   \
                                        phi, p2p, m2p, letM2p)
    if (h)
    {
        if (order == 3) { let ? CSTONE_WALK(3, true, true) : CSTONE_WALK(3, false, true); }
        else if (order == 2) { let ? CSTONE_WALK(2, true, true) : CSTONE_WALK(2, false, true); }
        else { let ? CSTONE_WALK(0, true, true) : CSTONE_WALK(0, false, true); }
    }
    else if (order == 3) { let ? CSTONE_WALK(3, true, false) : CSTONE_WALK(3, false, false); }
    else if (order == 2) { let ? CSTONE_WALK(2, true, false) : CSTONE_WALK(2, false, false); }
    else { let ? CSTONE_WALK(0, true, false) : CSTONE_WALK(0, false, false); }
#undef CSTONE_WALK
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

//! the checks and the dispatch behind cstone_hip_compute_gravity, cstone_hip_compute_gravity_let (octupoles == null,
//! order 0 | 2) and cstone_hip_compute_gravity_o3 (order 3, which needs the octupoles)
int computeGravity(cstone_hip_ctx* ctx, bool let, const char* name, int real_bits, int mass_bits, const void* x,
                   const void* y, const void* z, const void* m, const void* h, uint32_t first, uint32_t last,
                   const uint32_t* groups, uint32_t num_groups, const cstone_box* box_host, const int32_t* child_offsets,
                   const int32_t* internal_to_leaf, const uint32_t* layout, const void* expansion_centers,
                   const void* multipoles, const void* octupoles, int order, double G, double eps2, void* ax, void* ay,
                   void* az, void* phi, uint32_t* p2p_counts, uint32_t* m2p_counts, uint32_t* let_m2p_counts);

bool badBits(int bits) { return bits != 32 && bits != 64; }

int computeGravity(cstone_hip_ctx* ctx, bool let, const char* name, int real_bits, int mass_bits, const void* x,
                   const void* y, const void* z, const void* m, const void* h, uint32_t first, uint32_t last,
                   const uint32_t* groups, uint32_t num_groups, const cstone_box* box_host, const int32_t* child_offsets,
                   const int32_t* internal_to_leaf, const uint32_t* layout, const void* expansion_centers,
                   const void* multipoles, const void* octupoles, int order, double G, double eps2, void* ax, void* ay,
                   void* az, void* phi, uint32_t* p2p_counts, uint32_t* m2p_counts, uint32_t* let_m2p_counts)
{
    const bool badOrder = order == 3 ? !octupoles : (order != 0 && order != 2);
    if (!ctx || badBits(real_bits) || badBits(mass_bits) || badOrder || !(eps2 >= 0.0) ||
        last < first || !x || !y || !z || !m || (num_groups && !groups) || !box_host || !child_offsets ||
        !internal_to_leaf || !layout || !expansion_centers || !multipoles || !ax || !ay || !az)
        return fail(ctx, CSTONE_E_ARG, "%s: bad argument", name);
    if (box_host->bc[0] == 1 || box_host->bc[1] == 1 || box_host->bc[2] == 1)
        return fail(ctx, CSTONE_E_ARG, "%s: periodic boundaries need Ewald summation, which is not provided", name);
    if (last == first || num_groups == 0) return CSTONE_OK;
    {
        StageTimer timer(ctx, CSTONE_STAGE_GRAVITY);
#define CSTONE_GRAVITY(T, Tm)                                                                                          \
    launchGravity<T, Tm>(ctx, x, y, z, m, h, first, last, groups, num_groups, child_offsets, internal_to_leaf, layout,     \
                         expansion_centers, multipoles, octupoles, order, let, G, eps2, ax, ay, az, phi, p2p_counts,    \
                         m2p_counts, let_m2p_counts)
        int rc;
        if (real_bits == 64) rc = mass_bits == 64 ? CSTONE_GRAVITY(double, double) : CSTONE_GRAVITY(double, float);
        else rc = mass_bits == 64 ? CSTONE_GRAVITY(float, double) : CSTONE_GRAVITY(float, float);
#undef CSTONE_GRAVITY
        CS_TRY(rc);
    }
    // a stack overflow of the walk sets the sticky error word: report it here instead of returning a partial result
    return cstone_hip_ctx_sync(ctx);
}

//! how many segments cstone_hip_direct_gravity cuts the sources into when the caller leaves it open (see the header)
uint32_t directSegments(uint32_t numTargets, uint32_t n)
{
    const uint32_t tiles  = (n + 63u) / 64u;
    const uint32_t blocks = (numTargets + DG_BLOCK - 1) / DG_BLOCK;
    const uint32_t fill   = (1024u + blocks - 1) / blocks; // 1024 blocks of 4 waves: 16 waves on each of 256 CUs
    return std::max(1u, std::min(fill, tiles / 8u));       // at least 8 tiles (512 sources) per segment
}

template<class T, class Tm>
int launchDirect(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* m, const void* h,
                 uint32_t n, uint32_t first, const uint32_t* targets, uint32_t numTargets, uint32_t numSegments,
                 double G, double eps2, void* partial, void* ax, void* ay, void* az, void* phi)
{
    const dim3 grid(gridFor(numTargets, DG_BLOCK), numSegments);
    if (h)
        hipLaunchKernelGGL((directGravityKernel<T, Tm, true>), grid, DG_BLOCK, 0, ctx->stream, (const T*)x, (const T*)y,
                           (const T*)z, (const Tm*)m, (const T*)h, n, first, targets, numTargets, T(eps2), (T*)partial);
    else
        hipLaunchKernelGGL((directGravityKernel<T, Tm, false>), grid, DG_BLOCK, 0, ctx->stream, (const T*)x,
                           (const T*)y, (const T*)z, (const Tm*)m, (const T*)nullptr, n, first, targets, numTargets,
                           T(eps2), (T*)partial);
    hipLaunchKernelGGL(directGravityReduceKernel<T>, gridFor(numTargets, 256), 256, 0, ctx->stream, (const T*)partial,
                       numTargets, numSegments, T(G), (T*)ax, (T*)ay, (T*)az, (T*)phi);
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

} // namespace

} // namespace cship

using namespace cship;

extern "C"
{

int cstone_hip_upsweep_multipoles(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                  const void* z, const void* m, const int32_t* leaf_to_internal, int num_leaves,
                                  const uint32_t* layout, int num_levels, const int32_t* level_range_host,
                                  const int32_t* child_offsets, int num_nodes, const void* expansion_centers,
                                  void* multipoles)
{
    if (!ctx || badBits(real_bits) || badBits(mass_bits) || num_leaves < 1 || num_nodes < num_leaves || num_levels < 0 ||
        !x || !y || !z || !m || !leaf_to_internal || !layout || !level_range_host || !child_offsets ||
        !expansion_centers || !multipoles)
        return fail(ctx, CSTONE_E_ARG, "upsweep_multipoles: bad argument");
    for (int level = 0; level < num_levels; ++level)
        if (level_range_host[level] < 0 || level_range_host[level + 1] < level_range_host[level] ||
            level_range_host[level + 1] > num_nodes)
            return fail(ctx, CSTONE_E_ARG, "upsweep_multipoles: level_range_host is not a range of [0, num_nodes)");
    StageTimer timer(ctx, CSTONE_STAGE_MULTIPOLES);
#define CSTONE_UPSWEEP(T, Tm)                                                                                          \
    upsweepMultipoles<T, Tm>(ctx, x, y, z, m, leaf_to_internal, num_leaves, layout, num_levels, level_range_host,      \
                             child_offsets, expansion_centers, multipoles)
    if (real_bits == 64) return mass_bits == 64 ? CSTONE_UPSWEEP(double, double) : CSTONE_UPSWEEP(double, float);
    return mass_bits == 64 ? CSTONE_UPSWEEP(float, double) : CSTONE_UPSWEEP(float, float);
#undef CSTONE_UPSWEEP
}

int cstone_hip_compute_gravity_h(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                 const void* z, const void* m, const void* h, uint32_t first, uint32_t last,
                                 const uint32_t* groups, uint32_t num_groups, const cstone_box* box_host,
                                 const int32_t* child_offsets, const int32_t* internal_to_leaf, const uint32_t* layout,
                                 const void* expansion_centers, const void* multipoles, int order, double G, double eps2,
                                 void* ax, void* ay, void* az, void* phi, uint32_t* p2p_counts, uint32_t* m2p_counts)
{
    return computeGravity(ctx, false, "compute_gravity", real_bits, mass_bits, x, y, z, m, h, first, last, groups,
                          num_groups, box_host, child_offsets, internal_to_leaf, layout, expansion_centers, multipoles,
                          nullptr, order, G, eps2, ax, ay, az, phi, p2p_counts, m2p_counts, nullptr);
}

int cstone_hip_compute_gravity(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                               const void* z, const void* m, uint32_t first, uint32_t last, const uint32_t* groups,
                               uint32_t num_groups, const cstone_box* box_host, const int32_t* child_offsets,
                               const int32_t* internal_to_leaf, const uint32_t* layout, const void* expansion_centers,
                               const void* multipoles, int order, double G, double eps2, void* ax, void* ay, void* az,
                               void* phi, uint32_t* p2p_counts, uint32_t* m2p_counts)
{
    return cstone_hip_compute_gravity_h(ctx, real_bits, mass_bits, x, y, z, m, nullptr, first, last, groups, num_groups,
                                        box_host, child_offsets, internal_to_leaf, layout, expansion_centers, multipoles,
                                        order, G, eps2, ax, ay, az, phi, p2p_counts, m2p_counts);
}

int cstone_hip_compute_gravity_let_h(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                     const void* z, const void* m, const void* h, uint32_t first, uint32_t last,
                                     const uint32_t* groups, uint32_t num_groups, const cstone_box* box_host,
                                     const int32_t* child_offsets, const int32_t* internal_to_leaf,
                                     const uint32_t* layout, const void* expansion_centers, const void* multipoles,
                                     int order, double G, double eps2, void* ax, void* ay, void* az, void* phi,
                                     uint32_t* p2p_counts, uint32_t* m2p_counts, uint32_t* let_m2p_counts)
{
    return computeGravity(ctx, true, "compute_gravity_let", real_bits, mass_bits, x, y, z, m, h, first, last, groups,
                          num_groups, box_host, child_offsets, internal_to_leaf, layout, expansion_centers, multipoles,
                          nullptr, order, G, eps2, ax, ay, az, phi, p2p_counts, m2p_counts, let_m2p_counts);
}

int cstone_hip_compute_gravity_let(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                   const void* z, const void* m, uint32_t first, uint32_t last, const uint32_t* groups,
                                   uint32_t num_groups, const cstone_box* box_host, const int32_t* child_offsets,
                                   const int32_t* internal_to_leaf, const uint32_t* layout,
                                   const void* expansion_centers, const void* multipoles, int order, double G,
                                   double eps2, void* ax, void* ay, void* az, void* phi, uint32_t* p2p_counts,
                                   uint32_t* m2p_counts, uint32_t* let_m2p_counts)
{
    return cstone_hip_compute_gravity_let_h(ctx, real_bits, mass_bits, x, y, z, m, nullptr, first, last, groups,
                                            num_groups, box_host, child_offsets, internal_to_leaf, layout,
                                            expansion_centers, multipoles, order, G, eps2, ax, ay, az, phi, p2p_counts,
                                            m2p_counts, let_m2p_counts);
}

int cstone_hip_direct_gravity(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                              const void* z, const void* m, const void* h, uint32_t n, uint32_t first, uint32_t last,
                              const uint32_t* targets, uint32_t num_targets, int num_segments, double G, double eps2,
                              void* ax, void* ay, void* az, void* phi)
{
    if (!ctx || badBits(real_bits) || badBits(mass_bits) || !(eps2 >= 0.0) || num_segments < 0 || n > 0xffffffffu - 64u)
        return fail(ctx, CSTONE_E_ARG, "direct_gravity: bad argument");
    if (!targets && (last < first || last > n)) return fail(ctx, CSTONE_E_ARG, "direct_gravity: [first, last) is not a range of [0, n)");
    const uint32_t nt = targets ? num_targets : last - first;
    if (nt == 0) return CSTONE_OK;
    if (n == 0 || !x || !y || !z || !m || !ax || !ay || !az)
        return fail(ctx, CSTONE_E_ARG, "direct_gravity: bad argument");

    const uint32_t tiles = (n + 63u) / 64u;
    const uint32_t segs  = std::min(std::min(num_segments ? uint32_t(num_segments) : directSegments(nt, n), tiles), 65535u);
    const size_t wsBytes = alignUp(size_t(segs) * nt * 4 * size_t(real_bits / 8));
    CS_TRY(arenaReserve(ctx, wsBytes + 512));
    void* partial = arenaTake(ctx, wsBytes);
    int rc        = CSTONE_OK;
    if (targets)
    {
        // an index that is no particle must not reach the loads: looked for on the device, the flag read before the sum
        int* flag     = (int*)arenaTake(ctx, 256);
        int bad       = 0;
        hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), ctx->stream);
        if (e == hipSuccess)
        {
            hipLaunchKernelGGL(checkTargetsKernel, gridFor(nt, 256), 256, 0, ctx->stream, targets, nt, n, flag);
            e = hipGetLastError();
        }
        if (e != hipSuccess) rc = fail(ctx, CSTONE_E_HIP, "direct_gravity: %s", hipGetErrorString(e));
        if (rc == CSTONE_OK) rc = copyToHost(ctx, &bad, flag, sizeof(int));
        if (rc == CSTONE_OK && bad) rc = fail(ctx, CSTONE_E_ARG, "direct_gravity: a target index is not below n");
    }
    if (rc == CSTONE_OK)
    {
        StageTimer timer(ctx, CSTONE_STAGE_GRAVITY);
#define CSTONE_DIRECT(T, Tm)                                                                                           \
    launchDirect<T, Tm>(ctx, x, y, z, m, h, n, first, targets, nt, segs, G, eps2, partial, ax, ay, az, phi)
        if (real_bits == 64) rc = mass_bits == 64 ? CSTONE_DIRECT(double, double) : CSTONE_DIRECT(double, float);
        else rc = mass_bits == 64 ? CSTONE_DIRECT(float, double) : CSTONE_DIRECT(float, float);
#undef CSTONE_DIRECT
    }
    arenaReset(ctx);
    return rc;
}

int cstone_hip_upsweep_multipoles_nodes(cstone_hip_ctx* ctx, int real_bits, int num_levels,
                                        const int32_t* level_range_host, const int32_t* child_offsets, int num_nodes,
                                        const void* expansion_centers, void* multipoles)
{
    if (!ctx || badBits(real_bits) || num_levels < 0 || num_nodes < 1 || !level_range_host || !child_offsets ||
        !expansion_centers || !multipoles)
        return fail(ctx, CSTONE_E_ARG, "upsweep_multipoles_nodes: bad argument");
    for (int level = 0; level < num_levels; ++level)
        if (level_range_host[level] < 0 || level_range_host[level + 1] < level_range_host[level] ||
            level_range_host[level + 1] > num_nodes)
            return fail(ctx, CSTONE_E_ARG, "upsweep_multipoles_nodes: level_range_host is not a range of [0, num_nodes)");
    StageTimer timer(ctx, CSTONE_STAGE_MULTIPOLES);
    if (real_bits == 64)
        return upsweepLevels<double>(ctx, num_levels, level_range_host, child_offsets, expansion_centers, multipoles);
    return upsweepLevels<float>(ctx, num_levels, level_range_host, child_offsets, expansion_centers, multipoles);
}

int cstone_hip_upsweep_octupoles(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                 const void* z, const void* m, const int32_t* leaf_to_internal, int num_leaves,
                                 const uint32_t* layout, int num_levels, const int32_t* level_range_host,
                                 const int32_t* child_offsets, int num_nodes, const void* expansion_centers,
                                 const void* multipoles, void* octupoles)
{
    if (!ctx || badBits(real_bits) || badBits(mass_bits) || num_leaves < 1 || num_nodes < num_leaves || num_levels < 0 ||
        !x || !y || !z || !m || !leaf_to_internal || !layout || !level_range_host || !child_offsets ||
        !expansion_centers || !multipoles || !octupoles)
        return fail(ctx, CSTONE_E_ARG, "upsweep_octupoles: bad argument");
    if (badLevelRanges(num_levels, level_range_host, num_nodes))
        return fail(ctx, CSTONE_E_ARG, "upsweep_octupoles: level_range_host is not a range of [0, num_nodes)");
    StageTimer timer(ctx, CSTONE_STAGE_MULTIPOLES);
#define CSTONE_UPSWEEP(T, Tm)                                                                                          \
    upsweepOctupoles<T, Tm>(ctx, x, y, z, m, leaf_to_internal, num_leaves, layout, num_levels, level_range_host,       \
                            child_offsets, expansion_centers, multipoles, octupoles)
    if (real_bits == 64) return mass_bits == 64 ? CSTONE_UPSWEEP(double, double) : CSTONE_UPSWEEP(double, float);
    return mass_bits == 64 ? CSTONE_UPSWEEP(float, double) : CSTONE_UPSWEEP(float, float);
#undef CSTONE_UPSWEEP
}

int cstone_hip_upsweep_octupoles_nodes(cstone_hip_ctx* ctx, int real_bits, int num_levels,
                                       const int32_t* level_range_host, const int32_t* child_offsets, int num_nodes,
                                       const void* expansion_centers, const void* multipoles, void* octupoles)
{
    if (!ctx || badBits(real_bits) || num_levels < 0 || num_nodes < 1 || !level_range_host || !child_offsets ||
        !expansion_centers || !multipoles || !octupoles)
        return fail(ctx, CSTONE_E_ARG, "upsweep_octupoles_nodes: bad argument");
    if (badLevelRanges(num_levels, level_range_host, num_nodes))
        return fail(ctx, CSTONE_E_ARG, "upsweep_octupoles_nodes: level_range_host is not a range of [0, num_nodes)");
    StageTimer timer(ctx, CSTONE_STAGE_MULTIPOLES);
    if (real_bits == 64)
        return upsweepOctupoleLevels<double>(ctx, num_levels, level_range_host, child_offsets, expansion_centers,
                                             multipoles, octupoles);
    return upsweepOctupoleLevels<float>(ctx, num_levels, level_range_host, child_offsets, expansion_centers, multipoles,
                                        octupoles);
}

int cstone_hip_compute_gravity_o3(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                  const void* z, const void* m, const void* h, uint32_t first, uint32_t last,
                                  const uint32_t* groups, uint32_t num_groups, const cstone_box* box_host,
                                  const int32_t* child_offsets, const int32_t* internal_to_leaf, const uint32_t* layout,
                                  const void* expansion_centers, const void* multipoles, const void* octupoles, int let,
                                  double G, double eps2, void* ax, void* ay, void* az, void* phi, uint32_t* p2p_counts,
                                  uint32_t* m2p_counts, uint32_t* let_m2p_counts)
{
    return computeGravity(ctx, let != 0, "compute_gravity_o3", real_bits, mass_bits, x, y, z, m, h, first, last, groups,
                          num_groups, box_host, child_offsets, internal_to_leaf, layout, expansion_centers, multipoles,
                          octupoles, 3, G, eps2, ax, ay, az, phi, p2p_counts, m2p_counts,
                          let ? let_m2p_counts : nullptr);
}

} // extern "C"
