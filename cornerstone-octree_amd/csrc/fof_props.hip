// The friends-of-friends group catalogue on gfx950: mass, centre, velocity and rms radius of every group of a catalogue
// (cstone_hip_fof_group_properties), and the device steps of the catalogue across ranks
// (cstone_hip_domain_mr_fof_catalog, domain_mr.hip).  The rule -- offsets from the group's reference folded once in the
// coordinate type, sums in double, the WIDE and MASSLESS flags -- is stated in include/cstone_hip.h.
//
// The hot path is a segmented reduction over members[]: one lane takes one member, reads members[] coalesced and gathers
// x, y, z, m (, v) and the group's reference through it; a segmented inclusive scan over the 5 or 8 doubles runs inside the
// wave (six __shfl_up steps, a lane adds its neighbour's value iff that neighbour is at or behind the head of the lane's
// own segment).  The launch shape is FIXED: FOFP_WAVES waves, wave w walks the 64-member chunks [w cpw, (w + 1) cpw) with
// cpw = ceil(ceil(n / 64) / FOFP_WAVES) and carries the open segment from chunk to chunk in registers.  n =
// group_offsets[num_groups] is read on the device, so the call needs no read-back.  A group that begins and ends inside
// one wave's span is finished by the lane of its last member.  What is left are the first and the last segment of a span:
// they go to two carry slots per wave (the context's workspace), and a second kernel -- one wave per group that spans
// waves -- adds them in wave order: lane l sums a contiguous block of ceil(c / 64) carries, then a butterfly over the
// lanes.  No atomics; the order of every sum is a function of n and the group edges alone.
//
// How a lane learns its group: a binary search in group_offsets.  One full search per wave (for the first member of its
// span, the same address in every lane), then every lane searches the at most lane + 2 groups behind the group of the
// previous chunk's last lane -- groups are not empty, so member k + l cannot be further than l groups on: seven probes of
// a few cached lines.  Head flags plus the library's inclusive scan would need two more passes over n words and n words
// of workspace whose size the host does not know without a read-back.
#include <algorithm>

#include "cstone_hip_device.hpp"
#include "ctx.hpp"
#include "fof_props.hpp"
#include "scan.hpp"

namespace cship
{

namespace
{

constexpr uint32_t FOFP_WAVES  = 8192; // the fixed shape: 2048 workgroups of 4 waves
constexpr uint32_t FOFP_NONE   = 0xffffffffu;
constexpr int FOFP_ERR_LABEL   = 32; // bit of the sticky error word (that of fof.hip: a label outside its range)

//! the first or last segment of a wave's span: the group it belongs to (FOFP_NONE: the slot is empty) and its sums
struct FofCarry
{
    uint32_t group, wide;
    double v[8];
};

template<class T>
__device__ __forceinline__ T foldOffset(T d, T len, bool periodic)
{
    if (periodic)
    {
        const T half = T(0.5) * len;
        if (d >= half) d -= len;
        else if (d < -half) d += len;
    }
    return d;
}

template<class T>
__device__ __forceinline__ bool isWide(T d, T len, bool periodic)
{
    return periodic && fabs(d) >= T(0.25) * len;
}

//! the results of one group from its sums about ref (section "Results" of the rule), row `row` of the outputs
template<class T>
__device__ inline void fofFinishRow(const double* v, bool velocities, uint32_t wide, const double* ref,
                                    const cstone_hip::DeviceBox<T>& box, size_t row, const FofGroupOut& o)
{
    uint32_t fl    = wide ? CSTONE_FOF_GROUP_WIDE : 0u;
    const double M = v[0];
    T c[3], vel[3] = {T(0), T(0), T(0)}, rad = T(0);
    if (M == 0.0)
    {
        fl |= CSTONE_FOF_GROUP_MASSLESS;
        for (int a = 0; a < 3; ++a)
            c[a] = T(ref[a]);
    }
    else
    {
        double cm[3];
        for (int a = 0; a < 3; ++a)
        {
            cm[a]     = v[1 + a] / M;
            double cd = ref[a] + cm[a];
            if (box.bc[a] == 1)
            {
                if (cd < double(box.lo[a])) cd += double(box.len[a]);
                else if (cd >= double(box.hi[a])) cd -= double(box.len[a]);
            }
            T ct = T(cd);
            if (box.bc[a] == 1 && ct >= box.hi[a]) ct = box.lo[a]; // (the rounding to T may land on the upper face)
            c[a] = ct;
            if (velocities) vel[a] = T(v[5 + a] / M);
        }
        const double r2 = v[4] / M - (cm[0] * cm[0] + cm[1] * cm[1] + cm[2] * cm[2]);
        rad             = T(sqrt(r2 > 0.0 ? r2 : 0.0));
    }
    static_cast<T*>(o.mass)[row] = T(M);
    for (int a = 0; a < 3; ++a)
        static_cast<T*>(o.center)[3 * row + a] = c[a];
    if (o.velocity && velocities)
        for (int a = 0; a < 3; ++a)
            static_cast<T*>(o.velocity)[3 * row + a] = vel[a];
    if (o.radius) static_cast<T*>(o.radius)[row] = rad;
    if (o.flags) o.flags[row] = fl;
}

template<class T, bool RAW>
__device__ inline void fofEmitGroup(uint32_t g, const double* v, bool velocities, uint32_t wide, T rx, T ry, T rz,
                                    uint32_t gs, uint32_t ge, const cstone_hip::DeviceBox<T>& box, const FofGroupOut& out,
                                    FofPartial* __restrict__ partials, const uint64_t* __restrict__ sortedLabels)
{
    const double ref[3] = {double(rx), double(ry), double(rz)};
    if constexpr (RAW)
    {
        FofPartial p;
        p.label = sortedLabels[gs];
        p.count = ge - gs;
        for (int i = 0; i < 8; ++i)
            p.sums[i] = (velocities || i < 5) ? v[i] : 0.0;
        for (int a = 0; a < 3; ++a)
            p.ref[a] = ref[a];
        p.wide = wide ? 1u : 0u;
        p.pad  = 0;
        partials[g] = p;
    }
    else { fofFinishRow<T>(v, velocities, wide, ref, box, g, out); }
}

//! cpw, the chunks of 64 members one wave walks, for n members in all
__device__ __forceinline__ uint32_t chunksPerWave(uint32_t n)
{
    const uint32_t chunks = uint32_t((uint64_t(n) + 63u) / 64u);
    const uint32_t cpw    = (chunks + FOFP_WAVES - 1) / FOFP_WAVES;
    return cpw ? cpw : 1u;
}

template<class T, class TM, bool VEL, bool RAW>
__global__ __launch_bounds__(256) void fofPropsReduceKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                            const T* __restrict__ z, const TM* __restrict__ m,
                                                            const T* __restrict__ vx, const T* __restrict__ vy,
                                                            const T* __restrict__ vz, cstone_hip::DeviceBox<T> box,
                                                            const uint32_t* __restrict__ offsets,
                                                            const uint32_t* __restrict__ members, uint32_t G,
                                                            FofCarry* __restrict__ carries, FofGroupOut out,
                                                            FofPartial* __restrict__ partials,
                                                            const uint64_t* __restrict__ sortedLabels)
{
    constexpr int NV    = VEL ? 8 : 5;
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t w    = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t n    = offsets[G];
    const uint32_t chunks = uint32_t((uint64_t(n) + 63u) / 64u);
    const uint32_t cpw    = chunksPerWave(n);
    const uint64_t c0 = uint64_t(w) * cpw, c1 = std::min<uint64_t>(c0 + cpw, chunks);
    FofCarry* slot = carries + 2 * size_t(w);
    if (c0 >= c1)
    {
        if (lane < 2) slot[lane].group = FOFP_NONE;
        return;
    }
    const uint32_t spanStart = uint32_t(c0 * 64u);
    const bool px = box.bc[0] == 1, py = box.bc[1] == 1, pz = box.bc[2] == 1;

    // the group of the first member of the span: the smallest g with offsets[g + 1] > spanStart (the same in every lane)
    uint32_t gBase;
    {
        uint32_t lo = 0, hi = G - 1;
        while (lo < hi)
        {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (offsets[mid + 1] > spanStart) hi = mid;
            else lo = mid + 1;
        }
        gBase = lo;
    }

    bool open = false, wrote0 = false, wrote1 = false; // uniform over the wave
    double acc[NV];
    uint32_t accWide = 0, accG = 0;
    for (int i = 0; i < NV; ++i)
        acc[i] = 0.0;

    for (uint64_t c = c0; c < c1; ++c)
    {
        const uint64_t k64 = c * 64u + lane;
        const bool valid   = k64 < n;
        const uint32_t k   = valid ? uint32_t(k64) : n - 1;
        uint32_t g;
        {
            uint32_t lo = gBase, hi = uint32_t(std::min<uint64_t>(uint64_t(gBase) + lane + 1, G - 1));
            while (lo < hi)
            {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (offsets[mid + 1] > k) hi = mid;
                else lo = mid + 1;
            }
            g = lo;
        }
        const uint32_t gs = offsets[g], ge = offsets[g + 1];
        const bool head = valid && k == gs;
        const bool tail = valid && k + 1 == ge;

        const uint32_t ref = members[gs < n ? gs : n - 1]; // (gs < n unless the last group is empty, which is no partition)
        const T rx = x[ref], ry = y[ref], rz = z[ref];
        double v[NV];
        uint32_t wide = 0;
        if (valid)
        {
            const uint32_t j = members[k];
            const T dx = foldOffset(T(x[j] - rx), box.len[0], px);
            const T dy = foldOffset(T(y[j] - ry), box.len[1], py);
            const T dz = foldOffset(T(z[j] - rz), box.len[2], pz);
            wide = (isWide(dx, box.len[0], px) || isWide(dy, box.len[1], py) || isWide(dz, box.len[2], pz)) ? 1u : 0u;
            const double mj = double(m[j]), ex = double(dx), ey = double(dy), ez = double(dz);
            v[0] = mj;
            v[1] = mj * ex;
            v[2] = mj * ey;
            v[3] = mj * ez;
            v[4] = mj * (ex * ex + ey * ey + ez * ez);
            if constexpr (VEL)
            {
                v[5] = mj * double(vx[j]);
                v[6] = mj * double(vy[j]);
                v[7] = mj * double(vz[j]);
            }
        }
        else
        {
            for (int i = 0; i < NV; ++i)
                v[i] = 0.0;
        }

        // the lane of the head of my segment in this chunk; none at or below me: the segment came in from the left
        const uint64_t heads = __ballot(head);
        const uint64_t below = heads & (lane == 63 ? ~uint64_t(0) : ((uint64_t(2) << lane) - 1));
        const unsigned start = below ? 63u - unsigned(__clzll((long long)below)) : 0u;
#pragma unroll
        for (unsigned o = 1; o < 64; o <<= 1)
        {
            const bool take = lane >= start + o;
#pragma unroll
            for (int i = 0; i < NV; ++i)
            {
                const double t = __shfl_up(v[i], o);
                if (take) v[i] = t + v[i];
            }
            const uint32_t tw = uint32_t(__shfl_up(int(wide), o));
            if (take) wide |= tw;
        }
        if (open && !below)
        {
            for (int i = 0; i < NV; ++i)
                v[i] = acc[i] + v[i];
            wide |= accWide;
        }

        // a group's last member: the group is finished here if it began inside the span, else it is the span's first segment
        const bool whole = gs >= spanStart;
        if (tail)
        {
            if (whole) fofEmitGroup<T, RAW>(g, v, VEL, wide, rx, ry, rz, gs, ge, box, out, partials, sortedLabels);
            else
            {
                slot[0].group = g;
                slot[0].wide  = wide;
                for (int i = 0; i < 8; ++i)
                    slot[0].v[i] = i < NV ? v[i] : 0.0;
            }
        }
        wrote0 = wrote0 || __ballot(tail && !whole) != 0;

        // what the last valid lane holds stays open unless its group ends there
        const int lastLane = int(std::min<uint64_t>(63u, uint64_t(n) - 1 - c * 64u));
        open               = !__shfl(int(tail), lastLane);
        gBase              = uint32_t(__shfl(int(g), lastLane));
        if (open)
        {
            for (int i = 0; i < NV; ++i)
                acc[i] = __shfl(v[i], lastLane);
            accWide = uint32_t(__shfl(int(wide), lastLane));
            accG    = gBase;
        }
    }
    if (open)
    {
        // the group goes on behind the span: its last segment, or, if it came in from the left too, its only one
        const int s = offsets[accG] >= spanStart ? 1 : 0;
        if (lane == 0)
        {
            slot[s].group = accG;
            slot[s].wide  = accWide;
            for (int i = 0; i < 8; ++i)
                slot[s].v[i] = i < NV ? acc[i] : 0.0;
        }
        if (s) wrote1 = true;
        else wrote0 = true;
    }
    if (lane == 0 && !wrote0) slot[0].group = FOFP_NONE;
    if (lane == 0 && !wrote1) slot[1].group = FOFP_NONE;
}

/*! one wave per wave w of the reduction whose second slot is taken: the group that begins in w's span and ends in wave
 *  wb > w.  Its carries in wave order: slot 1 of w, slot 0 of w + 1 .. wb. */
template<class T, bool VEL, bool RAW>
__global__ __launch_bounds__(256) void fofPropsCarryKernel(const T* __restrict__ x, const T* __restrict__ y,
                                                           const T* __restrict__ z, cstone_hip::DeviceBox<T> box,
                                                           const uint32_t* __restrict__ offsets,
                                                           const uint32_t* __restrict__ members, uint32_t G,
                                                           const FofCarry* __restrict__ carries, FofGroupOut out,
                                                           FofPartial* __restrict__ partials,
                                                           const uint64_t* __restrict__ sortedLabels)
{
    constexpr int NV    = VEL ? 8 : 5;
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t w    = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t g    = carries[2 * size_t(w) + 1].group;
    if (g == FOFP_NONE || g >= G) return;
    const uint32_t n = offsets[G], cpw = chunksPerWave(n);
    const uint32_t gs = offsets[g], ge = offsets[g + 1];
    if (ge <= gs || ge > n) return;
    const uint32_t wb = std::min(((ge - 1) / 64u) / cpw, FOFP_WAVES - 1);
    if (wb < w) return;
    const uint32_t count = wb - w + 1, per = (count + 63u) / 64u;

    double v[NV];
    for (int i = 0; i < NV; ++i)
        v[i] = 0.0;
    uint32_t wide    = 0;
    const uint32_t a = lane * per, b = std::min(count, a + per);
    for (uint32_t i = a; i < b; ++i)
    {
        const FofCarry& cr = carries[i == 0 ? 2 * size_t(w) + 1 : 2 * (size_t(w) + i)];
        if (cr.group != g) continue; // (cannot be, for offsets that ascend)
        for (int q = 0; q < NV; ++q)
            v[q] = v[q] + cr.v[q];
        wide |= cr.wide;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1)
    {
#pragma unroll
        for (int q = 0; q < NV; ++q)
            v[q] = v[q] + __shfl_xor(v[q], o);
        wide |= uint32_t(__shfl_xor(int(wide), o));
    }
    if (lane == 0)
    {
        const uint32_t ref = members[gs];
        fofEmitGroup<T, RAW>(g, v, VEL, wide, x[ref], y[ref], z[ref], gs, ge, box, out, partials, sortedLabels);
    }
}

template<class T, class TM, bool VEL, bool RAW>
void launchReduce(cstone_hip_ctx* ctx, const void* x, const void* y, const void* z, const void* m, const void* vx,
                  const void* vy, const void* vz, const cstone_box& box, const uint32_t* offsets, const uint32_t* members,
                  uint32_t G, FofCarry* carries, const FofGroupOut& out, FofPartial* partials, const uint64_t* sortedLabels)
{
    const auto dbox = cstone_hip::makeDeviceBox<T>(box);
    hipLaunchKernelGGL((fofPropsReduceKernel<T, TM, VEL, RAW>), FOFP_WAVES / 4, 256, 0, ctx->stream, (const T*)x, (const T*)y,
                       (const T*)z, (const TM*)m, (const T*)vx, (const T*)vy, (const T*)vz, dbox, offsets, members, G, carries,
                       out, partials, sortedLabels);
    hipLaunchKernelGGL((fofPropsCarryKernel<T, VEL, RAW>), FOFP_WAVES / 4, 256, 0, ctx->stream, (const T*)x, (const T*)y,
                       (const T*)z, dbox, offsets, members, G, carries, out, partials, sortedLabels);
}

template<class T, class TM, bool VEL, class... A>
void launchReduceRaw(bool raw, A&&... a)
{
    if (raw) launchReduce<T, TM, VEL, true>(a...);
    else launchReduce<T, TM, VEL, false>(a...);
}

template<class T, class TM, class... A>
void launchReduceVel(bool vel, bool raw, A&&... a)
{
    if (vel) launchReduceRaw<T, TM, true>(raw, a...);
    else launchReduceRaw<T, TM, false>(raw, a...);
}

// ---- the catalogue across ranks -------------------------------------------------------------------------------------------

//! heads[k] = keys[k] begins a run; *bad += keys >= limit
__global__ __launch_bounds__(256) void fofpHeads64Kernel(const uint64_t* __restrict__ keys, uint32_t n, uint64_t limit,
                                                         uint32_t* __restrict__ heads, uint32_t* __restrict__ bad)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) heads[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1u : 0u;
    const uint64_t votes = __ballot(k < n && keys[k] >= limit);
    if ((threadIdx.x & 63u) == 0 && votes) atomicAdd(bad, uint32_t(__popcll(votes)));
}

__global__ __launch_bounds__(256) void fofpRunStarts64Kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ runId,
                                                             uint32_t n, uint32_t* __restrict__ runStart,
                                                             uint64_t* __restrict__ runLabels)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    if (k == 0 || keys[k] != keys[k - 1])
    {
        runStart[runId[k] - 1] = k;
        if (runLabels) runLabels[runId[k] - 1] = keys[k];
    }
    if (k == n - 1) runStart[runId[k]] = n;
}

__global__ __launch_bounds__(256) void fofpLabelsKernel(const FofPartial* __restrict__ records, uint32_t n,
                                                        uint64_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = records[i].label;
}

template<class T>
__global__ __launch_bounds__(256) void fofpCombineKernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                         cstone_hip::DeviceBox<T> box, const FofPartial* __restrict__ records,
                                                         const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ runStart, uint32_t numRuns,
                                                         uint64_t firstId, uint32_t first, uint32_t numOwn, uint64_t minMembers,
                                                         FofPartial* __restrict__ combined, uint32_t* __restrict__ keep,
                                                         int* __restrict__ errors)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= numRuns) return;
    const uint32_t a = runStart[r], b = runStart[r + 1];
    const uint64_t label = records[order[a]].label;
    const uint64_t own   = label - firstId;
    if (own >= numOwn)
    {
        atomicOr(errors, FOFP_ERR_LABEL);
        keep[r] = 0;
        return;
    }
    const uint32_t i0 = first + uint32_t(own);
    const T ref[3]    = {x[i0], y[i0], z[i0]};
    double v[8]       = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t count    = 0;
    uint32_t wide     = 0;
    for (uint32_t i = a; i < b; ++i)
    {
        const FofPartial& p = records[order[i]];
        double s[3];
        for (int d = 0; d < 3; ++d)
        {
            const T sd = foldOffset(T(T(p.ref[d]) - ref[d]), box.len[d], box.bc[d] == 1);
            if (isWide(sd, box.len[d], box.bc[d] == 1)) wide = 1;
            s[d] = double(sd);
        }
        const double Mp = p.sums[0];
        v[0] = v[0] + Mp;
        for (int d = 0; d < 3; ++d)
            v[1 + d] = v[1 + d] + (p.sums[1 + d] + Mp * s[d]);
        const double dot = s[0] * p.sums[1] + s[1] * p.sums[2] + s[2] * p.sums[3];
        const double s2  = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
        v[4] = v[4] + (p.sums[4] + 2.0 * dot + Mp * s2);
        for (int d = 0; d < 3; ++d)
            v[5 + d] = v[5 + d] + p.sums[5 + d];
        count += p.count;
        wide |= p.wide;
    }
    FofPartial c;
    c.label = label;
    c.count = count;
    for (int i = 0; i < 8; ++i)
        c.sums[i] = v[i];
    for (int d = 0; d < 3; ++d)
        c.ref[d] = double(ref[d]);
    c.wide = wide;
    c.pad  = 0;
    combined[r] = c;
    keep[r]     = count >= minMembers ? 1u : 0u;
}

template<class T>
__global__ __launch_bounds__(256) void fofpFinishKernel(cstone_hip::DeviceBox<T> box, bool velocities,
                                                        const FofPartial* __restrict__ combined,
                                                        const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                                                        uint32_t numRuns, FofGroupOut out)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= numRuns || !keep[r]) return;
    const FofPartial& c = combined[r];
    const size_t row    = pos[r];
    fofFinishRow<T>(c.sums, velocities, c.wide, c.ref, box, row, out);
    if (out.labels) out.labels[row] = c.label;
    if (out.sizes) out.sizes[row] = c.count;
}

} // namespace

int fofPropsReduce(cstone_hip_ctx* ctx, int realBits, int massBits, const void* x, const void* y, const void* z, const void* m,
                   const void* vx, const void* vy, const void* vz, const cstone_box& box, const uint32_t* groupOffsets,
                   const uint32_t* members, uint32_t numGroups, const FofGroupOut& out, FofPartial* partials,
                   const uint64_t* sortedLabels)
{
    if (numGroups == 0) return CSTONE_OK;
    const size_t carryBytes = alignUp(2 * size_t(FOFP_WAVES) * sizeof(FofCarry));
    CS_TRY(arenaReserve(ctx, carryBytes + 256));
    FofCarry* carries = static_cast<FofCarry*>(arenaTake(ctx, carryBytes));
    const bool vel = vx != nullptr, raw = partials != nullptr;
    if (realBits == 32 && massBits == 32)
        launchReduceVel<float, float>(vel, raw, ctx, x, y, z, m, vx, vy, vz, box, groupOffsets, members, numGroups, carries, out,
                                      partials, sortedLabels);
    else if (realBits == 32)
        launchReduceVel<float, double>(vel, raw, ctx, x, y, z, m, vx, vy, vz, box, groupOffsets, members, numGroups, carries, out,
                                       partials, sortedLabels);
    else if (massBits == 32)
        launchReduceVel<double, float>(vel, raw, ctx, x, y, z, m, vx, vy, vz, box, groupOffsets, members, numGroups, carries, out,
                                       partials, sortedLabels);
    else
        launchReduceVel<double, double>(vel, raw, ctx, x, y, z, m, vx, vy, vz, box, groupOffsets, members, numGroups, carries, out,
                                        partials, sortedLabels);
    arenaReset(ctx);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return fail(ctx, CSTONE_E_HIP, "fof_group_properties: %s", hipGetErrorString(e));
    return CSTONE_OK;
}

int fofRunsU64(cstone_hip_ctx* ctx, const uint64_t* keys, uint32_t n, uint64_t limit, uint32_t* work, uint32_t* runStart,
               uint64_t* runLabels, uint32_t host[2])
{
    host[0] = host[1] = 0;
    if (n == 0) return CSTONE_OK;
    uint32_t *heads = work, *runId = work + n, *scal = work + 2 * size_t(n); // scal[0]: numRuns, scal[1]: bad
    CS_TRY(arenaReserve(ctx, scanArenaBytes(n) + 1024));
    int rc = CSTONE_OK;
    if (hipError_t e = hipMemsetAsync(scal, 0, 8, ctx->stream); e != hipSuccess)
        rc = fail(ctx, CSTONE_E_HIP, "fof catalogue: %s", hipGetErrorString(e));
    if (rc == CSTONE_OK)
    {
        hipLaunchKernelGGL(fofpHeads64Kernel, gridFor(n, 256), 256, 0, ctx->stream, keys, n, limit, heads, scal + 1);
        rc = scanU32(ctx, heads, runId, n, 0u, true, scal);
    }
    if (rc == CSTONE_OK)
    {
        hipLaunchKernelGGL(fofpRunStarts64Kernel, gridFor(n, 256), 256, 0, ctx->stream, keys, runId, n, runStart, runLabels);
        rc = copyToHost(ctx, host, scal, 8);
    }
    arenaReset(ctx);
    return rc;
}

void fofPartialLabels(cstone_hip_ctx* ctx, const FofPartial* records, uint32_t n, uint64_t* keys)
{
    if (n) hipLaunchKernelGGL(fofpLabelsKernel, gridFor(n, 256), 256, 0, ctx->stream, records, n, keys);
}

int fofCombinePartials(cstone_hip_ctx* ctx, int realBits, const void* x, const void* y, const void* z, const cstone_box& box,
                       const FofPartial* records, const uint32_t* order, const uint32_t* runStart, uint32_t numRuns,
                       uint64_t firstId, uint32_t first, uint32_t numOwn, uint64_t minMembers, FofPartial* combined,
                       uint32_t* keep)
{
    if (numRuns == 0) return CSTONE_OK;
    if (realBits == 32)
        hipLaunchKernelGGL((fofpCombineKernel<float>), gridFor(numRuns, 256), 256, 0, ctx->stream, (const float*)x,
                           (const float*)y, (const float*)z, cstone_hip::makeDeviceBox<float>(box), records, order, runStart,
                           numRuns, firstId, first, numOwn, minMembers, combined, keep, ctx->devScalars + 63);
    else
        hipLaunchKernelGGL((fofpCombineKernel<double>), gridFor(numRuns, 256), 256, 0, ctx->stream, (const double*)x,
                           (const double*)y, (const double*)z, cstone_hip::makeDeviceBox<double>(box), records, order, runStart,
                           numRuns, firstId, first, numOwn, minMembers, combined, keep, ctx->devScalars + 63);
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

int fofFinishCombined(cstone_hip_ctx* ctx, int realBits, bool velocities, const cstone_box& box, const FofPartial* combined,
                      const uint32_t* keep, const uint32_t* pos, uint32_t numRuns, const FofGroupOut& out)
{
    if (numRuns == 0) return CSTONE_OK;
    if (realBits == 32)
        hipLaunchKernelGGL((fofpFinishKernel<float>), gridFor(numRuns, 256), 256, 0, ctx->stream,
                           cstone_hip::makeDeviceBox<float>(box), velocities, combined, keep, pos, numRuns, out);
    else
        hipLaunchKernelGGL((fofpFinishKernel<double>), gridFor(numRuns, 256), 256, 0, ctx->stream,
                           cstone_hip::makeDeviceBox<double>(box), velocities, combined, keep, pos, numRuns, out);
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

} // namespace cship

using namespace cship;

extern "C" int cstone_hip_fof_group_properties(cstone_hip_ctx* ctx, int real_bits, int mass_bits, const void* x, const void* y,
                                               const void* z, const void* m, const void* vx, const void* vy, const void* vz,
                                               const cstone_box* box_host, const uint32_t* group_offsets,
                                               const uint32_t* members, uint32_t num_groups, void* mass, void* center,
                                               void* velocity, void* radius, uint32_t* flags)
{
    if (!ctx) return fail(ctx, CSTONE_E_ARG, "fof_group_properties: no context");
    if ((real_bits != 32 && real_bits != 64) || (mass_bits != 32 && mass_bits != 64))
        return fail(ctx, CSTONE_E_ARG, "fof_group_properties: real_bits %d, mass_bits %d unsupported", real_bits, mass_bits);
    const int nv = (vx ? 1 : 0) + (vy ? 1 : 0) + (vz ? 1 : 0);
    if (nv != 0 && nv != 3) return fail(ctx, CSTONE_E_ARG, "fof_group_properties: vx, vy, vz: all three or none");
    if (nv == 3 && !velocity) return fail(ctx, CSTONE_E_ARG, "fof_group_properties: velocities given without a velocity output");
    if (num_groups == 0) return CSTONE_OK;
    if (!x || !y || !z || !m || !box_host || !group_offsets || !members || !mass || !center)
        return fail(ctx, CSTONE_E_ARG, "fof_group_properties: null pointer");
    const FofGroupOut out{mass, center, velocity, radius, flags, nullptr, nullptr};
    return fofPropsReduce(ctx, real_bits, mass_bits, x, y, z, m, vx, vy, vz, *box_host, group_offsets, members, num_groups, out,
                          nullptr, nullptr);
}
