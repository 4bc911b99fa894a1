// Incremental re-sort of Domain::sync: leaf table, mover binning and the leaf pass (see resort.hpp for the scheme).
// Replaces, for a sync whose particles mostly stayed in their leaves, the reference's full sort of all keys
// (sortByKeyGpu, R/primitives/primitives_gpu.cu:305-353).  gfx950: wave64, 160 KB LDS per CU.
#include <cstdlib>
#include <type_traits>

#include "device_keys.hpp"
#include "leaf_steps.hpp"
#include "resort.hpp"
#include "scan.hpp"
#include "wave_lanes.hpp"

namespace cship
{
// CSTONE_RESORT_TRACE (tuning builds only, tools/leafpass_trace.py): thread 0 of every workgroup of the leaf pass for
// tiles with movers records wall-clock stamps (100 MHz) at its phase boundaries
#ifdef CSTONE_RESORT_TRACE
constexpr int RESORT_TRACE_SLOTS = 12;
__device__ uint64_t* g_resortTrace;
#define RESORT_TRACE(slot)                                                                                             \
    if (g_resortTrace && threadIdx.x == 0) g_resortTrace[size_t(blockIdx.x) * RESORT_TRACE_SLOTS + (slot)] = wall_clock64();
#else
#define RESORT_TRACE(slot)
#endif
namespace
{

/*! Leaf-start bitmask without atomics: bit p of mask is set when a non-empty leaf starts at position p.  The thread of
 *  the first non-empty leaf that starts inside a 64-position word builds that word from the leaves that follow (a leaf
 *  holds a few dozen particles: one or two starts per word), clears the words between the previous start and its own
 *  and stores the words' bit counts for the rank scan.  The thread of the last non-empty leaf also clears the tail. */
__global__ __launch_bounds__(256) void leafStartWordsKernel(const uint32_t* __restrict__ layout, int numLeaves,
                                                            uint32_t n, uint64_t* __restrict__ mask,
                                                            uint32_t* __restrict__ bits, uint32_t words)
{
    int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= numLeaves) return;
    const uint32_t a = layout[l];
    if (layout[l + 1] <= a) return; // empty
    const uint32_t w = a >> 6;
    // the previous non-empty leaf (empty ones in between start at a as well)
    int prev = l - 1;
    while (prev >= 0 && layout[prev] == a)
        --prev;
    const bool first = prev < 0;
    if (!first && (layout[prev] >> 6) == w) return; // not the first start inside this word
    uint64_t word = 0;
    uint32_t pos  = a;
    int m         = l;
    while (m < numLeaves && (pos >> 6) == w)
    {
        if (layout[m + 1] > pos) word |= 1ull << (pos & 63u);
        ++m;
        pos = m < numLeaves ? layout[m] : n;
        // (empty leaves repeat the position of their successor: the bit is set once, by the non-empty one)
    }
    mask[w] = word;
    bits[w] = uint32_t(__popcll(word));
    for (uint32_t v = first ? 0u : (layout[prev] >> 6) + 1; v < w; ++v)
        mask[v] = 0, bits[v] = 0;
    if (m >= numLeaves || pos >= n)
    {
        // nothing starts behind this word
        for (uint32_t v = w + 1; v < words; ++v)
            mask[v] = 0, bits[v] = 0;
    }
}

//! the j-th non-empty leaf: first key (0 for the first one: keys in front of it belong to it) and first position;
//! entries J and J + 1 close the table: keys from endKey on (the remove markers) form a leaf of their own without positions
template<class K>
__global__ __launch_bounds__(256) void fillCompactLeavesKernel(const K* __restrict__ tree,
                                                               const uint32_t* __restrict__ layout, int numLeaves,
                                                               const uint64_t* __restrict__ mask,
                                                               const uint32_t* __restrict__ rank,
                                                               const uint32_t* __restrict__ numCompact, uint32_t n,
                                                               K* __restrict__ leafLo, uint32_t* __restrict__ leafPos,
                                                               uint32_t* __restrict__ outCount,
                                                               uint32_t* __restrict__ incoming)
{
    int l = blockIdx.x * 256 + threadIdx.x;
    if (l < numLeaves + 3) outCount[l] = 0, incoming[l] = 0; // the departure / arrival counters of this sync
    if (l == 0)
    {
        uint32_t J     = *numCompact;
        leafLo[J]      = endKey<K>();
        leafLo[J + 1]  = ~K(0);
        leafPos[J]     = n;
        leafPos[J + 1] = n;
    }
    if (l >= numLeaves) return;
    uint32_t a = layout[l], b = layout[l + 1];
    if (b <= a) return;
    uint32_t j = rank[a >> 6] + uint32_t(__popcll(mask[a >> 6] & ((1ull << (a & 63u)) - 1)));
    leafLo[j]  = j == 0 ? K(0) : tree[l];
    leafPos[j] = a;
}

//! coarse[c] = last leaf j with leafLo[j] <= c << RESORT_COARSE_SHIFT, for the 2^RESORT_COARSE_BITS + 1 values of c that
//! keys have in their leading bits: the search for a mover's leaf then starts from a handful of candidates
template<class K>
__global__ __launch_bounds__(256) void coarseLeafTableKernel(const K* __restrict__ leafLo,
                                                             const uint32_t* __restrict__ numCompact,
                                                             uint32_t* __restrict__ coarse)
{
    constexpr int shift = 3 * int(maxLevel<K>()) - RESORT_COARSE_BITS;
    const uint32_t c    = blockIdx.x * 256 + threadIdx.x;
    if (c > (1u << RESORT_COARSE_BITS)) return;
    const K key      = K(c) << shift; // c = 2^bits: endKey, the markers' entry
    const uint32_t J = *numCompact;
    uint32_t lo = 0, hi = J + 1;
    while (hi - lo > 1)
    {
        uint32_t mid = (lo + hi) / 2;
        if (leafLo[mid] <= key) lo = mid;
        else hi = mid;
    }
    coarse[c] = lo;
}

//! leaf of a mover's new key, its slot among the movers arriving there
template<class K>
__global__ __launch_bounds__(256) void binMoversKernel(const K* __restrict__ moverKeys,
                                                       const uint32_t* __restrict__ moverCount, uint32_t moverCap,
                                                       const K* __restrict__ leafLo,
                                                       const uint32_t* __restrict__ numCompact,
                                                       const uint32_t* __restrict__ coarse,
                                                       uint32_t* __restrict__ incoming, uint32_t* __restrict__ dest,
                                                       uint32_t* __restrict__ slot)
{
    const uint32_t M = *moverCount;
    if (M > moverCap) return; // list incomplete: the caller falls back
    const uint32_t J = *numCompact;
    for (uint32_t m = blockIdx.x * 256 + threadIdx.x; m < M; m += gridDim.x * 256)
    {
        const K key = moverKeys[m];
        // last j in [0, J] with leafLo[j] <= key (leafLo[0] = 0)
        uint32_t lo = 0, hi = J + 1;
        if (coarse)
        {
            // the leaves of the key's coarse cell: from the last leaf at or before the cell's first key to the last one
            // at or before the next cell's
            constexpr int shift = 3 * int(maxLevel<K>()) - RESORT_COARSE_BITS;
            const uint32_t c    = uint32_t(key >> shift); // (a marker: 2^bits)
            lo                  = coarse[c];
            hi                  = c < (1u << RESORT_COARSE_BITS) ? coarse[c + 1] + 1 : J + 1;
        }
        while (hi - lo > 1)
        {
            uint32_t mid = (lo + hi) / 2;
            if (leafLo[mid] <= key) lo = mid;
            else hi = mid;
        }
        dest[m] = lo;
        slot[m] = atomicAdd(&incoming[lo], 1u);
    }
}

//! size of every leaf after the moves; [1] |= 1: a leaf too long for the leaf pass
__global__ __launch_bounds__(256) void newLeafSizesKernel(const uint32_t* __restrict__ leafPos,
                                                          const uint32_t* __restrict__ outCount,
                                                          const uint32_t* __restrict__ incoming,
                                                          const uint32_t* __restrict__ numCompact, uint32_t entries,
                                                          uint32_t* __restrict__ newCount, int* __restrict__ scalars)
{
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= entries) return;
    const uint32_t J = *numCompact;
    uint32_t c       = 0;
    if (j <= J)
    {
        uint32_t old = j < J ? leafPos[j + 1] - leafPos[j] : 0u;
        c            = old - outCount[j] + incoming[j];
        // (entry J, the remove markers, does not go through the leaf pass)
        // (slot numbers 0 .. RESORT_LEAF_CAP - 2 only: the digest of slot 255 behind 24 set key bits would equal the
        //  hole's ~0u)
        if (j < J && old + incoming[j] >= RESORT_LEAF_CAP) atomicOr(&scalars[1], 1);
    }
    newCount[j] = c;
}

//! [1] |= 2: the leaves of a workgroup of the leaf pass need more LDS slots than it has, |= 4: mover list overflow,
//! |= 8 (no failure): a large quiet tile; [0]: particles carrying the remove marker
__global__ __launch_bounds__(256) void checkTilesKernel(const uint32_t* __restrict__ leafPos,
                                                        const uint32_t* __restrict__ inOffset,
                                                        const uint32_t* __restrict__ layoutNew,
                                                        const uint32_t* __restrict__ numCompact,
                                                        const uint32_t* __restrict__ moverCount, uint32_t moverCap,
                                                        int leavesPerTile, int* __restrict__ scalars)
{
    const uint32_t J = *numCompact;
    uint32_t t       = blockIdx.x * 256 + threadIdx.x;
    if (t == 0)
    {
        scalars[0] = int(inOffset[J + 1] - inOffset[J]);
        if (*moverCount > moverCap) atomicOr(&scalars[1], 4);
    }
    uint32_t j0 = t * uint32_t(leavesPerTile);
    if (j0 >= J) return;
    uint32_t j1    = min(j0 + uint32_t(leavesPerTile), J);
    const uint32_t old = leafPos[j1] - leafPos[j0], arrivals = inOffset[j1] - inOffset[j0];
    if (old + arrivals > RESORT_TILE_SLOTS) atomicOr(&scalars[1], 2);
    // a tile in which nothing moved but with more slots than the quiet-tile kernel of the leaf pass has: the wave
    // kernel has to be launched for it even without movers
    if (arrivals == 0 && layoutNew[j1] - layoutNew[j0] == old && old > RESORT_QUIET_SLOTS) atomicOr(&scalars[1], 8);
}

template<class K>
__global__ __launch_bounds__(256) void placeMoversKernel(const K* __restrict__ moverKeys,
                                                         const uint32_t* __restrict__ moverIdx,
                                                         const uint32_t* __restrict__ dest,
                                                         const uint32_t* __restrict__ slot, uint32_t M,
                                                         const uint32_t* __restrict__ inOffset, K* __restrict__ binKeys,
                                                         uint32_t* __restrict__ binIdx)
{
    uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    uint32_t at = inOffset[dest[m]] + slot[m];
    binKeys[at] = moverKeys[m];
    binIdx[at]  = moverIdx[m];
}

/*! The leaf pass for QUIET tiles.  A workgroup takes G consecutive (non-empty) leaves of the previous sync, a tile.  The
 *  encode pass has replaced the key of every particle that left its leaf by a hole (key ~0, sorts last).  A tile is
 *  quiet when nothing arrived in its leaves and every leaf keeps its size, i.e. nobody left either: the common case of
 *  a region at rest.  Its keys (the old positions of its leaves, as they are) go to LDS with the 16-bit slot they came
 *  from -- up to RESORT_QUIET_SLOTS of them, 39 KB: four workgroups per CU --, one lane per leaf insertion-sorts the
 *  leaf there by (key, old index) -- the particles come in the order of the previous sync, i.e. almost sorted: one LDS
 *  read per element --, and the tile is written back slot by slot to layoutNew[first leaf] ...: ascending keys, ties
 *  by old index = the stable sort.  A workgroup whose tile is not quiet, or quiet but longer than that, leaves after
 *  the vote: leafSortWaveKernel below takes those tiles (same grid, same vote). */
template<class K, int G>
__global__ __launch_bounds__(256) void leafSortKernel(const K* __restrict__ keysIn, const uint32_t* __restrict__ leafPos,
                                                      const uint32_t* __restrict__ inOffset,
                                                      const uint32_t* __restrict__ layoutNew, uint32_t J,
                                                      bool alwaysCount, K* __restrict__ keysOut,
                                                      uint32_t* __restrict__ orderOut)
{
    constexpr int ITER = (RESORT_TILE_SLOTS + 255) / 256;
    __shared__ __attribute__((aligned(8))) K sKey[RESORT_QUIET_SLOTS]; // the keys ...
    __shared__ uint16_t sIdx[RESORT_QUIET_SLOTS];                      // ... and the slots of the tile they came from
    __shared__ uint32_t posK[G + 1], inK[G + 1], outK[G + 1];

    const uint32_t j0 = blockIdx.x * uint32_t(G);
    const uint32_t nl = min(uint32_t(G), J - j0);
    const uint32_t t  = threadIdx.x;
    if (t <= nl)
    {
        posK[t] = leafPos[j0 + t];
        inK[t]  = inOffset[j0 + t];
        outK[t] = layoutNew[j0 + t];
    }
    __syncthreads();
    const uint32_t p0 = posK[0], p1 = posK[nl], in0 = inK[0], in1 = inK[nl];
    const uint32_t nOldAll = p1 - p0, slots = nOldAll + (in1 - in0);
    // guarded by checkTilesKernel: a launch only happens when every workgroup fits
    if (slots > RESORT_TILE_SLOTS) return;
    // quiet tile: no arrivals, and every leaf keeps its size (without arrivals: nobody left)
    bool changed = in1 != in0 || alwaysCount;
    if (t < nl) changed = changed || (outK[t + 1] - outK[t]) != (posK[t + 1] - posK[t]);
    // (a quiet tile beyond RESORT_QUIET_SLOTS goes the other way as well: the wave kernel holds no keys in LDS)
    const bool quiet = !__syncthreads_or(changed) && nOldAll <= RESORT_QUIET_SLOTS;
    if (!quiet) return;

    // old positions: all loads of a thread are issued before the first is used
    K key[ITER];
#pragma unroll
    for (int i = 0; i < ITER; ++i)
    {
        const uint32_t p = p0 + t + 256u * i;
        if (p < p1) key[i] = keysIn[p];
    }
#pragma unroll
    for (int i = 0; i < ITER; ++i)
    {
        const uint32_t p = p0 + t + 256u * i;
        if (p < p1)
        {
            sKey[p - p0] = key[i];
            sIdx[p - p0] = uint16_t(p - p0);
        }
    }
    __syncthreads();

    if (t < nl)
    {
        const uint32_t s = posK[t] - p0, nOld = posK[t + 1] - posK[t];
        if (nOld > 1)
        {
            const uint32_t e = s + nOld;
            K pk             = sKey[s];
            K nk             = sKey[s + 1];
            for (uint32_t a = s + 1; a < e; ++a)
            {
                const K ka = nk;
                if (a + 1 < e) nk = sKey[a + 1];
                if (ka > pk)
                {
                    pk = ka;
                    continue;
                }
                const uint32_t ia = sIdx[a];
                if (ka == pk && ia > sIdx[a - 1]) continue;
                uint32_t b = a;
                while (b > s)
                {
                    const K kb        = sKey[b - 1];
                    const uint32_t ib = sIdx[b - 1];
                    if (kb < ka || (kb == ka && ib < ia)) break;
                    sKey[b] = kb;
                    sIdx[b] = ib;
                    --b;
                }
                sKey[b] = ka;
                sIdx[b] = ia;
            }
        }
    }
    __syncthreads();
    // every leaf kept its size: slot e of the tile goes to layoutNew[first leaf] + e
    const uint32_t out0 = outK[0];
#pragma unroll
    for (int i = 0; i < ITER; ++i)
    {
        const uint32_t e = t + 256u * i;
        if (e < nOldAll)
        {
            keysOut[out0 + e]  = sKey[e];
            orderOut[out0 + e] = p0 + sIdx[e];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The leaf pass for tiles in which something moved (round 3): ONE WAVE PER LEAF, sorted in registers.
//
// What the phase trace of the earlier formulations showed (tools/leafpass_trace.py, CSTONE_RESORT_TRACE): 25-30 us of a
// tile's 32 us went into its LDS phases -- every element looked its leaf up (six dependent, bank-conflicting reads), took
// a place by a returning atomic, scanned its bucket (or its whole leaf) entry by entry; the LDS pipe of a CU serves four
// such tiles at a time and is what those kernels waited for, whatever the arithmetic around it (counting over the leaf
// 0.97-1.07 ms at 10^8 particles, eight buckets per leaf 0.90-0.95 ms, the same with batched accesses 0.99-1.05 ms, with
// stores staged through LDS 1.03-1.10 ms).
// A leaf of the focus tree holds at most a bucket of particles and a wave has 64 lanes.  So: lane s of a wave loads slot
// s of the leaf (old slots, then the arrivals; coalesced) and builds the 32-bit digest (24 leading bits of key - first
// key of the leaf, then the slot number); the wave sorts the digests with a bitonic network in registers (21
// compare-exchange steps for 64 elements, no search: the leaf is the wave's).  The partners come through DPP inside a
// row of 16 lanes and v_permlane16_swap / v_permlane32_swap across rows, all on the VALU: the same network over
// ds_bpermute was bound by the LDS pipe again (0.95 ms).  The place of every slot in the new order goes back to the lane
// that loaded it through a 16-bit table per wave in LDS (two LDS accesses per element), and that lane stores its key and
// old index at layoutNew[leaf] + place: every key is read once and never leaves its register.  Holes (digest ~0) sort
// last.  Leaves with 65..255 slots take two or four elements per lane.  Two sorted neighbours with equal leading bits
// (equal keys among them; about one leaf in 10^4) send the leaf to the exact path: every element counts the elements
// in front of it by (key, old index) proper.  A leaf nothing arrived in and whose remaining keys are still in order goes
// out as it came in, without the network.
// The loop over the wave's leaves is ROLLED (see below).  What decides a step -- which leaves it takes, how many lanes
// each gets, whether there is anything to sort -- depends on the leaves' slot counts only and is the same for all lanes:
// it is worked out once per tile (leaf_steps.hpp), held one word per leaf in a lane register and taken into scalar
// registers with v_readlane, so the loop counts and branches in scalars.  (Round 3 declared the wave number uniform
// and read the leaf's table entries through readfirstlane instead: every leaf then started with a chain of LDS read ->
// s_waitcnt -> v_readfirstlane -> scalar ALU before its first load could be issued, 0.74 / 0.83 ms against 0.66 /
// 0.75 ms, 1 % movers / everything drifting.  The table entries themselves stay in vector registers here.)
// ---------------------------------------------------------------------------------------------------------------------
// ---- cross-lane partners on the VALU (no LDS pipe): DPP within a row of 16 lanes, v_permlane16/32_swap (gfx950) across
//      rows; lane mappings verified with tools/dpp_probe.hip on the hardware.  dppMov, dppAll and laneXor<X> live in
//      wave_lanes.hpp, which knn.hip shares
//! compare-exchange with the lane at distance X, for N independent registers at once (one step of N sorts: their
//! instructions interleave, which fills the wait states between a VALU write and a DPP read); the lane whose bit LOWBIT
//! is clear is the lower one and keeps the minimum
template<int X, unsigned LOWBIT, int N>
__device__ __forceinline__ void cmpExchange(uint32_t (&v)[N], unsigned lane)
{
    if constexpr ((X == 4 || X == 8) && LOWBIT == unsigned(X))
    {
        // the lower lanes of such a step are whole DPP banks (four lanes each): the minimum goes to them through a masked
        // row_shl, the maximum to the upper banks through a masked row_shr of the ORIGINAL values; lanes outside a mask
        // keep their operand (old), so no select is needed -- four instructions (two when the moves fold) instead of five
#pragma unroll
        for (int n = 0; n < N; ++n)
        {
            const uint32_t a = v[n];
            uint32_t r       = a;
            // (written as instructions: the compiler does not fold a masked DPP move into its consumer.  s_nop 1: a DPP
            //  operand written by the instruction before needs two wait states, and the assembler text hides the DPP
            //  from the compiler's hazard pass)
            if constexpr (X == 4)
            {
                asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %1, %0 row_shl:4 row_mask:0xf bank_mask:0x5" : "+v"(r) : "v"(a));
                asm volatile("v_max_u32_dpp %0, %1, %0 row_shr:4 row_mask:0xf bank_mask:0xa" : "+v"(r) : "v"(a));
            }
            else
            {
                asm volatile("s_nop 1\n\tv_min_u32_dpp %0, %1, %0 row_shl:8 row_mask:0xf bank_mask:0x3" : "+v"(r) : "v"(a));
                asm volatile("v_max_u32_dpp %0, %1, %0 row_shr:8 row_mask:0xf bank_mask:0xc" : "+v"(r) : "v"(a));
            }
            v[n] = r;
        }
        return;
    }
    const bool upper = (lane & LOWBIT) != 0;
#pragma unroll
    for (int n = 0; n < N; ++n)
    {
        const uint32_t o = laneXor<X>(v[n], lane);
        v[n]             = upper ? max(v[n], o) : min(v[n], o);
    }
}

//! the half-cleaners behind a merge step: distances J, J/2, ... 1
template<int J, int N>
__device__ __forceinline__ void halfClean(uint32_t (&v)[N], unsigned lane)
{
    if constexpr (J >= 1)
    {
        cmpExchange<J, unsigned(J), N>(v, lane);
        halfClean<J / 2, N>(v, lane);
    }
}

/*! N independent ascending sorts of 64 values each (register n of every lane: one sort): bitonic network without
 *  direction flags -- every merge of two sorted blocks starts with a compare-exchange against the MIRRORED position
 *  (distance k - 1), followed by half-cleaners at distances k/4 ... 1, the lower lane always keeps the minimum. */
template<int N>
__device__ __forceinline__ void waveSort64(uint32_t (&v)[N], unsigned lane)
{
    cmpExchange<1, 1u, N>(v, lane);                              // blocks of 2
    cmpExchange<3, 2u, N>(v, lane), halfClean<1, N>(v, lane);    // 4
    cmpExchange<7, 4u, N>(v, lane), halfClean<2, N>(v, lane);    // 8
    cmpExchange<15, 8u, N>(v, lane), halfClean<4, N>(v, lane);   // 16
    cmpExchange<31, 16u, N>(v, lane), halfClean<8, N>(v, lane);  // 32
    cmpExchange<63, 32u, N>(v, lane), halfClean<16, N>(v, lane); // 64
}

//! ascending sort of the 64 R values d[r] (element 64 r + lane) of a wave
template<int R>
__device__ __forceinline__ void waveBitonicSort(uint32_t (&d)[R], unsigned lane)
{
    waveSort64<R>(d, lane);
    if constexpr (R >= 2)
    {
        // blocks of 128: element (r, lane) against (r ^ 1, 63 - lane)
#pragma unroll
        for (int r = 0; r < R; r += 2)
        {
            const uint32_t a = d[r], b = d[r + 1];
            d[r]     = min(a, laneXor<63>(b, lane));
            d[r + 1] = max(b, laneXor<63>(a, lane));
        }
        halfClean<32, R>(d, lane);
    }
    if constexpr (R == 4)
    {
        // blocks of 256: (r, lane) against (3 - r, 63 - lane), then distance 64 (registers r, r ^ 1), then within registers
        const uint32_t a0 = d[0], a1 = d[1], a2 = d[2], a3 = d[3];
        d[0] = min(a0, laneXor<63>(a3, lane)), d[3] = max(a3, laneXor<63>(a0, lane));
        d[1] = min(a1, laneXor<63>(a2, lane)), d[2] = max(a2, laneXor<63>(a1, lane));
        const uint32_t b0 = d[0], b1 = d[1], b2 = d[2], b3 = d[3];
        d[0] = min(b0, b1), d[1] = max(b0, b1), d[2] = min(b2, b3), d[3] = max(b2, b3);
        halfClean<32, R>(d, lane);
    }
}

// ---- two elements per lane: lane l of a segment holds the elements 2 l (register 0) and 2 l + 1 (register 1) of its
//      leaf, so that a leaf of up to 64 slots takes HALF a wave and a wave step sorts two leaves (or four of up to 32
//      slots).  Six of the 21 steps of the 64-element network are then compare-exchanges inside a lane (two
//      instructions for both registers, no cross-lane move, no select), the others run on both registers at half the
//      lane distance.
__device__ __forceinline__ void inLaneExchange(uint32_t (&d)[2])
{
    const uint32_t lo = min(d[0], d[1]);
    d[1]              = max(d[0], d[1]);
    d[0]              = lo;
}
//! first step of the merge of two sorted blocks of K/2 elements each: element e against the mirrored element
//! e ^ (K - 1), i.e. (lane, register) against (lane ^ M, other register), M = K/2 - 1; LOWBIT = K/4 in lane space
template<int M, unsigned LOWBIT>
__device__ __forceinline__ void mirrorExchange(uint32_t (&d)[2], unsigned lane)
{
    const uint32_t o1 = laneXor<M>(d[1], lane), o0 = laneXor<M>(d[0], lane);
    const bool upper  = (lane & LOWBIT) != 0;
    d[0]              = upper ? max(d[0], o1) : min(d[0], o1);
    d[1]              = upper ? max(d[1], o0) : min(d[1], o0);
}
//! ascending sort of the 2 * SEG elements of every segment of SEG lanes (SEG = 32: 64 elements, SEG = 16: 32)
template<int SEG>
__device__ __forceinline__ void pairSort(uint32_t (&d)[2], unsigned lane)
{
    inLaneExchange(d);                                                                       // blocks of 2
    mirrorExchange<1, 1u>(d, lane), inLaneExchange(d);                                       // 4
    mirrorExchange<3, 2u>(d, lane), cmpExchange<1, 1u, 2>(d, lane), inLaneExchange(d);       // 8
    mirrorExchange<7, 4u>(d, lane), halfClean<2, 2>(d, lane), inLaneExchange(d);             // 16
    mirrorExchange<15, 8u>(d, lane), halfClean<4, 2>(d, lane), inLaneExchange(d);            // 32
    if constexpr (SEG >= 32) { mirrorExchange<31, 16u>(d, lane), halfClean<8, 2>(d, lane), inLaneExchange(d); } // 64
}

template<class K, int G, int MODE>
__global__ __launch_bounds__(256) void leafSortWaveKernel(
    const K* __restrict__ keysIn, const K* __restrict__ leafLo, const uint32_t* __restrict__ leafPos,
    const uint32_t* __restrict__ inOffset, const uint32_t* __restrict__ layoutNew, const K* __restrict__ binKeys,
    const uint32_t* __restrict__ binIdx, uint32_t J, bool alwaysCount, bool allTiles, K* __restrict__ keysOut,
    uint32_t* __restrict__ orderOut)
{
    constexpr K HOLE = ~K(0);
    //! what a step reads of a leaf, written once per tile: one record, two or three wide LDS reads
    struct alignas(16) LeafRec
    {
        uint32_t pk, nOld, ik, nInc, ok, nNew, cut; // old slots, arrivals (in the bins), new content; shift of the digest
        K lo;
    };
    __shared__ LeafRec recK[G + 1];    // [G]: no leaf -- nothing old, nothing arriving, nothing to store
    __shared__ uint32_t slotsK[G + 4]; // old slots + arrivals of every leaf, zeros behind the last one
    __shared__ uint16_t sPlace[4][256];

    RESORT_TRACE(0)
    const uint32_t j0 = blockIdx.x * uint32_t(G);
    const uint32_t nl = min(uint32_t(G), J - j0);
    const uint32_t t  = threadIdx.x;
    uint32_t slots = 0, nOld = 0, nNew = 0;
    if (t < nl)
    {
        LeafRec r;
        r.pk = leafPos[j0 + t], r.nOld = nOld = leafPos[j0 + t + 1] - r.pk;
        r.ik = inOffset[j0 + t], r.nInc = inOffset[j0 + t + 1] - r.ik;
        r.ok = layoutNew[j0 + t], r.nNew = nNew = layoutNew[j0 + t + 1] - r.ok;
        r.lo = leafLo[j0 + t];
        // how far a leaf's keys are shifted for the 24 leading bits of the digest: once per leaf here, not once per step
        const K span   = leafLo[j0 + t + 1] - r.lo - 1;
        const int bits = span ? int(8 * sizeof(K)) - clzKey(span) : 0;
        r.cut          = uint32_t(bits > 24 ? bits - 24 : 0);
        recK[t]        = r;
        slots          = r.nOld + r.nInc;
    }
    else if (t == uint32_t(G)) { recK[G] = LeafRec{0, 0, 0, 0, 0, 0, 0, 0}; }
    if (t < uint32_t(G) + 4u) slotsK[t] = slots;
    if (!allTiles)
    {
        // leafSortKernel takes the tiles in which nothing moved (same vote as there)
        const uint32_t nOldAll = leafPos[j0 + nl] - leafPos[j0];
        const bool changed     = inOffset[j0 + nl] != inOffset[j0] || alwaysCount || nNew != nOld;
        const bool quiet       = !__syncthreads_or(changed) && nOldAll <= RESORT_QUIET_SLOTS;
        if (quiet) return;
    }
    __syncthreads(); // (recK, slotsK)
    const unsigned lane = t & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(t >> 6); // (once per tile: the loops below count in scalars)

    //! what the loop needs to know about leaf k
    struct Leaf
    {
        uint32_t pk, nOld, ik, nInc, ok, nNew, slots;
        K lo;
        unsigned cut;
    };
    auto leafOf = [&](uint32_t k)
    {
        const LeafRec r = recK[k];
        Leaf f;
        f.pk = r.pk, f.nOld = r.nOld, f.ik = r.ik, f.nInc = r.nInc, f.ok = r.ok, f.nNew = r.nNew;
        f.slots = r.nOld + r.nInc;
        f.lo    = r.lo;
        f.cut   = r.cut;
        return f;
    };
    // slot s of a leaf: an old position or an arrival (key and old position; requested one wave step ahead).  Without a
    // branch: one address per array, chosen between the old slot and the bin entry, and one load under the lane's
    // condition; a lane without a leaf (recK[G]) loads nothing
    auto loadSlot = [&](const Leaf& f, uint32_t s, K& key, uint32_t& idx)
    {
        const bool old = s < f.nOld, have = s < f.slots;
        const uint32_t at = old ? f.pk + s : f.ik + (s - f.nOld);
        const K* src      = old ? keysIn : binKeys;
        key = HOLE, idx = old ? at : 0u;
        if (have) key = src[at];
        if (have && !old) idx = binIdx[at];
    };
    // the values requested for the NEXT step are pinned (an empty asm that "uses" them) before the stores of this step go
    // out: the compiler then waits for those loads HERE, where they have had the whole step to return, instead of at the
    // top of the next step behind this step's stores -- vmcnt counts loads and stores in one in-order queue, and a wait
    // placed there has to cover the path of the loop that stores nothing, i.e. it waits for the stores as well
    auto pinNext = [&](K& key, uint32_t& idx) { asm volatile("" : "+v"(key), "+v"(idx)); };
    auto storeAt = [&](uint32_t at, K key, uint32_t idx)
    {
        keysOut[at]  = key;
        orderOut[at] = idx;
    };
    auto digestOf = [&](const Leaf& f, K key, uint32_t slot) -> uint32_t
    { return key == HOLE ? ~0u : ((uint32_t((key - f.lo) >> f.cut) << 8) | slot); };

    // the sorted digests of a leaf -> its new content: the place of every slot in the new order goes back to the lane that
    // loaded the slot (and still holds its key) through a 16-bit table per wave in LDS, two LDS accesses per element; that
    // lane stores key and old index at layoutNew[leaf] + place.  false: two neighbours in the new order have equal leading
    // key bits (the caller then places the leaf by keys and old indices proper)
    auto finishLeaf = [&](const Leaf& f, auto rTag, const K* key, const uint32_t* idx, uint32_t* d) -> bool
    {
        constexpr int R = decltype(rTag)::value;
        bool clash      = false;
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            // the element in front: the lane below, for lane 0 the last lane of the register before (all lanes shuffle)
            const uint32_t below = uint32_t(__shfl_up(int(d[r]), 1));
            const uint32_t last  = R > 1 ? uint32_t(__shfl(int(d[r > 0 ? r - 1 : 0]), 63)) : ~0u;
            const uint32_t prev  = lane != 0 ? below : (r > 0 ? last : ~0u);
            clash = clash || (d[r] != ~0u && prev != ~0u && (d[r] >> 8) == (prev >> 8));
        }
        if (__any(clash)) return false;
        uint16_t* place = sPlace[wave];
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (d[r] != ~0u) place[d[r] & 0xFFu] = uint16_t(lane + 64u * r);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            if (key[r] == HOLE) continue;
            const uint32_t at = place[lane + 64u * r];
            if (at < f.nNew) storeAt(f.ok + at, key[r], idx[r]);
        }
        __builtin_amdgcn_wave_barrier();
        return true;
    };
    // exact path: every loaded element counts the elements of its leaf in front of it by (key, old index)
    auto exactLeaf = [&](const Leaf& f, int R, const K* key, const uint32_t* idx)
    {
        for (int r = 0; r < R; ++r)
        {
            if (key[r] == HOLE) continue;
            uint32_t less = 0;
            for (uint32_t q = 0; q < f.nOld; ++q)
            {
                const K kq = keysIn[f.pk + q]; // (a hole is larger than any key)
                less += (kq < key[r] || (kq == key[r] && f.pk + q < idx[r])) ? 1u : 0u;
            }
            for (uint32_t q = 0; q < f.nInc; ++q)
            {
                const K kq = binKeys[f.ik + q];
                less += (kq < key[r] || (kq == key[r] && binIdx[f.ik + q] < idx[r])) ? 1u : 0u;
            }
            storeAt(f.ok + less, key[r], idx[r]);
        }
    };
    auto bigLeaf = [&](const Leaf& f, auto rTag)
    {
        constexpr int R = decltype(rTag)::value;
        K key[R];
        uint32_t idx[R], d[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            loadSlot(f, lane + 64u * r, key[r], idx[r]);
            d[r] = digestOf(f, key[r], lane + 64u * r);
        }
        waveBitonicSort<R>(d, lane);
        if (!finishLeaf(f, rTag, key, idx, d)) exactLeaf(f, R, key, idx);
    };

    if constexpr (MODE == 0)
    {
        // The leaves of this wave: wave, wave + 4, ...  A ROLLED loop: the body (load, 64-element network, store) is a few
        // hundred instructions and stays in the instruction cache; unrolled over the wave's 16 leaves the kernel was
        // 24-41 thousand instructions (190-330 KB of code streaming through the instruction cache) and took 0.7-0.9 ms
        // whatever the network cost.  The key of the NEXT leaf is requested before the current one is sorted.
        // What kind of step a leaf takes follows from its slots: lane l holds those of the wave's l-th leaf, and the loop
        // takes them from there into a scalar (v_readlane), so that it counts and branches in scalars without waiting
        // for the leaf's record in front of every branch.
        if (wave >= nl) return;
        const uint32_t numSteps = (nl - wave + 3u) / 4u; // (at most G / 4 = 16)
        const uint32_t slotsOf  = lane < numSteps ? slotsK[wave + 4u * lane] : 0u;
        Leaf cur        = leafOf(wave);
        uint32_t slotsN = __builtin_amdgcn_readlane(slotsOf, 0);
        K keyN          = HOLE;
        uint32_t idxN   = 0;
        if (slotsN <= 64) loadSlot(cur, lane, keyN, idxN);
    #pragma unroll 1
        for (uint32_t s = 0; s < numSteps; ++s)
        {
            const Leaf f         = cur;
            const uint32_t slots = slotsN;
            K key1[1]            = {keyN};
            uint32_t idx1[1]     = {idxN};
            keyN = HOLE, idxN = 0;
            if (s + 1 < numSteps)
            {
                cur    = leafOf(wave + 4u * (s + 1));
                slotsN = __builtin_amdgcn_readlane(slotsOf, s + 1);
                if (slotsN <= 64) loadSlot(cur, lane, keyN, idxN);
            }
            if (slots == 0) continue;
            if (slots <= 64)
            {
                // nothing arrived and what stayed is still in order (a departure leaves the largest key behind, so only
                // departures from the end of the leaf pass): the content goes out as it came in
                {
                    const K below     = K(__shfl_up((unsigned long long)key1[0], 1));
                    const bool behind = lane != 0 && key1[0] < below;
                    if (f.nInc == 0 && !__any(behind))
                    {
                        pinNext(keyN, idxN);
                        if (lane < f.nNew) storeAt(f.ok + lane, key1[0], idx1[0]);
                        continue;
                    }
                }
                uint32_t d[1] = {digestOf(f, key1[0], lane)};
                waveBitonicSort<1>(d, lane);
                pinNext(keyN, idxN);
                if (!finishLeaf(f, std::integral_constant<int, 1>{}, key1, idx1, d)) exactLeaf(f, 1, key1, idx1);
            }
            else if (slots <= 128) { bigLeaf(f, std::integral_constant<int, 2>{}); }
            else { bigLeaf(f, std::integral_constant<int, 4>{}); }
        }
        return;
    }
    if constexpr (MODE == 1)
    {
        // ---- two elements per lane (see pairSort): a step takes TWO consecutive leaves of up to 64 slots (a segment of
        //      32 lanes each) or FOUR of up to 32 slots (16 lanes each); a leaf with more than 64 slots has the wave
        //      to itself as in the other flavours.  The wave's leaves: a contiguous quarter of the tile.
#ifdef CSTONE_RESORT_TRACE
        RESORT_TRACE(1)
        long long trSteps = 0, trIssue = 0, trWait = 0, trSort = 0, trFinish = 0, trT = clock64();
#define WAVE_TRACE(acc)                                                                                                \
    {                                                                                                                  \
        const long long now_ = clock64();                                                                              \
        acc += now_ - trT;                                                                                             \
        trT = now_;                                                                                                    \
    }
#else
#define WAVE_TRACE(acc)
#endif
        const uint32_t per    = (nl + 3u) / 4u;
        const uint32_t kBegin = min(nl, wave * per), kEnd = min(nl, kBegin + per);
        if (kBegin >= kEnd) return;
        const uint32_t n = kEnd - kBegin; // leaves of this wave's quarter: 1 ... G / 4 = 16
        // The step plan (leaf_steps.hpp), once per tile: lane l holds the step that starts at leaf l of the quarter.  The
        // loop takes the word of its step into a scalar (v_readlane) and the next step starts behind the leaves this one
        // consumes, so everything that decides a step -- its first leaf, the segment size, the kind -- lives in scalar
        // registers, and no LDS read stands in front of a branch.
        uint32_t stepOf = 0;
        if (lane < n)
        {
            const uint32_t* s = slotsK + kBegin + lane;
            stepOf            = leafStepAt(lane, n - lane, s[0], s[1], s[2], s[3]);
        }
        // the leaf of this lane in the step `word` (none: the zero record recK[G], so is every lane with on == false or in a
        // step of one long leaf, which bigLeaf loads itself) and the request for the lane's two slots
        auto requestStep = [&](uint32_t word, bool on, Leaf& f, K (&key)[2], uint32_t (&idx)[2])
        {
            const uint32_t bits = leafStepBits(word);
            const uint32_t seg  = lane >> bits;
            const bool mine     = on && bits != 6u && seg < leafStepLeaves(word);
            const uint32_t kk   = kBegin + leafStepFirst(word) + seg;
            f                   = leafOf(mine ? kk : uint32_t(G));
            const uint32_t sl   = lane & ((1u << bits) - 1u);
            loadSlot(f, 2 * sl, key[0], idx[0]);
            loadSlot(f, 2 * sl + 1, key[1], idx[1]);
        };
        uint32_t q     = 0; // leaves of the quarter the steps so far have consumed
        uint32_t wordN = __builtin_amdgcn_readlane(stepOf, 0);
        bool more      = true;
        Leaf cur;
        K keyN[2];
        uint32_t idxN[2];
        requestStep(wordN, true, cur, keyN, idxN);
        // (a counted loop: a step consumes at least one leaf, so n steps are enough whatever the plan says)
#pragma unroll 1
        for (uint32_t step = 0; step < n && more; ++step)
        {
            const uint32_t word   = wordN;
            const Leaf f          = cur;
            const unsigned b      = leafStepBits(word);
            const K key[2]        = {keyN[0], keyN[1]};
            const uint32_t idx[2] = {idxN[0], idxN[1]};
            const uint32_t sl     = lane & ((1u << (b == 6 ? 5u : b)) - 1u);
            q += leafStepLeaves(word);
            more  = q < n;
            wordN = __builtin_amdgcn_readlane(stepOf, more ? q : 0u);
            requestStep(wordN, more, cur, keyN, idxN);
#ifdef CSTONE_RESORT_TRACE
            ++trSteps;
            WAVE_TRACE(trIssue)
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); // (the keys of this step: all but the loads just issued)
            WAVE_TRACE(trWait)
#endif
            if (b == 6)
            {
                const Leaf g = leafOf(kBegin + leafStepFirst(word));
                if (!leafStepWide(word)) { bigLeaf(g, std::integral_constant<int, 2>{}); }
                else { bigLeaf(g, std::integral_constant<int, 4>{}); }
                continue;
            }
            if (leafStepEmpty(word)) continue;
            // the element in front of (lane, 0) is (lane - 1, 1), the one in front of (lane, 1) is (lane, 0)
            const K front = K(__shfl_up((unsigned long long)key[1], 1));
            // nothing arrived and what stayed is still in order: the content goes out as it came in
            const bool behind = (sl != 0 && key[0] < front) || key[1] < key[0];
            if (!__any(f.nInc != 0 || behind))
            {
                pinNext(keyN[0], idxN[0]);
                pinNext(keyN[1], idxN[1]);
#pragma unroll
                for (int r = 0; r < 2; ++r)
                {
                    if (2 * sl + r < f.nNew) storeAt(f.ok + 2 * sl + r, key[r], idx[r]);
                }
                continue;
            }
            uint32_t d[2] = {digestOf(f, key[0], 2 * sl), digestOf(f, key[1], 2 * sl + 1)};
            if (b == 5) pairSort<32>(d, lane);
            else pairSort<16>(d, lane);
            WAVE_TRACE(trSort)
            pinNext(keyN[0], idxN[0]);
            pinNext(keyN[1], idxN[1]);
            // equal leading bits among neighbours of the new order?  (by segment: ballot masked with the segment's lanes)
            const uint32_t dFront  = uint32_t(__shfl_up(int(d[1]), 1));
            const bool clash0      = sl != 0 && d[0] != ~0u && dFront != ~0u && (d[0] >> 8) == (dFront >> 8);
            const bool clash1      = d[1] != ~0u && d[0] != ~0u && (d[1] >> 8) == (d[0] >> 8);
            const uint64_t clashes = __ballot(clash0 || clash1);
            const unsigned base    = lane - sl; // first lane of my segment
            const uint64_t segment = ((b == 5 ? 0xFFFFFFFFull : 0xFFFFull)) << base;
            const bool exact       = (clashes & segment) != 0;
            uint16_t* place        = sPlace[wave] + 2u * base; // 2 * SEG entries per segment
            if (d[0] != ~0u) place[d[0] & 0xFFu] = uint16_t(2 * sl);
            if (d[1] != ~0u) place[d[1] & 0xFFu] = uint16_t(2 * sl + 1);
            __builtin_amdgcn_wave_barrier();
            if (!exact)
            {
#pragma unroll
                for (int r = 0; r < 2; ++r)
                {
                    if (key[r] == HOLE) continue;
                    const uint32_t at = place[2 * sl + r];
                    if (at < f.nNew) storeAt(f.ok + at, key[r], idx[r]);
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (exact) exactLeaf(f, 2, key, idx);
            WAVE_TRACE(trFinish)
        }
#ifdef CSTONE_RESORT_TRACE
        if (g_resortTrace && threadIdx.x == 0)
        {
            uint64_t* tr = g_resortTrace + size_t(blockIdx.x) * RESORT_TRACE_SLOTS;
            tr[2] = wall_clock64(), tr[3] = uint64_t(trSteps), tr[4] = uint64_t(trIssue), tr[5] = uint64_t(trWait),
            tr[6] = uint64_t(trSort), tr[7] = uint64_t(trFinish);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            tr[8] = wall_clock64();
        }
#endif
#undef WAVE_TRACE
    }
}

/*! Positions of the leaf boundaries of ANOTHER tree (the focus tree after its rebalance) in the keys this re-sort has just
 *  ordered: the leaf table knows where every old leaf starts now (layoutNew), so the search for a boundary key only
 *  covers the particles of the one old leaf whose key range holds it -- a few dozen keys instead of all of them. */
template<class K>
__global__ __launch_bounds__(256) void bracketedPositionsKernel(const K* __restrict__ tree, NodeIdx numNodes,
                                                                const K* __restrict__ keys,
                                                                const K* __restrict__ leafLo,
                                                                const uint32_t* __restrict__ numCompact,
                                                                const uint32_t* __restrict__ coarse,
                                                                const uint32_t* __restrict__ layoutNew,
                                                                uint32_t* __restrict__ pos)
{
    NodeIdx i = blockIdx.x * 256 + threadIdx.x;
    if (i > numNodes) return;
    const K key      = tree[i];
    const uint32_t J = *numCompact;
    uint32_t lo = 0, hi = J + 1; // last j in [0, J] with leafLo[j] <= key
    if (coarse)
    {
        constexpr int shift = 3 * int(maxLevel<K>()) - RESORT_COARSE_BITS;
        const uint32_t c    = uint32_t(key >> shift);
        lo                  = coarse[c];
        hi                  = c < (1u << RESORT_COARSE_BITS) ? coarse[c + 1] + 1 : J + 1;
    }
    while (hi - lo > 1)
    {
        uint32_t mid = (lo + hi) / 2;
        if (leafLo[mid] <= key) lo = mid;
        else hi = mid;
    }
    // first index with keys[index] >= key, inside that leaf's new range -- its start, without looking at any key, when
    // the boundary is that of the old leaf itself (most leaves of a tree outlive an update)
    const bool onBoundary = leafLo[lo] == key;
    uint32_t a = layoutNew[lo], len = onBoundary ? 0u : layoutNew[lo + 1] - a;
    while (len > 0)
    {
        uint32_t half = len >> 1;
        if (keys[a + half] < key) { a += half + 1, len -= half + 1; }
        else { len = half; }
    }
    pos[i] = a;
}

__global__ __launch_bounds__(256) void countsOfPositionsKernel(const uint32_t* __restrict__ pos, NodeIdx numNodes,
                                                               uint32_t maxCount, uint32_t* __restrict__ counts)
{
    NodeIdx i = blockIdx.x * 256 + threadIdx.x;
    if (i >= numNodes) return;
    uint32_t c = pos[i + 1] - pos[i];
    counts[i]  = c < maxCount ? c : maxCount;
}

//! the particles that carry the remove marker: behind every leaf, by ascending old position (idx sorted by the caller)
template<class K>
__global__ __launch_bounds__(256) void placeMarkersKernel(const uint32_t* __restrict__ idx, uint32_t count,
                                                          const uint32_t* __restrict__ layoutNew,
                                                          const uint32_t* __restrict__ numCompact,
                                                          K* __restrict__ keysOut, uint32_t* __restrict__ orderOut)
{
    uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= count) return;
    const uint32_t at = layoutNew[*numCompact] + r;
    keysOut[at]       = endKey<K>();
    orderOut[at]      = idx[r];
}

//! where J, the number of non-empty leaves of the table, lives on the device: the kernels read it there, the host reads
//! it back with the other scalars of the attempt
uint32_t* compactLeafCount(cstone_hip_ctx* ctx) { return (uint32_t*)(ctx->devScalars + RESORT_SCALARS) + 2; }

} // namespace

template<class K>
int LeafResort<K>::prepare(cstone_hip_ctx* ctx, const K* tree, const uint32_t* layout, int numLeaves, size_t n,
                           K* keysOut, bool expectMovers)
{
    // (the attempt's result scalars are cleared first, the table's scan writes J behind that; [3]: the mover counter)
    CS_HIP(ctx, hipMemsetAsync(ctx->devScalars + RESORT_SCALARS, 0, 4 * sizeof(int), ctx->stream));
    args_.keysOut = keysOut;
    StageTimer timer(ctx, CSTONE_STAGE_RESORT_BINS);
    numLeaves_         = numLeaves;
    n_                 = n;
    uint32_t* numJ     = compactLeafCount(ctx);
    const size_t words = (n + 63) / 64 + 1;
    const size_t ent   = size_t(numLeaves) + 3; // J + 2 <= numLeaves + 2 table entries, one more for the scans' totals
    const size_t cap   = n / 8 + 1024;
    CS_TRY(mask_.ensure(ctx, words * 8));
    CS_TRY(rank_.ensure(ctx, words * 4));
    CS_TRY(popc_.ensure(ctx, words * 4));
    CS_TRY(leafLo_.ensure(ctx, ent * sizeof(K)));
    CS_TRY(leafPos_.ensure(ctx, ent * 4));
    CS_TRY(outCount_.ensure(ctx, ent * 4));
    CS_TRY(incoming_.ensure(ctx, ent * 4));
    CS_TRY(newCount_.ensure(ctx, ent * 4));
    CS_TRY(layoutNew_.ensure(ctx, ent * 4));
    CS_TRY(inOffset_.ensure(ctx, ent * 4));
    CS_TRY(moverKeys_.ensure(ctx, cap * sizeof(K)));
    CS_TRY(moverIdx_.ensure(ctx, cap * 4));
    CS_TRY(moverDest_.ensure(ctx, cap * 4));
    CS_TRY(moverSlot_.ensure(ctx, cap * 4));
    CS_TRY(binKeys_.ensure(ctx, cap * sizeof(K)));
    CS_TRY(binIdx_.ensure(ctx, cap * 4));

    hipLaunchKernelGGL(leafStartWordsKernel, gridFor(numLeaves, 256), 256, 0, ctx->stream, layout, numLeaves, uint32_t(n),
                       mask_.as<uint64_t>(), popc_.as<uint32_t>(), uint32_t(words));
    // rank of every word and, in *numJ, the number of non-empty leaves
    CS_TRY(arenaReserve(ctx, scanArenaBytes(words)));
    int rc = scanU32(ctx, popc_.as<uint32_t>(), rank_.as<uint32_t>(), words, 0u, false, numJ);
    arenaReset(ctx);
    CS_TRY(rc);
    hipLaunchKernelGGL(fillCompactLeavesKernel<K>, gridFor(size_t(numLeaves) + 3, 256), 256, 0, ctx->stream, tree, layout,
                       numLeaves, mask_.as<uint64_t>(), rank_.as<uint32_t>(), numJ, uint32_t(n), leafLo_.as<K>(),
                       leafPos_.as<uint32_t>(), outCount_.as<uint32_t>(), incoming_.as<uint32_t>());
    // many movers expected (the previous sync had them): the coarse table that shortens their searches
    haveCoarse_ = expectMovers;
    constexpr uint32_t cells = (1u << RESORT_COARSE_BITS) + 1;
    CS_TRY(coarse_.ensure(ctx, size_t(cells) * 4)); // (4 MB, once: no allocation in the middle of a run)
    if (haveCoarse_)
    {
        hipLaunchKernelGGL(coarseLeafTableKernel<K>, gridFor(cells, 256), 256, 0, ctx->stream, leafLo_.as<K>(), numJ,
                           coarse_.as<uint32_t>());
    }
    CS_HIP(ctx, hipGetLastError());

    args_.leafStart  = mask_.as<uint64_t>();
    args_.leafRank   = rank_.as<uint32_t>();
    args_.leafLo     = leafLo_.as<K>();
    args_.outCount   = outCount_.as<uint32_t>();
    args_.moverKeys  = moverKeys_.as<K>();
    args_.moverIdx   = moverIdx_.as<uint32_t>();
    args_.moverCount = (uint32_t*)(ctx->devScalars + RESORT_SCALARS) + 3;
    args_.moverCap   = uint32_t(cap);
    return CSTONE_OK;
}

template<class K>
int LeafResort<K>::binMovers(cstone_hip_ctx* ctx, int leavesPerTile)
{
    StageTimer timer(ctx, CSTONE_STAGE_RESORT_BINS);
    int* scalars          = ctx->devScalars + RESORT_SCALARS;
    const uint32_t ent    = uint32_t(numLeaves_) + 3;
    const uint32_t* numJ  = compactLeafCount(ctx);
    const uint32_t* count = (const uint32_t*)scalars + 3;
    hipLaunchKernelGGL(binMoversKernel<K>, unsigned(ctx->numCu) * 16, 256, 0, ctx->stream, moverKeys_.as<K>(), count,
                       args_.moverCap, leafLo_.as<K>(), numJ, haveCoarse_ ? coarse_.as<uint32_t>() : nullptr,
                       incoming_.as<uint32_t>(), moverDest_.as<uint32_t>(), moverSlot_.as<uint32_t>());
    hipLaunchKernelGGL(newLeafSizesKernel, gridFor(ent, 256), 256, 0, ctx->stream, leafPos_.as<uint32_t>(),
                       outCount_.as<uint32_t>(), incoming_.as<uint32_t>(), numJ, ent, newCount_.as<uint32_t>(), scalars);
    CS_TRY(arenaReserve(ctx, 2 * scanArenaBytes(ent)));
    int rc = scanU32Pair(ctx, newCount_.as<uint32_t>(), layoutNew_.as<uint32_t>(), incoming_.as<uint32_t>(),
                         inOffset_.as<uint32_t>(), ent);
    arenaReset(ctx);
    CS_TRY(rc);
    hipLaunchKernelGGL(checkTilesKernel, gridFor(size_t(numLeaves_) / leavesPerTile + 1, 256), 256, 0, ctx->stream,
                       leafPos_.as<uint32_t>(), inOffset_.as<uint32_t>(), layoutNew_.as<uint32_t>(), numJ, count,
                       args_.moverCap, leavesPerTile, scalars);
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

template<class K>
int LeafResort<K>::sortLeaves(cstone_hip_ctx* ctx, const K* keysIn, K* keysOut, uint32_t* orderOut, uint32_t numMovers,
                              uint32_t numMarkers, uint32_t J, int leavesPerTile, bool largeQuietTiles)
{
    if (numMovers)
    {
        StageTimer timer(ctx, CSTONE_STAGE_RESORT_BINS);
        hipLaunchKernelGGL(placeMoversKernel<K>, gridFor(numMovers, 256), 256, 0, ctx->stream, moverKeys_.as<K>(),
                           moverIdx_.as<uint32_t>(), moverDest_.as<uint32_t>(), moverSlot_.as<uint32_t>(), numMovers,
                           inOffset_.as<uint32_t>(), binKeys_.as<K>(), binIdx_.as<uint32_t>());
    }
    if (numMarkers)
    {
        // all markers are equal keys: their stable order is that of their old positions
        StageTimer timer(ctx, CSTONE_STAGE_RESORT_BINS);
        // their bin is the last one: it starts at movers - markers
        uint32_t* idx = binIdx_.as<uint32_t>() + (numMovers - numMarkers);
        CS_TRY(cstone_hip_sort_keys(ctx, 32, idx, numMarkers));
        hipLaunchKernelGGL(placeMarkersKernel<K>, gridFor(numMarkers, 256), 256, 0, ctx->stream, idx, numMarkers,
                           layoutNew_.as<uint32_t>(), compactLeafCount(ctx), keysOut, orderOut);
    }
    if (J == 0) return CSTONE_OK;
    StageTimer timer(ctx, CSTONE_STAGE_RESORT_LEAVES);
    const unsigned grid    = (J + unsigned(leavesPerTile) - 1) / unsigned(leavesPerTile);
    const bool alwaysCount = std::getenv("CSTONE_RESORT_COUNT") != nullptr; // tuning/tests: no quiet-tile shortcut
    // quiet tiles and tiles in which something moved: one launch each over all tiles (without movers there are none of
    // the second kind)
    const bool someMoved = numMovers > 0 || alwaysCount || largeQuietTiles;
    // With at least one mover per tile on average hardly a tile is quiet: the wave kernel then takes all tiles and the
    // launch for quiet tiles is left out (at 10^8 particles 0.56 / 0.72 ms instead of 0.59 / 0.77 ms;
    // CSTONE_RESORT_WAVE_ALL=0/1 forces either)
    static const char* waveAllEnv = std::getenv("CSTONE_RESORT_WAVE_ALL");
    const bool waveAll            = !alwaysCount && (waveAllEnv ? waveAllEnv[0] == '1' : numMovers >= grid);
    // leaves that are less than half full on average: two or four of them per wave step, two elements per lane (the
    // kernel's flavour 1, pairSort; with fuller leaves it saves a few per cent when everything moves and loses more when
    // most leaves are still in order -- a step then sorts two leaves if either needs it; CSTONE_RESORT_PAIRS=0/1 forces)
    const char* pairsEnv        = std::getenv("CSTONE_RESORT_PAIRS"); // (read at every launch: the tests switch it)
    // (... and with fuller leaves when more than 3 % of the particles changed their leaf: hardly a leaf is still in order then)
    const bool pairs = pairsEnv ? pairsEnv[0] == '1' : (n_ < size_t(J) * 32u || size_t(numMovers) * 32u > n_);
    auto launch = [&](auto gTag)
    {
        constexpr int G = decltype(gTag)::value;
        if (!waveAll)
            hipLaunchKernelGGL((leafSortKernel<K, G>), grid, 256, 0, ctx->stream, keysIn, leafPos_.as<uint32_t>(),
                               inOffset_.as<uint32_t>(), layoutNew_.as<uint32_t>(), J, alwaysCount, keysOut, orderOut);
        if (!(someMoved || waveAll)) return;
        auto* wave = pairs ? leafSortWaveKernel<K, G, 1> : leafSortWaveKernel<K, G, 0>;
        hipLaunchKernelGGL(wave, grid, 256, 0, ctx->stream, keysIn, leafLo_.as<K>(), leafPos_.as<uint32_t>(),
                           inOffset_.as<uint32_t>(), layoutNew_.as<uint32_t>(), binKeys_.as<K>(), binIdx_.as<uint32_t>(),
                           J, alwaysCount, waveAll, keysOut, orderOut);
    };
    if (leavesPerTile == 64) launch(std::integral_constant<int, 64>{});
    else if (leavesPerTile == 32) launch(std::integral_constant<int, 32>{});
    else if (leavesPerTile == 16) launch(std::integral_constant<int, 16>{});
    else return fail(ctx, CSTONE_E_INTERNAL, "resort: %d leaves per workgroup not instantiated", leavesPerTile);
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

template<class K>
int LeafResort<K>::countLeaves(cstone_hip_ctx* ctx, const K* tree, int numNodes, const K* keys, uint32_t maxCount,
                               uint32_t* counts)
{
    if (numNodes <= 0) return CSTONE_OK;
    StageTimer timer(ctx, CSTONE_STAGE_NODE_COUNTS);
    CS_TRY(arenaReserve(ctx, alignUp(size_t(numNodes + 1) * sizeof(uint32_t)) + 1024));
    auto* pos = (uint32_t*)arenaTake(ctx, size_t(numNodes + 1) * sizeof(uint32_t));
    hipLaunchKernelGGL(bracketedPositionsKernel<K>, gridFor(size_t(numNodes) + 1, 256), 256, 0, ctx->stream, tree,
                       NodeIdx(numNodes), keys, leafLo_.as<K>(), compactLeafCount(ctx),
                       haveCoarse_ ? coarse_.as<uint32_t>() : nullptr, layoutNew_.as<uint32_t>(), pos);
    hipLaunchKernelGGL(countsOfPositionsKernel, gridFor(numNodes, 256), 256, 0, ctx->stream, pos, NodeIdx(numNodes),
                       maxCount, counts);
    arenaReset(ctx);
    CS_HIP(ctx, hipGetLastError());
    return CSTONE_OK;
}

template class LeafResort<uint32_t>;
template class LeafResort<uint64_t>;

#ifdef CSTONE_RESORT_TRACE
//! tuning builds: device buffer of RESORT_TRACE_SLOTS stamps per workgroup (nullptr: off)
extern "C" int cstone_hip_resort_trace_set(void* buffer)
{
    uint64_t* p = static_cast<uint64_t*>(buffer);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_resortTrace), &p, sizeof p) == hipSuccess ? 0 : 1;
}
#endif

} // namespace cship
