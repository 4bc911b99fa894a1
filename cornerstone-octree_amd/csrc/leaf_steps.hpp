// The step plan of the leaf pass with two elements per lane (leafSortWaveKernel, flavour 1 in resort.hip): which leaves of a
// wave's quarter of a tile share a wave step.  It depends on the leaves' slot counts only (old slots + arrivals), never on
// the keys, so the kernel decides it once per tile and the step loop runs on the packed result.  Plain C++ without HIP
// types: tests/leaf_steps_check.cpp walks the same functions on the CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CSTONE_LEAF_STEPS_HD __host__ __device__
#else
#define CSTONE_LEAF_STEPS_HD
#endif

namespace cship
{

/*! One word per step: bits 0-7 the first leaf (counted from the start of the quarter), bits 8-10 log2 of the lanes of a
 *  segment (4: up to four leaves of at most 32 slots, 16 lanes each; 5: up to two leaves of at most 64 slots, 32 lanes
 *  each; 6: one leaf of more than 64 slots has the wave to itself), bits 12-14 the leaves the step consumes (1-4).  A
 *  step's leaves are first, first + 1, ...: the lanes of segment g hold leaf first + g if g < leaves, no leaf otherwise.
 *  Bit 11: none of the step's leaves has a slot; bit 15: the step's one leaf has more than 128 slots (four registers per
 *  lane instead of two).  No step is the word 0. */
CSTONE_LEAF_STEPS_HD inline constexpr uint32_t leafStepPack(uint32_t first, uint32_t bits, uint32_t leaves)
{
    return first | (bits << 8) | (leaves << 12);
}
CSTONE_LEAF_STEPS_HD inline constexpr uint32_t leafStepFirst(uint32_t word) { return word & 0xFFu; }
CSTONE_LEAF_STEPS_HD inline constexpr uint32_t leafStepBits(uint32_t word) { return (word >> 8) & 7u; }
CSTONE_LEAF_STEPS_HD inline constexpr uint32_t leafStepLeaves(uint32_t word) { return (word >> 12) & 7u; }
CSTONE_LEAF_STEPS_HD inline constexpr bool leafStepEmpty(uint32_t word) { return (word & 0x800u) != 0; }
CSTONE_LEAF_STEPS_HD inline constexpr bool leafStepWide(uint32_t word) { return (word & 0x8000u) != 0; }

/*! The step that starts at leaf `first` of a quarter with `left` >= 1 leaves from there to its end; s0 ... s3: the slots of
 *  that leaf and the three behind it (those at or behind the quarter's end are not looked at).
 *  More than 64 slots: the leaf alone.  At most 32 slots in all four: the four together (fewer at the quarter's end).
 *  Otherwise two, or the first alone if the second has more than 64 slots (it waits for a step of its own) or lies
 *  behind the end. */
CSTONE_LEAF_STEPS_HD inline constexpr uint32_t leafStepAt(uint32_t first, uint32_t left, uint32_t s0, uint32_t s1,
                                                          uint32_t s2, uint32_t s3)
{
    s1 = left > 1u ? s1 : 0u;
    s2 = left > 2u ? s2 : 0u;
    s3 = left > 3u ? s3 : 0u;
    if (s0 > 64u) return leafStepPack(first, 6u, 1u) | (s0 > 128u ? 0x8000u : 0u);
    const uint32_t m2 = s0 > s1 ? s0 : s1, m3 = s2 > s3 ? s2 : s3, m4 = m2 > m3 ? m2 : m3;
    if (m4 <= 32u) return leafStepPack(first, 4u, left < 4u ? left : 4u) | (m4 == 0u ? 0x800u : 0u);
    if (s1 > 64u) return leafStepPack(first, 5u, 1u) | (s0 == 0u ? 0x800u : 0u);
    return leafStepPack(first, 5u, left > 1u ? 2u : 1u) | (m2 == 0u ? 0x800u : 0u);
}

/*! The steps of a quarter of n leaves with the given slots: words[0 ... return value), at most n of them.  Every step
 *  consumes at least one leaf and none reaches behind the quarter's end, so the walk visits every leaf exactly once.
 *  (The kernel holds leafStepAt of every leaf in a lane and walks the same way: next first = first + leaves.) */
CSTONE_LEAF_STEPS_HD inline constexpr uint32_t leafStepPlan(const uint32_t* slots, uint32_t n, uint32_t* words)
{
    uint32_t numSteps = 0;
    for (uint32_t q = 0; q < n && numSteps < n;)
    {
        const uint32_t left = n - q;
        const uint32_t w    = leafStepAt(q, left, slots[q], left > 1u ? slots[q + 1] : 0u, left > 2u ? slots[q + 2] : 0u,
                                         left > 3u ? slots[q + 3] : 0u);
        words[numSteps++]   = w;
        q += leafStepLeaves(w);
    }
    return numSteps;
}

} // namespace cship
