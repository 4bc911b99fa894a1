// Stand-alone check of csrc/leaf_steps.hpp (the step plan of the leaf pass with two elements per lane) against a direct
// restatement of the rule the kernel used to evaluate inside its step loop: segBits and stepLeaves walked leaf by leaf,
// with leafAt2's choice of the leaves a step's lane segments hold.  tests/test_leaf_steps_host.py compiles this file with
// g++, once plain and once with -fsanitize=address,undefined, and runs both.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "leaf_steps.hpp"

namespace
{

struct Step
{
    uint32_t first, bits, leaves;
    bool empty, wide;
};

//! the rule as resort.hip had it: slots[0 ... n) are the quarter's leaves (kBegin = 0, kEnd = n); the steps go to want[]
uint32_t walkedLeafByLeaf(const uint32_t* slots, uint32_t n, Step* want)
{
    auto segBits = [&](uint32_t q) -> unsigned
    {
        const uint32_t s0 = slots[q];
        const uint32_t s1 = q + 1 < n ? slots[q + 1] : 0u;
        const uint32_t s2 = q + 2 < n ? slots[q + 2] : 0u;
        const uint32_t s3 = q + 3 < n ? slots[q + 3] : 0u;
        if (s0 > 64u) return 6u;
        const uint32_t m2 = std::max(s0, s1), m4 = std::max(m2, std::max(s2, s3));
        return m4 <= 32u ? 4u : 5u;
    };
    auto stepLeaves = [&](uint32_t q, unsigned bits) -> uint32_t
    {
        if (bits == 6) return 1u;
        if (bits == 4) return 4u;
        return (q + 1 < n && slots[q + 1] > 64u) ? 1u : 2u;
    };
    uint32_t numSteps = 0, k = 0;
    while (k < n)
    {
        const unsigned bits = segBits(k);
        // the leaves of the step's lane segments (leafAt2): segment g holds leaf k + g unless that lies behind the end or
        // is a second leaf of more than 64 slots
        const uint32_t secondSlots = k + 1 < n ? slots[k + 1] : 0u;
        uint32_t held = 0;
        bool empty    = true;
        for (uint32_t g = 0; g < (bits == 6 ? 1u : (64u >> bits)); ++g)
        {
            bool mine = k + g < n;
            if (bits == 5 && g == 1 && secondSlots > 64u) mine = false;
            if (!mine) continue;
            if (g != held) { std::printf("reference: segments with a leaf are not the first ones\n"), std::exit(2); }
            ++held;
            empty = empty && slots[k + g] == 0;
        }
        want[numSteps++] = {k, bits, held, empty, bits == 6 && slots[k] > 128u};
        if (held != std::min(stepLeaves(k, bits), n - k)) { std::printf("reference: held != consumed\n"), std::exit(2); }
        k += stepLeaves(k, bits);
    }
    return numSteps;
}

unsigned long long g_checked = 0;
constexpr uint32_t MAXQ = 16;
// The quarter and its plan END at the end of a heap block each, whatever the quarter's length: the sanitizer sees a read
// or a write behind the quarter's end.
std::unique_ptr<uint32_t[]> g_slots(new uint32_t[MAXQ]), g_words(new uint32_t[MAXQ]);

//! 0: the plan of this quarter is the walk's
int checkQuarter(const uint32_t* quarter, uint32_t n)
{
    uint32_t *slots = g_slots.get() + (MAXQ - n), *words = g_words.get() + (MAXQ - n);
    for (uint32_t i = 0; i < n; ++i)
        slots[i] = quarter[i], words[i] = 0;
    const uint32_t numSteps = cship::leafStepPlan(slots, n, words);
    Step want[MAXQ];
    const uint32_t numWant = walkedLeafByLeaf(slots, n, want);
    auto fail = [&](const char* what, uint32_t s)
    {
        std::printf("FAILED (%s, step %u): n = %u, slots =", what, s, n);
        for (uint32_t i = 0; i < n; ++i)
            std::printf(" %u", slots[i]);
        std::printf("\n");
        return 1;
    };
    if (numSteps > n) return fail("more steps than leaves", numSteps);
    if (numSteps != numWant) return fail("number of steps", numSteps);
    int seen[MAXQ] = {};
    for (uint32_t s = 0; s < numSteps; ++s)
    {
        const uint32_t w = words[s];
        const uint32_t first = cship::leafStepFirst(w), bits = cship::leafStepBits(w), leaves = cship::leafStepLeaves(w);
        if (w == 0) return fail("word 0", s);
        if (first != want[s].first || bits != want[s].bits || leaves != want[s].leaves) return fail("step differs", s);
        if (cship::leafStepEmpty(w) != want[s].empty || cship::leafStepWide(w) != want[s].wide) return fail("kind", s);
        if (leaves == 0 || first + leaves > n) return fail("step crosses the quarter's end", s);
        if (bits != 6 && leaves > (64u >> bits)) return fail("more leaves than segments", s);
        for (uint32_t g = 0; g < leaves; ++g)
            ++seen[first + g];
        // what the kernel holds in a lane for the leaf at `first` is the same word, whatever lies behind the end
        const uint32_t left = n - first;
        const uint32_t at   = cship::leafStepAt(first, left, slots[first], left > 1 ? slots[first + 1] : 77u,
                                                left > 2 ? slots[first + 2] : 77u, left > 3 ? slots[first + 3] : 77u);
        if (at != w) return fail("leafStepAt looks behind the end", s);
    }
    for (uint32_t i = 0; i < n; ++i)
        if (seen[i] != 1) return fail("a leaf in no step or in two", i);
    ++g_checked;
    return 0;
}

} // namespace

int main()
{
    const uint32_t sizes[9] = {0, 1, 32, 33, 64, 65, 128, 129, 255};
    uint32_t state = 20240607u; // (xorshift32, fixed seed)
    auto rng       = [&state]()
    {
        state ^= state << 13, state ^= state >> 17, state ^= state << 5;
        return state;
    };
    // every sequence of 1-6 sizes, in a quarter of every length from the sequence's to 16: in front of a padding of random
    // sizes (from the list or anything below 256), and behind one of one leaf and one that fills the quarter up to 16
    for (uint32_t len = 1; len <= 6; ++len)
    {
        uint32_t count = 1;
        for (uint32_t i = 0; i < len; ++i)
            count *= 9;
        for (uint32_t code = 0; code < count; ++code)
        {
            uint32_t seq[6];
            for (uint32_t i = 0, c = code; i < len; ++i, c /= 9)
                seq[i] = sizes[c % 9];
            for (uint32_t n = len; n <= 16; ++n)
            {
                for (int behind = 0; behind < (n > len && (n == len + 1 || n == MAXQ) ? 2 : 1); ++behind)
                {
                    uint32_t quarter[MAXQ];
                    for (uint32_t i = 0; i < n - len; ++i)
                    {
                        const uint32_t r             = rng();
                        quarter[behind ? i : len + i] = (r & 1u) ? sizes[(r >> 1) % 9u] : (r >> 1) % 256u;
                    }
                    for (uint32_t i = 0; i < len; ++i)
                        quarter[behind ? n - len + i : i] = seq[i];
                    if (checkQuarter(quarter, n)) return 1;
                }
            }
        }
    }
    std::printf("leaf steps ok: %llu quarters\n", g_checked);
    return 0;
}
