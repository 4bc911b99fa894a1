// TEST INFRASTRUCTURE.  The update step of the global tree that every steady-state sync makes on the HOST
// (cornerstone-octree_amd/csrc/host_rules.hpp, globalTreeStepHost) against the oracle's update_octree, for 32- and 64-bit
// keys and buckets of 16 and 64: from the root and the exact counts of a clustered cloud to convergence, then on through
// a drift, the removal of most of a region and a collapse onto a clump.  Each step starts from the ORACLE's tree and
// counts; the product must say "unchanged" exactly when the oracle's leaf array is unchanged and otherwise produce the
// same array.  Every decision (merge, keep, split by 8 / 64 / 512 / 4096) must have been taken on the way.
// Built by `make -C oracle rules` as host_rules_check and, with -fsanitize=address,undefined, host_rules_check_asan.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "host_rules.hpp"

extern "C"
{
int cstone_oracle_node_counts(int key_bits, const void* tree, unsigned* counts, int num_nodes, const void* keys, size_t n,
                              unsigned max_count);
int cstone_oracle_node_ops(int key_bits, const void* tree, int num_nodes, const unsigned* counts, unsigned bucket,
                           int* node_ops, int* converged);
int cstone_oracle_update_octree(int key_bits, const void* keys, size_t n, unsigned bucket, void* tree_io,
                                unsigned* counts_io, int* num_leaves, int cap_leaves, unsigned max_count, int* converged);
}

namespace
{

constexpr int CAP = 1 << 20; // leaves the oracle's step may produce
const int OPS[6]  = {0, 1, 8, 64, 512, 4096};

template<class K>
struct Run
{
    static constexpr int kb = 8 * sizeof(K);
    static constexpr K end  = K(1) << (3 * cship::hostMaxLevel<K>());
    unsigned bucket;
    std::vector<K> keys, tree{0, end};
    std::vector<uint32_t> counts{0};
    long tally[6] = {0, 0, 0, 0, 0, 0};
    int steps     = 0;

    void recount()
    {
        std::sort(keys.begin(), keys.end());
        cstone_oracle_node_counts(kb, tree.data(), counts.data(), int(counts.size()), keys.data(), keys.size(), ~0u);
    }

    //! one step on both sides; true: the leaf array stayed.  Exits on a difference.
    bool step()
    {
        const int numNodes = int(counts.size());
        std::vector<int> ops(numNodes + 1);
        int conv = 0;
        cstone_oracle_node_ops(kb, tree.data(), numNodes, counts.data(), bucket, ops.data(), &conv);
        for (int i = 0; i < numNodes; ++i)
            for (int o = 0; o < 6; ++o)
                tally[o] += ops[i] == OPS[o];

        std::vector<K> mine;
        const bool same = cship::globalTreeStepHost<K>(tree, counts, bucket, mine);

        std::vector<K> ref(tree);
        std::vector<uint32_t> refCounts(counts);
        ref.resize(CAP + 1), refCounts.resize(CAP);
        int leaves = numNodes;
        const int rc = cstone_oracle_update_octree(kb, keys.data(), keys.size(), bucket, ref.data(), refCounts.data(),
                                                   &leaves, CAP, ~0u, &conv);
        if (rc != 0) fail("the oracle's update step failed");
        ref.resize(leaves + 1), refCounts.resize(leaves);
        const bool refSame = ref == tree;
        if (same != refSame) fail(same ? "reports an unchanged tree, the oracle changed it" : "changed a tree the oracle kept");
        if (!same && !(mine == ref)) fail("leaf arrays differ");
        tree.swap(ref), counts.swap(refCounts);
        ++steps;
        return refSame;
    }

    void untilConverged()
    {
        for (int guard = 0; !step(); ++guard)
            if (guard > 60) fail("no convergence");
    }

    [[noreturn]] void fail(const char* what) const
    {
        std::printf("HOST_RULES FAILED k%d bucket %u step %d (%zu leaves): %s\n", kb, bucket, steps, counts.size(), what);
        std::exit(1);
    }
};

template<class K>
void check(unsigned bucket, size_t n, unsigned seed)
{
    Run<K> r;
    r.bucket = bucket;
    std::mt19937_64 rng(seed);
    constexpr unsigned top = cship::hostMaxLevel<K>();
    auto span   = [](unsigned level) { return K(1) << (3 * (top - level)); };
    auto within = [&](K start, K len) { return K(start + K(rng() % uint64_t(len))); };
    // a uniform background and clumps of 1/4, 1/16, 1/64 and 1/256 of the keys inside cells of level 5, so that the nodes
    // the first split (by 4096, to level 4) leaves behind hold counts on either side of every threshold
    r.keys.resize(n);
    const K clump[4] = {within(0, r.end), within(0, r.end), within(0, r.end), within(0, r.end)};
    for (size_t i = 0; i < n; ++i)
    {
        int c = -1;
        for (int q = 0; q < 4 && c < 0; ++q)
            if (i % (size_t(4) << (2 * q)) == size_t(q + 1)) c = q;
        r.keys[i] = c < 0 ? within(0, r.end) : within(K(clump[c] / span(5) * span(5)), span(5));
    }
    r.counts[0] = 0;
    r.recount();
    r.untilConverged();
    // drift: every key moves by up to a cell of level 6 (merges and splits by 8 at the edges of the clumps)
    for (int round = 0; round < 3; ++round)
    {
        for (K& k : r.keys)
            k = K(std::min<uint64_t>(uint64_t(r.end) - 1, uint64_t(k) + rng() % uint64_t(span(6))));
        r.recount();
        r.step();
    }
    // most of the lower half of the curve goes away: its leaves merge level by level
    {
        std::vector<K> kept;
        for (K k : r.keys)
            if (k >= r.end / 2 || rng() % 16 == 0) kept.push_back(k);
        r.keys.swap(kept);
    }
    r.recount();
    r.untilConverged();
    // everything collapses onto one cell of level 7: merges everywhere else, splits by 4096 there
    for (K& k : r.keys)
        k = within(K(clump[0] / span(7) * span(7)), span(7));
    r.recount();
    r.untilConverged();

    std::printf("HOST_RULES k%d bucket %u: %d steps, merge %ld keep %ld split8 %ld split64 %ld split512 %ld split4096 %ld\n",
                r.kb, bucket, r.steps, r.tally[0], r.tally[1], r.tally[2], r.tally[3], r.tally[4], r.tally[5]);
    for (int o = 0; o < 6; ++o)
        if (r.tally[o] == 0) r.fail("a decision was never taken");
}

} // namespace

int main()
{
    // more than 64 x 512 keys: the root itself splits by 4096 at either bucket size
    check<uint32_t>(16, 40000, 1);
    check<uint32_t>(64, 40000, 2);
    check<uint64_t>(16, 40000, 3);
    check<uint64_t>(64, 40000, 4);
    std::printf("HOST_RULES OK\n");
    return 0;
}
