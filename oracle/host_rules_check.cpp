// TEST INFRASTRUCTURE.  The update step of the global tree that every steady-state sync makes on the HOST
// (cornerstone-octree_amd/csrc/host_rules.hpp, globalTreeStepHost) against the oracle's update_octree, for 32- and 64-bit
// keys and buckets of 16 and 64: from the root and the exact counts of a clustered cloud to convergence, then on through
// a drift, the removal of most of a region and a collapse onto a clump.  Each step starts from the ORACLE's tree and
// counts; the product must say "unchanged" exactly when the oracle's leaf array is unchanged and otherwise produce the
// same array.  Every decision (merge, keep, split by 8 / 64 / 512 / 4096) must have been taken on the way.
// exchangePlan and resultMargins / blockWithHalos (the multi-rank sync) are held against known answers written by hand.
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

// ---- known answers for the two rules of the multi-rank sync that need no oracle (exchangePlan, resultMargins)

int cases = 0;
void expect(bool ok, const char* what)
{
    ++cases;
    if (ok) return;
    std::printf("HOST_RULES FAILED %s\n", what);
    std::exit(1);
}

using Rows = std::vector<uint64_t>;
bool planIs(const cship::ExchangePlan& e, uint64_t movedAny, uint64_t mSend, uint64_t na, uint64_t nb)
{
    return e.failedRank == -1 && e.badRank == -1 && e.movedAny == movedAny && e.mSend == mSend && e.na == na && e.nb == nb;
}

void checkExchangePlan()
{
    using cship::exchangePlan;
    // one rank: the rows are not read, everything stays
    cship::ExchangePlan e = exchangePlan(0, 1, {0, 10}, {});
    expect(planIs(e, 0, 0, 10, 0) && e.sendCounts == Rows{10} && e.matrix == Rows{10}, "exchangePlan: one rank");
    // three ranks, rows of send counts with their status word; each rank's cut points are the prefix sums of its row
    const Rows rows{5, 2, 1, 0, /**/ 0, 7, 3, 0, /**/ 4, 0, 6, 0};
    const Rows matrix{5, 2, 1, 0, 7, 3, 4, 0, 6};
    e = exchangePlan(0, 3, {0, 5, 7, 8}, rows);
    expect(planIs(e, 10, 3, 5, 4) && e.sendCounts == Rows{5, 2, 1} && e.matrix == matrix, "exchangePlan: rank 0 of 3");
    e = exchangePlan(1, 3, {0, 0, 7, 10}, rows);
    expect(planIs(e, 10, 3, 7, 2) && e.sendCounts == Rows{0, 7, 3} && e.matrix == matrix, "exchangePlan: rank 1 of 3");
    e = exchangePlan(2, 3, {0, 4, 4, 10}, rows);
    expect(planIs(e, 10, 4, 6, 4) && e.sendCounts == Rows{4, 0, 6} && e.matrix == matrix, "exchangePlan: rank 2 of 3");
    Rows r = rows;
    r[1 * 4 + 3] = 1; // rank 1 reports a failure
    expect(exchangePlan(0, 3, {0, 5, 7, 8}, r).failedRank == 1, "exchangePlan: status word of rank 1");
    r = rows;
    r[0 * 4 + 1] = r[1 * 4 + 1] = 0; // nobody keeps or sends anything for rank 1
    e = exchangePlan(2, 3, {0, 4, 4, 10}, r);
    expect(e.failedRank == -1 && e.badRank == 1 && e.badArriving == 0, "exchangePlan: a rank that receives nothing");
    r = rows;
    r[0 * 4 + 2] = (uint64_t(1) << 30) - 9; // 2^30 arrive at rank 2
    e = exchangePlan(0, 3, {0, 5, 7, 7 + r[2]}, r);
    expect(e.failedRank == -1 && e.badRank == 2 && e.badArriving == uint64_t(1) << 30, "exchangePlan: a rank at 2^30");
    --r[0 * 4 + 2];
    expect(exchangePlan(0, 3, {0, 5, 7, 7 + r[2]}, r).badRank == -1, "exchangePlan: a rank at 2^30 - 1");
}

bool blockIs(const cship::BlockWithHalos& b, bool move, uint64_t M2, uint64_t cap2, uint64_t off)
{
    return b.move == move && b.M2 == M2 && b.cap2 == cap2 && b.off == off;
}

void checkResultMargins()
{
    using cship::blockWithHalos;
    using cship::resultMargins;
    // the first call: a quarter of the block on either side, M rounded up to 4 elements
    cship::ResultMargins m = resultMargins(40006, 0, 0, true, true);
    expect(m.M == 10004 && m.cap == 10004 + 40006 + 10001, "resultMargins: first call");
    m = resultMargins(1000, 0, 0, true, true);
    expect(m.M == 4096 && m.cap == 4096 + 1000 + 4096, "resultMargins: first call of a small rank");
    // steady state: twice the halos of the previous sync and a page; the block fits
    m = resultMargins(1000, 11, 7, false, true);
    expect(m.M == 4120 && m.cap == 4120 + 1000 + 14 + 4096, "resultMargins: steady state");
    expect(blockIs(blockWithHalos(m.M, m.cap, 1000, 12, 9), false, m.M, m.cap, m.M - 12), "blockWithHalos: fits");
    // the lower side
    expect(blockIs(blockWithHalos(m.M, m.cap, 1000, m.M, 9), false, m.M, m.cap, 0), "blockWithHalos: nlo == M");
    expect(blockIs(blockWithHalos(m.M, m.cap, 1000, m.M + 1, 9), true, m.M + 4, m.M + 4 + 1000 + 9, 3),
           "blockWithHalos: nlo == M + 1");
    // the upper side
    const uint64_t room = m.cap - m.M - 1000;
    expect(blockIs(blockWithHalos(m.M, m.cap, 1000, 12, room), false, m.M, m.cap, m.M - 12), "blockWithHalos: up to cap");
    expect(blockIs(blockWithHalos(m.M, m.cap, 1000, 12, room + 1), true, 12, 12 + 1000 + room + 1, 0),
           "blockWithHalos: up to cap + 1");
    // no margins: the block starts the arrays and moves as soon as there is a halo
    m = resultMargins(1000, 11, 7, false, false);
    expect(m.M == 0 && m.cap == 1000, "resultMargins: no margins");
    expect(blockIs(blockWithHalos(0, 1000, 1000, 0, 0), false, 0, 1000, 0), "blockWithHalos: no margins, no halos");
    expect(blockIs(blockWithHalos(0, 1000, 1000, 5, 2), true, 8, 1010, 3), "blockWithHalos: no margins, halos");
}

// ---- partialSortStartPass: which digit passes Domain::sync leaves to the fix-up of the runs (sort.hip)

//! the rule restated: low bits below the deepest leaf level + margin, in whole digits, rounded down to an even count
template<class K>
void checkStartPassProperties()
{
    const int top = int(cship::hostMaxLevel<K>());
    for (uint32_t bucket : {16u, 64u, 128u, 129u, 1024u, 1025u})
    {
        const int margin = bucket <= 128 ? 1 : bucket <= 1024 ? 2 : 3;
        for (int L = 0; L <= top; ++L)
        {
            const int p  = cship::partialSortStartPass<K>(L, bucket);
            auto holds   = [&](int q) { return 8 * q + 3 * (L + margin) <= 3 * top; };
            auto inRange = [&](int q) { return q >= 0 && q <= int(sizeof(K)) - 2; };
            expect(p % 2 == 0 && inRange(p), "partialSortStartPass: even and in [0, sizeof(K) - 2]");
            expect(!holds(0) || holds(p), "partialSortStartPass: skipped digits lie below level L + margin");
            expect(!holds(0) ? p == 0 : (!inRange(p + 2) || !holds(p + 2)), "partialSortStartPass: no two more digits fit");
        }
    }
}

void checkPartialSortStartPass()
{
    using cship::partialSortStartPass;
    expect(partialSortStartPass<uint64_t>(4, 64) == 6, "partialSortStartPass<uint64_t>(4, 64)");
    expect(partialSortStartPass<uint64_t>(9, 64) == 4, "partialSortStartPass<uint64_t>(9, 64)");
    expect(partialSortStartPass<uint64_t>(10, 64) == 2, "partialSortStartPass<uint64_t>(10, 64)");
    expect(partialSortStartPass<uint64_t>(15, 64) == 0, "partialSortStartPass<uint64_t>(15, 64)");
    expect(partialSortStartPass<uint64_t>(9, 200) == 2, "partialSortStartPass<uint64_t>(9, 200)");
    expect(partialSortStartPass<uint64_t>(21, 64) == 0, "partialSortStartPass<uint64_t>(21, 64)");
    expect(partialSortStartPass<uint32_t>(3, 64) == 2, "partialSortStartPass<uint32_t>(3, 64)");
    expect(partialSortStartPass<uint32_t>(4, 64) == 0, "partialSortStartPass<uint32_t>(4, 64)");
    expect(partialSortStartPass<uint32_t>(2, 200) == 2, "partialSortStartPass<uint32_t>(2, 200)");
}

} // namespace

int main()
{
    checkExchangePlan();
    checkResultMargins();
    std::printf("HOST_RULES exchangePlan and resultMargins: %d known answers\n", cases);
    cases = 0;
    checkPartialSortStartPass();
    const int hand = cases;
    checkStartPassProperties<uint32_t>();
    checkStartPassProperties<uint64_t>();
    std::printf("HOST_RULES partialSortStartPass: %d hand values, %d property checks\n", hand, cases - hand);
    // more than 64 x 512 keys: the root itself splits by 4096 at either bucket size
    check<uint32_t>(16, 40000, 1);
    check<uint32_t>(64, 40000, 2);
    check<uint64_t>(16, 40000, 3);
    check<uint64_t>(64, 40000, 4);
    std::printf("HOST_RULES OK\n");
    return 0;
}
