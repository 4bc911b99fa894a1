// The lock-free union-find of the friends-of-friends finder (cornerstone-octree_amd/csrc/union_find.hpp) on the host: the
// text the link kernel runs, with std::atomic for the device atomics.  Several threads unite the edges of known graphs in
// shuffled order; afterwards every vertex must end at the minimum index of its component (computed by a plain sequential
// search), the invariant parent[v] <= v must hold, and no union may have given up.  Every graph runs twice: with each edge
// once, in a random orientation, and with each edge in BOTH orientations plus a second copy of every third one -- what the
// link kernel hands over now that a pair is united from either side (a pair that both walks report comes twice, (i, j)
// from the lane of i and (j, i) from the lane of j, usually at the same time).  A compare-and-swap that always fails
// shows that the retry cap ends the loop and is reported.  Build plain, with -fsanitize=address,undefined and with
// -fsanitize=thread: this is where a lost update or a retry that does not end is found.
//
//   union_find_check [threads] [rounds]
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "union_find.hpp"

using namespace cship;
using Edge = std::pair<uint32_t, uint32_t>;

//! vertices first .. first + n - 1 at p[v - first], like the label array of a target range
struct HostParents
{
    std::atomic<uint32_t>* p;
    uint32_t first;
    uint32_t load(uint32_t v) const { return p[v - first].load(std::memory_order_relaxed); }
    uint32_t cas(uint32_t v, uint32_t expect, uint32_t set) const
    {
        p[v - first].compare_exchange_strong(expect, set, std::memory_order_relaxed);
        return expect; // what was found: the expected value on success
    }
};

//! a compare-and-swap that never succeeds and reports a value the invariant rules out (above the root it was tried on)
struct StuckParents : HostParents
{
    mutable uint64_t attempts = 0;
    uint32_t cas(uint32_t v, uint32_t, uint32_t) const
    {
        ++attempts;
        return v + 1;
    }
};

static std::vector<uint32_t> sequentialLabels(uint32_t first, uint32_t n, const std::vector<Edge>& edges)
{
    std::vector<std::vector<uint32_t>> adj(n);
    for (auto [a, b] : edges)
    {
        adj[a - first].push_back(b - first);
        adj[b - first].push_back(a - first);
    }
    std::vector<uint32_t> label(n, UINT32_MAX), stack;
    for (uint32_t s = 0; s < n; ++s) // ascending: the first vertex that reaches a component is its minimum
    {
        if (label[s] != UINT32_MAX) continue;
        label[s] = first + s;
        stack.push_back(s);
        while (!stack.empty())
        {
            uint32_t v = stack.back();
            stack.pop_back();
            for (uint32_t w : adj[v])
                if (label[w] == UINT32_MAX)
                {
                    label[w] = first + s;
                    stack.push_back(w);
                }
        }
    }
    return label;
}

static int failures = 0;

static void checkOnce(const std::string& name, uint32_t first, uint32_t n, std::vector<Edge> edges, int threads,
                      uint32_t seed, bool keepRoot, bool doubled)
{
    if (doubled)
    {
        const size_t m = edges.size();
        for (size_t e = 0; e < m; ++e)
        {
            edges.push_back({edges[e].second, edges[e].first});
            if (e % 3 == 0) edges.push_back(edges[e]);
        }
    }
    std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[n]);
    for (uint32_t k = 0; k < n; ++k)
        parent[k].store(first + k);
    HostParents ops{parent.get(), first};
    std::mt19937 rng(seed);
    std::shuffle(edges.begin(), edges.end(), rng);
    for (auto& e : edges)
        if (rng() & 1u) std::swap(e.first, e.second);

    std::atomic<int> gaveUp{0};
    std::atomic<bool> go{false};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back(
            [&, t]
            {
                while (!go.load()) {}
                bool mine = false;
                // keepRoot: as the kernel's lanes do, stay with one vertex for a stretch of edges and start from its last
                // known root
                uint32_t anchor = UINT32_MAX, root = 0;
                for (size_t e = t; e < edges.size(); e += threads)
                {
                    auto [a, b] = edges[e];
                    if (keepRoot && a == anchor) { root = ufUnite(ops, root, b, ufRetryCap, &mine); }
                    else
                    {
                        if (keepRoot && anchor != UINT32_MAX) ufCompress(ops, anchor, root);
                        anchor = a;
                        root   = ufUnite(ops, a, b, ufRetryCap, &mine);
                    }
                }
                if (keepRoot && anchor != UINT32_MAX) ufCompress(ops, anchor, root);
                if (mine) gaveUp.fetch_add(1);
            });
    go.store(true);
    for (auto& th : pool)
        th.join();

    const std::vector<uint32_t> want = sequentialLabels(first, n, edges);
    uint32_t bad = 0, broken = 0;
    for (uint32_t k = 0; k < n; ++k)
    {
        if (parent[k].load() > first + k || parent[k].load() < first) ++broken;
        if (ufFind(ops, first + k) != want[k]) ++bad;
    }
    if (bad || broken || gaveUp.load())
    {
        ++failures;
        std::printf("UNION_FIND FAIL %s%s: %u wrong labels, %u parents above their vertex, %d threads gave up\n", name.c_str(),
                    doubled ? " (edges doubled)" : "", bad, broken, gaveUp.load());
    }
}

static void check(const std::string& name, uint32_t first, uint32_t n, const std::vector<Edge>& edges, int threads,
                  uint32_t seed, bool keepRoot)
{
    checkOnce(name, first, n, edges, threads, seed, keepRoot, false);
    checkOnce(name, first, n, edges, threads, seed + 500, keepRoot, true);
}

int main(int argc, char** argv)
{
    const int threads = argc > 1 ? std::atoi(argv[1]) : 8;
    const int rounds  = argc > 2 ? std::atoi(argv[2]) : 3;
    int graphs        = 0;
    for (int round = 0; round < rounds; ++round)
        for (int keepRoot = 0; keepRoot < 2; ++keepRoot)
        {
            const uint32_t seed = 1000u * round + keepRoot, first = 37u * round;
            std::mt19937 rng(seed + 7);
            // a path: the longest chains
            {
                const uint32_t n = 5000;
                std::vector<Edge> e;
                for (uint32_t v = 1; v < n; ++v)
                    e.push_back({first + v, first + v - 1});
                check("path", first, n, e, threads, seed, keepRoot);
            }
            // a star on the LAST vertex: every union moves the same root
            {
                const uint32_t n = 3000;
                std::vector<Edge> e;
                for (uint32_t v = 0; v + 1 < n; ++v)
                    e.push_back({first + n - 1, first + v});
                check("star", first, n, e, threads, seed, keepRoot);
            }
            // two cliques, without and with a bridge
            for (int bridge = 0; bridge < 2; ++bridge)
            {
                const uint32_t m = 60, n = 2 * m + 5; // five singletons behind them
                std::vector<Edge> e;
                for (uint32_t c = 0; c < 2; ++c)
                    for (uint32_t a = 0; a < m; ++a)
                        for (uint32_t b = 0; b < a; ++b)
                            e.push_back({first + c * m + a, first + c * m + b});
                if (bridge) e.push_back({first + m - 1, first + 2 * m - 1});
                check(bridge ? "cliques+bridge" : "cliques", first, n, e, threads, seed, keepRoot);
            }
            // random graphs around the percolation threshold (mean degree 0.5, 1, 2) and a dense one
            for (double degree : {0.5, 1.0, 2.0, 8.0})
            {
                const uint32_t n = 20000;
                std::vector<Edge> e;
                std::uniform_int_distribution<uint32_t> pick(0, n - 1);
                for (uint32_t k = 0; k < uint32_t(degree * n / 2); ++k)
                {
                    uint32_t a = pick(rng), b = pick(rng);
                    if (a != b) e.push_back({first + a, first + b});
                }
                check("random-" + std::to_string(degree), first, n, e, threads, seed, keepRoot);
            }
            graphs += 8;
        }

    // the retry cap: a compare-and-swap that never succeeds ends after exactly cap attempts and is reported
    {
        std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[8]);
        for (uint32_t k = 0; k < 8; ++k)
            parent[k].store(k);
        for (uint32_t cap : {1u, 5u, 1000u, ufRetryCap})
        {
            StuckParents stuck{{parent.get(), 0}};
            bool gaveUp = false;
            (void)ufUnite(stuck, 6, 3, cap, &gaveUp);
            bool untouched = true;
            for (uint32_t k = 0; k < 8; ++k)
                untouched = untouched && parent[k].load() == k;
            if (!gaveUp || stuck.attempts != cap || !untouched)
            {
                ++failures;
                std::printf("UNION_FIND FAIL retry cap %u: gaveUp %d after %llu attempts\n", cap, int(gaveUp),
                            (unsigned long long)stuck.attempts);
            }
        }
        // ... and a union that needs no retry does not report one
        HostParents ops{parent.get(), 0};
        bool gaveUp = false;
        if (ufUnite(ops, 6, 3, 1, &gaveUp) != 3 || gaveUp || ufFind(ops, 6) != 3)
        {
            ++failures;
            std::printf("UNION_FIND FAIL plain union\n");
        }
    }
    if (failures) return 1;
    std::printf("UNION_FIND OK: %d graphs, %d threads, retry cap checked; every graph also with its edges reversed and "
                "duplicated\n",
                graphs, threads);
    return 0;
}
