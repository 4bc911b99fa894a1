// Friends-of-friends groups through the C++20 host layer on one MI355X: sync a few Gaussian blobs over a thin background
// in a periodic box, find the groups at a linking length of 0.2 x the mean particle separation, list those with at least
// 20 members.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/fof_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o fof_example
// Exits non-zero if the members of a listed group are not mutually reachable over links (checked on the host with the
// rule of include/cstone_hip.h), or if the catalogue disagrees with the labels.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "cstone_amd/cstone_amd.hpp"

using namespace cstone_amd;

int main(int argc, char** argv)
{
    using KeyType = std::uint64_t;
    using T       = double;
    std::size_t n = argc > 1 ? std::stoul(argv[1]) : 40000;
    const int numBlobs       = 6;
    const unsigned minMembers = 20;

    // blobs of sigma 0.02 (one of them across the corner of the box) and a uniform background of one particle in four
    std::mt19937 rng(42);
    std::normal_distribution<T> gauss(0.0, 0.02);
    std::uniform_real_distribution<T> uni(0.0, 1.0);
    const T centers[numBlobs][3] = {{0.0, 0.0, 0.0}, {0.3, 0.7, 0.2}, {0.7, 0.3, 0.6}, {0.5, 0.5, 0.9}, {0.2, 0.2, 0.5}, {0.8, 0.8, 0.3}};
    std::vector<T> hx(n), hy(n), hz(n), hh(n, 0.01);
    auto wrap = [](T v) { v -= std::floor(v); return v < 1.0 ? v : 0.0; };
    for (std::size_t i = 0; i < n; ++i)
    {
        if (i % 4 == 3) { hx[i] = uni(rng), hy[i] = uni(rng), hz[i] = uni(rng); }
        else
        {
            const T* c = centers[i % numBlobs];
            hx[i] = wrap(c[0] + gauss(rng)), hy[i] = wrap(c[1] + gauss(rng)), hz[i] = wrap(c[2] + gauss(rng));
        }
    }
    DeviceVector<T> x(hx.data(), hx.data() + n), y(hy.data(), hy.data() + n), z(hz.data(), hz.data() + n),
        h(hh.data(), hh.data() + n), scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    Box<T> box(0, 1, BoundaryType::periodic);
    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f, box);
    domain.sync(keys, x, y, z, h, std::tie(), scratch);

    const double b = 0.2 * std::cbrt(1.0 / double(n));
    DeviceVector<LocalIndex> labels, offsets, members;
    DeviceVector<unsigned> sizes;
    const unsigned numGroups = domain.friendsOfFriends(x, y, z, b, labels, &sizes);
    const unsigned numListed = fofCatalogGpu(labels.data(), domain.startIndex(), domain.endIndex(), minMembers, offsets, members);

    // the same through the free function: range, tree view and box spelled out
    DeviceVector<LocalIndex> labels2(domain.nParticles());
    const unsigned numGroups2 = friendsOfFriendsGpu(x.data(), y.data(), z.data(), domain.startIndex(), domain.endIndex(),
                                                    domain.box(), domain.octreeProperties(), b, labels2.data());
    const auto hl = toHost(labels), hs = toHost(sizes), ho = toHost(offsets), hm = toHost(members);
    const bool same = toHost(labels2) == hl && numGroups2 == numGroups;

    std::vector<unsigned> listedSizes;
    for (unsigned g = 0; g < numListed; ++g)
        listedSizes.push_back(ho[g + 1] - ho[g]);
    std::sort(listedSizes.rbegin(), listedSizes.rend());
    std::printf("fof: particles %zu, linking length %.6f, groups %u, groups with at least %u members %u\n", hl.size(), b,
                numGroups, minMembers, numListed);
    std::printf("largest:");
    for (std::size_t g = 0; g < std::min<std::size_t>(listedSizes.size(), 8); ++g)
        std::printf(" %u", listedSizes[g]);
    std::printf("\nfriendsOfFriendsGpu on the domain's tree view: %s\n", same ? "identical" : "DIFFERENT");

    // host check: inside every listed group, a search over links from its first member reaches every member; the members
    // carry the group's label and size.  The link test is the library's rule: T arithmetic, d2 a left fold, strict <
    const auto px = toHost(x), py = toHost(y), pz = toHost(z);
    const T hi = T(0.5) * T(b), radSq = T(4) * hi * hi;
    const LocalIndex first = domain.startIndex();
    auto fold = [](T d) { return d - T(1) * std::rint(d * T(1)); };
    unsigned bad = 0;
    for (unsigned g = 0; g < numListed; ++g)
    {
        const LocalIndex* m = hm.data() + ho[g];
        const unsigned cnt  = ho[g + 1] - ho[g];
        std::vector<char> seen(cnt, 0);
        std::vector<unsigned> stack{0};
        seen[0]          = 1;
        unsigned reached = 1;
        while (!stack.empty())
        {
            const unsigned a = stack.back();
            stack.pop_back();
            for (unsigned c = 0; c < cnt; ++c)
            {
                if (seen[c]) continue;
                const T dx = fold(px[m[c]] - px[m[a]]), dy = fold(py[m[c]] - py[m[a]]), dz = fold(pz[m[c]] - pz[m[a]]);
                if (dx * dx + dy * dy + dz * dz < radSq)
                {
                    seen[c] = 1;
                    ++reached;
                    stack.push_back(c);
                }
            }
        }
        bool ok = reached == cnt && m[0] == hl[m[0] - first];
        for (unsigned c = 0; c < cnt; ++c)
            ok = ok && hl[m[c] - first] == m[0] && hs[m[c] - first] == cnt && (c == 0 || m[c - 1] < m[c]);
        bad += !ok;
    }
    std::printf("listed groups whose members are not mutually reachable: %u\n", bad);
    return (bad || !same || numListed == 0) ? 1 : 0;
}
