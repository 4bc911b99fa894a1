// The friends-of-friends group catalogue through the C++20 host layer on one MI355X: sync a few Gaussian blobs of
// different richness over a thin background in a periodic box -- every blob moves with a bulk velocity of its own --,
// find the groups, and print the five most massive with mass, centre, velocity and rms radius.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/fof_catalog_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o fof_catalog_example
// Then the same cloud through a multi-rank domain on a communicator of one rank (no collective is made):
// Domain::friendsOfFriendsGlobal and Domain::fofCatalogGlobal, the call that joins groups across ranks.
// Exits non-zero if Domain::fofGroupProperties and fofGroupPropertiesGpu disagree, if a listed group is flagged, if
// the centre of one of the five does not lie within a blob's sigma of a blob centre (modulo the box), or if the
// multi-rank table differs from the single-rank one by more than rounding (the filtered single-rank catalogue lists fewer
// members, so its group edges fall on other lanes and the sums may differ in the last places).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
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
    const int numBlobs        = 6;
    const unsigned minMembers = 20;
    const T sigma             = 0.02;

    // blob i gets a share of the particles that grows with i; one particle in four is background.  One blob sits across
    // the corner of the box
    std::mt19937 rng(42);
    std::normal_distribution<T> gauss(0.0, sigma);
    std::uniform_real_distribution<T> uni(0.0, 1.0);
    const T centers[numBlobs][3] = {{0.0, 0.0, 0.0}, {0.3, 0.7, 0.2}, {0.7, 0.3, 0.6}, {0.5, 0.5, 0.9}, {0.2, 0.2, 0.5}, {0.8, 0.8, 0.3}};
    const T bulk[numBlobs][3]    = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}};
    std::discrete_distribution<int> pick({1, 2, 3, 4, 5, 6});
    std::vector<T> hx(n), hy(n), hz(n), hh(n, 0.01), hm(n), hvx(n), hvy(n), hvz(n);
    auto wrap = [](T v) { v -= std::floor(v); return v < 1.0 ? v : 0.0; };
    for (std::size_t i = 0; i < n; ++i)
    {
        hm[i] = 0.5 + uni(rng);
        if (i % 4 == 3)
        {
            hx[i] = uni(rng), hy[i] = uni(rng), hz[i] = uni(rng);
            hvx[i] = hvy[i] = hvz[i] = 0;
        }
        else
        {
            const int b = pick(rng);
            hx[i] = wrap(centers[b][0] + gauss(rng)), hy[i] = wrap(centers[b][1] + gauss(rng)), hz[i] = wrap(centers[b][2] + gauss(rng));
            hvx[i] = bulk[b][0] + 0.1 * gauss(rng), hvy[i] = bulk[b][1] + 0.1 * gauss(rng), hvz[i] = bulk[b][2] + 0.1 * gauss(rng);
        }
    }
    auto dev = [n](const std::vector<T>& v) { return DeviceVector<T>(v.data(), v.data() + n); };
    DeviceVector<T> x = dev(hx), y = dev(hy), z = dev(hz), h = dev(hh), m = dev(hm), vx = dev(hvx), vy = dev(hvy), vz = dev(hvz),
                    scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    Box<T> box(0, 1, BoundaryType::periodic);
    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f, box);
    domain.sync(keys, x, y, z, h, std::tie(m, vx, vy, vz), scratch);

    const double b = 0.2 * std::cbrt(1.0 / double(n));
    DeviceVector<LocalIndex> labels, offsets, members;
    domain.friendsOfFriends(x, y, z, b, labels);
    const unsigned numListed = fofCatalogGpu(labels.data(), domain.startIndex(), domain.endIndex(), minMembers, offsets, members);

    FofGroupTable<T> table, table2;
    domain.fofGroupProperties(x, y, z, m, &vx, &vy, &vz, offsets, members, table);
    fofGroupPropertiesGpu(x.data(), y.data(), z.data(), m.data(), vx.data(), vy.data(), vz.data(), domain.box(), offsets,
                          members, table2);
    const auto mass = toHost(table.mass), center = toHost(table.center), velocity = toHost(table.velocity),
               radius = toHost(table.radius);
    const auto flags = toHost(table.flags), ho = toHost(offsets);
    const bool same  = toHost(table2.mass) == mass && toHost(table2.center) == center && toHost(table2.velocity) == velocity &&
                      toHost(table2.radius) == radius && toHost(table2.flags) == flags;

    std::vector<unsigned> byMass(numListed);
    std::iota(byMass.begin(), byMass.end(), 0u);
    std::sort(byMass.begin(), byMass.end(), [&](unsigned a, unsigned c) { return mass[a] > mass[c]; });
    std::printf("fof catalogue: particles %zu, linking length %.6f, groups with at least %u members %u\n", n, b, minMembers,
                numListed);
    unsigned flagged = 0, astray = 0;
    for (unsigned g = 0; g < numListed; ++g)
        flagged += flags[g] != 0;
    for (unsigned r = 0; r < std::min(numListed, 5u); ++r)
    {
        const unsigned g = byMass[r];
        std::printf("group %u: members %u mass %.6f centre (%.5f %.5f %.5f) velocity (%+.4f %+.4f %+.4f) radius %.5f\n", r,
                    ho[g + 1] - ho[g], mass[g], center[3 * g], center[3 * g + 1], center[3 * g + 2], velocity[3 * g],
                    velocity[3 * g + 1], velocity[3 * g + 2], radius[g]);
        T nearest = 1;
        for (int c = 0; c < numBlobs; ++c)
        {
            T d2 = 0;
            for (int a = 0; a < 3; ++a)
            {
                T d = center[3 * g + a] - centers[c][a];
                d -= std::rint(d);
                d2 += d * d;
            }
            nearest = std::min(nearest, std::sqrt(d2));
        }
        astray += nearest > sigma;
    }
    std::printf("flagged groups: %u, centres away from every blob: %u\n", flagged, astray);
    std::printf("fofGroupPropertiesGpu with the domain's box: %s\n", same ? "identical" : "DIFFERENT");

    // the multi-rank domain on one rank
    cstone_hip_comm_ops noComm{};
    Domain<KeyType, T> global(0, 1, 1024, 64, 0.5f, box, noComm);
    DeviceVector<T> gx = dev(hx), gy = dev(hy), gz = dev(hz), gh = dev(hh), gm = dev(hm), gvx = dev(hvx), gvy = dev(hvy),
                    gvz = dev(hvz);
    DeviceVector<KeyType> gkeys(n);
    Context::check(cstone_hip_memset(Context::get(), gkeys.data(), 0, n * sizeof(KeyType)), "memset");
    global.sync(gkeys, gx, gy, gz, gh, std::tie(gm, gvx, gvy, gvz), scratch);
    DeviceVector<std::uint64_t> glabels, groupLabels, groupSizes;
    global.friendsOfFriendsGlobal(gx, gy, gz, b, glabels);
    FofGroupTable<T> gtable;
    const unsigned numGlobal = global.fofCatalogGlobal(gx, gy, gz, gm, &gvx, &gvy, &gvz, glabels, minMembers, groupLabels,
                                                       groupSizes, gtable);
    const auto gmass = toHost(gtable.mass), gcenter = toHost(gtable.center);
    const auto gsizes = toHost(groupSizes);
    bool agree = numGlobal == numListed;
    for (unsigned g = 0; agree && g < numListed; ++g)
    {
        agree = gsizes[g] == ho[g + 1] - ho[g] && std::abs(gmass[g] - mass[g]) <= 1e-12 * mass[g];
        for (int a = 0; a < 3; ++a)
            agree = agree && std::abs(gcenter[3 * g + a] - center[3 * g + a]) <= 1e-12;
    }
    std::printf("fofCatalogGlobal on a communicator of one rank: %u groups, %s\n", numGlobal,
                agree ? "the same table" : "ANOTHER table");
    return (!same || !agree || flagged || astray || numListed < 5) ? 1 : 0;
}
