// Radial profiles and spherical-overdensity masses about the centres of friends-of-friends groups, through the C++20
// host layer on one MI355X: sync a few Gaussian blobs over a thin background in a periodic box, find the groups, build
// the catalogue, take the mass profile about every group's centre in bins scaled by the group's rms radius (out to 3
// radii), and print R_Delta and M_Delta at 200 times the mean density for the five most massive groups.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/sphere_profiles_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o sphere_profiles_example
// Exits non-zero if Domain::sphereProfiles and sphereProfilesGpu on the domain's octree disagree in a bit, if a count of
// the innermost bins is not what the host counts, or if one of the five has no resolved overdensity radius.
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

    std::mt19937 rng(42);
    std::normal_distribution<T> gauss(0.0, sigma);
    std::uniform_real_distribution<T> uni(0.0, 1.0);
    const T centers[numBlobs][3] = {{0.0, 0.0, 0.0}, {0.3, 0.7, 0.2}, {0.7, 0.3, 0.6}, {0.5, 0.5, 0.9}, {0.2, 0.2, 0.5}, {0.8, 0.8, 0.3}};
    std::discrete_distribution<int> pick({1, 2, 3, 4, 5, 6});
    std::vector<T> hx(n), hy(n), hz(n), hh(n, 0.01), hm(n);
    auto wrap = [](T v) { v -= std::floor(v); return v < 1.0 ? v : 0.0; };
    for (std::size_t i = 0; i < n; ++i)
    {
        hm[i] = (0.5 + uni(rng)) / double(n);
        if (i % 4 == 3) { hx[i] = uni(rng), hy[i] = uni(rng), hz[i] = uni(rng); }
        else
        {
            const int b = pick(rng);
            hx[i] = wrap(centers[b][0] + gauss(rng)), hy[i] = wrap(centers[b][1] + gauss(rng)), hz[i] = wrap(centers[b][2] + gauss(rng));
        }
    }
    auto dev = [n](const std::vector<T>& v) { return DeviceVector<T>(v.data(), v.data() + n); };
    DeviceVector<T> x = dev(hx), y = dev(hy), z = dev(hz), h = dev(hh), m = dev(hm), scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    Box<T> box(0, 1, BoundaryType::periodic);
    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f, box);
    domain.sync(keys, x, y, z, h, std::tie(m), scratch);

    const double b = 0.2 * std::cbrt(1.0 / double(n));
    DeviceVector<LocalIndex> labels, offsets, members;
    domain.friendsOfFriends(x, y, z, b, labels);
    const unsigned numGroups = fofCatalogGpu(labels.data(), domain.startIndex(), domain.endIndex(), minMembers, offsets, members);
    FofGroupTable<T> groups;
    domain.fofGroupProperties(x, y, z, m, static_cast<const DeviceVector<T>*>(nullptr), nullptr, nullptr, offsets, members, groups);

    // 16 bins from the centre out to 3 rms radii: the first from 0 (the overdensity finish asks for it), then logarithmic
    const int numBins = 16;
    std::vector<double> edges(numBins + 1, 0.0);
    for (int k = 1; k <= numBins; ++k)
        edges[k] = 3.0 * std::pow(0.3 / 3.0, double(numBins - k) / double(numBins - 1));

    SphereProfileTable profiles, profiles2;
    domain.sphereProfiles(x, y, z, &m, groups.center, &groups.radius, edges, profiles);
    sphereProfilesGpu(x.data(), y.data(), z.data(), m.data(), domain.startIndex(), domain.endIndex(), domain.box(),
                      domain.octreeProperties(), groups.center.data(), groups.radius.data(), numGroups, edges, profiles2);
    const auto counts = toHost(profiles.counts);
    const auto sums   = toHost(profiles.sums);
    const bool same   = toHost(profiles2.counts) == counts && toHost(profiles2.sums) == sums &&
                      toHost(profiles2.flags) == toHost(profiles.flags);

    // 200 times the mean density of the box (total mass over volume 1)
    const auto sm = toHost(m);
    const double rhoMean = std::accumulate(sm.begin(), sm.end(), 0.0);
    SphericalOverdensityTable so;
    sphericalOverdensityGpu(groups.radius.data(), numGroups, edges, profiles, 200.0 * rhoMean, so);
    const auto rDelta = toHost(so.radius), mDelta = toHost(so.mass);
    const auto soFlags = toHost(so.flags);
    const auto mass = toHost(groups.mass), center = toHost(groups.center), radius = toHost(groups.radius);

    // the host's count of the two innermost bins of every group, by the rule of include/cstone_hip.h
    const auto sx = toHost(x), sy = toHost(y), sz = toHost(z);
    unsigned miscounted = 0;
    for (unsigned g = 0; g < numGroups; ++g)
    {
        std::uint64_t inner[2] = {0, 0};
        const T e1 = radius[g] * T(edges[1]), e2 = radius[g] * T(edges[2]);
        for (std::size_t j = domain.startIndex(); j < domain.endIndex(); ++j)
        {
            T dx = sx[j] - center[3 * g], dy = sy[j] - center[3 * g + 1], dz = sz[j] - center[3 * g + 2];
            dx -= std::rint(dx), dy -= std::rint(dy), dz -= std::rint(dz); // (box length 1: len = inv = 1)
            const T d2 = dx * dx + dy * dy + dz * dz;
            if (d2 < e1 * e1) ++inner[0];
            else if (d2 < e2 * e2) ++inner[1];
        }
        miscounted += inner[0] != counts[std::size_t(g) * numBins] || inner[1] != counts[std::size_t(g) * numBins + 1];
    }

    std::vector<unsigned> byMass(numGroups);
    std::iota(byMass.begin(), byMass.end(), 0u);
    std::sort(byMass.begin(), byMass.end(), [&](unsigned a, unsigned c) { return mass[a] > mass[c]; });
    std::printf("sphere profiles: particles %zu, groups with at least %u members %u, %d bins out to 3 radii\n", n, minMembers,
                numGroups, numBins);
    unsigned unresolved = 0;
    for (unsigned r = 0; r < std::min(numGroups, 5u); ++r)
    {
        const unsigned g = byMass[r];
        std::printf("group %u: fof mass %.6f rms radius %.5f  R_200 %.5f M_200 %.6f flags %u\n", r, mass[g], radius[g], rDelta[g],
                    mDelta[g], soFlags[g]);
        unresolved += soFlags[g] != 0;
    }
    std::printf("sphereProfilesGpu on the domain's octree: %s; groups miscounted by the host's rule: %u; unresolved among the "
                "five: %u\n", same ? "identical" : "DIFFERENT", miscounted, unresolved);
    return (!same || miscounted || unresolved || numGroups < 5) ? 1 : 0;
}
