// A k-nearest-neighbour density estimate at probe points, through the C++20 host layer on one MI355X: sync a few Gaussian
// blobs over a thin background in a periodic box, ask for the k = 32 nearest particles of 2 000 probe points (half of them
// at random, half inside the blobs) and print  rho_k = (mass of the k nearest) / (4 pi / 3 r_k^3)  for a few of them.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/knn_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o knn_example
// Exits non-zero if Domain::nearestNeighbors and knnGpu on the domain's octree disagree in a bit, or if a row differs
// from the host's brute force by the rule of include/cstone_hip.h (sorted by squared distance, then index).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "cstone_amd/cstone_amd.hpp"

using namespace cstone_amd;

int main(int argc, char** argv)
{
    using KeyType = std::uint64_t;
    using T       = double;
    std::size_t n = argc > 1 ? std::stoul(argv[1]) : 40000;
    const std::size_t numProbes = 2000;
    const unsigned k            = 32;
    const int numBlobs          = 6;
    const T sigma               = 0.02;

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
    std::vector<T> hq(3 * numProbes);
    for (std::size_t q = 0; q < numProbes; ++q)
    {
        const int b = pick(rng);
        for (int a = 0; a < 3; ++a)
            hq[3 * q + a] = q % 2 ? uni(rng) : wrap(centers[b][a] + gauss(rng));
    }
    auto dev = [n](const std::vector<T>& v) { return DeviceVector<T>(v.data(), v.data() + n); };
    DeviceVector<T> x = dev(hx), y = dev(hy), z = dev(hz), h = dev(hh), m = dev(hm), scratch;
    DeviceVector<T> probes(hq.data(), hq.data() + hq.size());
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    Box<T> box(0, 1, BoundaryType::periodic);
    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f, box);
    domain.sync(keys, x, y, z, h, std::tie(m), scratch);

    KnnTable<T> table, table2;
    domain.nearestNeighbors(x, y, z, probes, nullptr, nullptr, k, table);
    knnGpu(x.data(), y.data(), z.data(), domain.startIndex(), domain.endIndex(), domain.box(), domain.octreeProperties(),
           probes.data(), static_cast<const T*>(nullptr), static_cast<const unsigned*>(nullptr), numProbes, k, table2);
    const auto nb = toHost(table.neighbors);
    const auto d2 = toHost(table.dist2);
    const auto cn = toHost(table.counts);
    const bool same = toHost(table2.neighbors) == nb && toHost(table2.dist2) == d2 && toHost(table2.counts) == cn;

    // the host's brute force by the rule: (d2, index) ascending, the first k (box length 1: len = inv = 1)
    const auto sx = toHost(x), sy = toHost(y), sz = toHost(z), sm = toHost(m);
    unsigned differ = 0;
    std::vector<std::pair<T, unsigned>> all(domain.endIndex() - domain.startIndex());
    for (std::size_t q = 0; q < numProbes; q += 10)
    {
        for (std::size_t j = domain.startIndex(); j < domain.endIndex(); ++j)
        {
            T dx = sx[j] - hq[3 * q], dy = sy[j] - hq[3 * q + 1], dz = sz[j] - hq[3 * q + 2];
            dx -= std::rint(dx), dy -= std::rint(dy), dz -= std::rint(dz);
            all[j - domain.startIndex()] = {dx * dx + dy * dy + dz * dz, unsigned(j)};
        }
        std::partial_sort(all.begin(), all.begin() + k, all.end());
        bool ok = cn[q] == k;
        for (unsigned e = 0; e < k; ++e)
            ok = ok && nb[q * k + e] == all[e].second && d2[q * k + e] == all[e].first;
        differ += !ok;
    }

    std::printf("knn density: particles %zu, probes %zu, k %u\n", n, numProbes, k);
    const double fourPi3 = 4.0 * 3.14159265358979323846 / 3.0;
    for (std::size_t q = 0; q < 6; ++q)
    {
        double mass = 0;
        for (unsigned e = 0; e < k; ++e)
            mass += sm[nb[q * k + e]];
        const double rk = std::sqrt(double(d2[q * k + k - 1]));
        std::printf("probe %zu at (%.3f %.3f %.3f): r_k %.5f rho_k %.4f (mean density 1)\n", q, hq[3 * q], hq[3 * q + 1],
                    hq[3 * q + 2], rk, mass / (fourPi3 * rk * rk * rk));
    }
    std::printf("knnGpu on the domain's octree: %s; probes that differ from the host's brute force: %u\n",
                same ? "identical" : "DIFFERENT", differ);
    return (!same || differ) ? 1 : 0;
}
