// Adaptive smoothing lengths through the C++20 host layer on one MI355X: sync, then every particle's h iterated inside
// one kernel to 100 +- 10 neighbours.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/adapt_h_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o adapt_h_example
// The particles follow a closed form (an additive recurrence in [0, 1)^3); h starts at the value that gives 100 neighbours
// at the mean density, off by up to 20 % either way.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "cstone_amd/cstone_amd.hpp"

using namespace cstone_amd;

int main(int argc, char** argv)
{
    using KeyType = std::uint64_t;
    using T       = double;
    std::size_t n = argc > 1 ? std::stoul(argv[1]) : 50000;
    const unsigned ng0 = 100, tol = 10, maxIter = 10;

    const T h0 = 0.5 * std::cbrt(3.0 * ng0 / (4.0 * 3.14159265358979323846 * T(n)));
    std::vector<T> hx(n), hy(n), hz(n), hh(n);
    for (std::size_t i = 0; i < n; ++i)
    {
        hx[i] = std::fmod(T(i) * 0.7548776662466927 + 0.1, 1.0);
        hy[i] = std::fmod(T(i) * 0.5698402909980532 + 0.2, 1.0);
        hz[i] = std::fmod(T(i) * 0.3819660112501051 + 0.3, 1.0);
        hh[i] = h0 * (0.8 + 0.4 * std::fmod(T(i) * 0.6180339887498949, 1.0));
    }
    DeviceVector<T> x(hx.data(), hx.data() + n), y(hy.data(), hy.data() + n), z(hz.data(), hz.data() + n),
        h(hh.data(), hh.data() + n), scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    // periodic, so that every particle can reach its count
    Box<T> box(0, 1, BoundaryType::periodic);
    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f, box);
    domain.sync(keys, x, y, z, h, std::tie(), scratch);

    // the same search through the free function, on a copy of the synced h: range, tree view and box spelled out
    auto hSynced = toHost(h);
    DeviceVector<T> h2(hSynced.data(), hSynced.data() + hSynced.size());
    DeviceVector<unsigned> counts2(domain.nParticles()), status2(domain.nParticles());

    DeviceVector<unsigned> counts, status;
    domain.adaptSmoothingLengths(x, y, z, h, ng0, tol, maxIter, /*growLimit: none*/ 0.0f, counts, status);
    adaptSmoothingLengthsGpu(x.data(), y.data(), z.data(), h2.data(), domain.startIndex(), domain.endIndex(), domain.box(),
                             domain.octreeProperties(), ng0, tol, maxIter, INFINITY, counts2.data(), status2.data());
    auto hs = toHost(status), hc = toHost(counts);
    auto hn = toHost(h);

    std::size_t converged = 0, notConverged = 0, capped = 0, stalled = 0, walks = 0;
    T hsum = 0;
    for (std::size_t i = 0; i < hs.size(); ++i)
    {
        walks += hs[i] & AdaptStatus::walksMask;
        notConverged += (hs[i] & AdaptStatus::notConverged) != 0;
        capped += (hs[i] & AdaptStatus::capped) != 0;
        stalled += (hs[i] & AdaptStatus::stalled) != 0;
        converged += (hs[i] & ~AdaptStatus::walksMask) == 0;
        hsum += hn[domain.startIndex() + i];
    }
    std::printf("adapt_h: particles %zu, ng0 %u +- %u, mean walks %.2f, mean h %.6f (start %.6f)\n", hs.size(), ng0, tol,
                double(walks) / double(hs.size()), hsum / T(hs.size()), h0);
    std::printf("converged %zu not_converged %zu capped %zu stalled %zu\n", converged, notConverged, capped, stalled);
    std::printf("first counts: %u %u %u %u\n", hc[0], hc[1], hc[2], hc[3]);
    const bool same = toHost(h2) == hn && toHost(counts2) == hc && toHost(status2) == hs;
    std::printf("adaptSmoothingLengthsGpu on the domain's tree view: %s\n", same ? "identical" : "DIFFERENT");
    if (!same) return 1;
    return 0;
}
