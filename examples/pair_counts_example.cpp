// The two-point correlation function xi(r) of a clustered cloud in a periodic box, beside that of a uniform cloud of the
// same size, through the C++20 host layer on one MI355X: sync, Domain::pairCounts (the ordered pair counts DD(r) in radial
// bins, one shared traversal per 64 particles) and xiNatural, the natural estimator for a periodic box.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/pair_counts_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o pair_counts_example
// Exits non-zero if Domain::pairCounts and pairCountsGpu on the domain's octree disagree in a bit, if the cross counts
// about the particles' own positions are not the auto counts plus the n selves in the first bin, if the total of the counts
// is not what the kernel says it binned, or if the ordered counts of a bin are odd.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "cstone_amd/cstone_amd.hpp"

using namespace cstone_amd;

using KeyType = std::uint64_t;
using T       = double;

struct Result
{
    std::vector<std::uint64_t> counts;
    bool consistent;
    double testsPerPair;
};

//! DD(r) of a cloud in the periodic unit box, checked against the free calls on the domain's octree
static Result pairCountsOf(const std::vector<T>& hx, const std::vector<T>& hy, const std::vector<T>& hz,
                           const std::vector<double>& edges)
{
    const std::size_t n = hx.size();
    auto dev = [n](const std::vector<T>& v) { return DeviceVector<T>(v.data(), v.data() + n); };
    std::vector<T> hh(n, 0.01);
    DeviceVector<T> x = dev(hx), y = dev(hy), z = dev(hz), h = dev(hh), scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    Box<T> box(0, 1, BoundaryType::periodic);
    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 16, /*theta*/ 0.5f, box);
    domain.sync(keys, x, y, z, h, std::tie(), scratch);

    const DeviceVector<T>* none = nullptr;
    PairCountTable a, b, c;
    domain.pairCounts(x, y, z, none, edges, a, true);
    pairCountsGpu(x.data(), y.data(), z.data(), static_cast<const T*>(nullptr), domain.startIndex(), domain.endIndex(),
                  domain.startIndex(), domain.endIndex(), domain.box(), domain.octreeProperties(), edges, b);
    // the particles as their own queries, interleaved x, y, z: nothing is excluded, so every particle finds itself at d2 = 0
    const auto sx = toHost(x), sy = toHost(y), sz = toHost(z);
    std::vector<T> hq(3 * n);
    for (std::size_t i = 0; i < n; ++i)
        hq[3 * i] = sx[i], hq[3 * i + 1] = sy[i], hq[3 * i + 2] = sz[i];
    DeviceVector<T> q(hq.data(), hq.data() + 3 * n);
    domain.pairCountsCross(x, y, z, none, q, none, edges, c);

    Result r;
    r.counts         = toHost(a.counts);
    const auto cross = toHost(c.counts);
    r.consistent     = toHost(b.counts) == r.counts;
    std::uint64_t total = 0;
    for (std::size_t k = 0; k < r.counts.size(); ++k)
    {
        total += r.counts[k];
        r.consistent = r.consistent && r.counts[k] % 2 == 0 && cross[k] == r.counts[k] + (k == 0 && edges[0] == 0.0 ? n : 0);
    }
    r.consistent   = r.consistent && total == a.stats[1];
    r.testsPerPair = total ? double(a.stats[0]) / double(total) : 0.0;
    return r;
}

int main(int argc, char** argv)
{
    std::size_t n      = argc > 1 ? std::stoul(argv[1]) : 40000;
    const int numBlobs = 6;
    const T sigma      = 0.02;

    std::mt19937 rng(42);
    std::normal_distribution<T> gauss(0.0, sigma);
    std::uniform_real_distribution<T> uni(0.0, 1.0);
    const T centers[numBlobs][3] = {{0.0, 0.0, 0.0}, {0.3, 0.7, 0.2}, {0.7, 0.3, 0.6}, {0.5, 0.5, 0.9}, {0.2, 0.2, 0.5}, {0.8, 0.8, 0.3}};
    std::discrete_distribution<int> pick({1, 2, 3, 4, 5, 6});
    auto wrap = [](T v) { v -= std::floor(v); return v < 1.0 ? v : 0.0; };
    std::vector<T> cx(n), cy(n), cz(n), ux(n), uy(n), uz(n);
    for (std::size_t i = 0; i < n; ++i)
    {
        if (i % 4 == 3) { cx[i] = uni(rng), cy[i] = uni(rng), cz[i] = uni(rng); }
        else
        {
            const int b = pick(rng);
            cx[i] = wrap(centers[b][0] + gauss(rng)), cy[i] = wrap(centers[b][1] + gauss(rng)), cz[i] = wrap(centers[b][2] + gauss(rng));
        }
    }
    for (std::size_t i = 0; i < n; ++i)
        ux[i] = uni(rng), uy[i] = uni(rng), uz[i] = uni(rng);

    // the first bin from 0 (coincident particles and, for the cross counts, the selves), then 12 logarithmic bins
    const int numBins = 13;
    std::vector<double> edges(numBins + 1, 0.0);
    for (int k = 1; k <= numBins; ++k)
        edges[k] = 0.1 * std::pow(0.005 / 0.1, double(numBins - k) / double(numBins - 1));

    const Result clustered = pairCountsOf(cx, cy, cz, edges);
    const Result uniform   = pairCountsOf(ux, uy, uz, edges);
    const auto xiC = xiNatural(clustered.counts, edges, double(n), double(n - 1), 1.0);
    const auto xiU = xiNatural(uniform.counts, edges, double(n), double(n - 1), 1.0);

    std::printf("pair counts: particles %zu, %d bins out to %.3f; distance tests per pair binned: clustered %.2f, uniform %.2f\n", n,
                numBins, edges[numBins], clustered.testsPerPair, uniform.testsPerPair);
    const double fourPi3 = 4.0 * 3.14159265358979323846 / 3.0;
    for (int k = 0; k < numBins; ++k)
    {
        const double expected = double(n) * double(n - 1) * fourPi3 * (edges[k + 1] * edges[k + 1] * edges[k + 1] - edges[k] * edges[k] * edges[k]);
        std::printf("bin %2d [%.5f, %.5f) xi_clustered %.5f xi_uniform %.5f expected %.1f\n", k, edges[k], edges[k + 1], xiC[k], xiU[k],
                    expected);
    }
    const bool same = clustered.consistent && uniform.consistent;
    std::printf("pairCountsGpu and the cross counts about the particles on the domain's octree: %s\n", same ? "identical" : "DIFFERENT");
    return same ? 0 : 1;
}
