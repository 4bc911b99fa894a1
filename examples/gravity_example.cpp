// Barnes-Hut gravity through the C++20 host layer on one MI355X: sync, expansion centres, accelerations.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/gravity_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o gravity_example
// The particles follow a closed form (an additive recurrence in [0, 1)^3, masses 1 / n) so that another client can
// rebuild them exactly; the rows printed at the end are compared with the Python binding by tests/test_gravity.py.
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
    std::size_t n = argc > 1 ? std::stoul(argv[1]) : 20000;
    const T eps   = 0.01;

    std::vector<T> hx(n), hy(n), hz(n), hh(n, 0.01), hm(n, T(1) / T(n));
    for (std::size_t i = 0; i < n; ++i)
    {
        hx[i] = std::fmod(T(i) * 0.7548776662466927 + 0.1, 1.0);
        hy[i] = std::fmod(T(i) * 0.5698402909980532 + 0.2, 1.0);
        hz[i] = std::fmod(T(i) * 0.3819660112501051 + 0.3, 1.0);
    }
    DeviceVector<T> x(hx.data(), hx.data() + n), y(hy.data(), hy.data() + n), z(hz.data(), hz.data() + n),
        h(hh.data(), hh.data() + n), m(hm.data(), hm.data() + n), scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");

    Domain<KeyType, T> domain(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f);
    // Domain::syncGrav on one rank: sync with the masses as a property, then the expansion centres of the new tree
    domain.sync(keys, x, y, z, h, std::tie(m), scratch);
    domain.updateExpansionCenters(x, y, z, m);

    DeviceVector<T> ax, ay, az, phi;
    domain.computeGravity(x, y, z, m, ax, ay, az, &phi, T(1), eps);
    auto hax = toHost(ax), hay = toHost(ay), haz = toHost(az), hphi = toHost(phi);
    std::printf("gravity: %zu particles, %u after sync, %d focus leaves\n", n, domain.endIndex(),
                domain.view().num_focus_leaves);
    T sum = 0;
    for (std::size_t i = 0; i < hax.size(); ++i)
        sum += std::sqrt(hax[i] * hax[i] + hay[i] * hay[i] + haz[i] * haz[i]);
    std::printf("mean |a|: %.6e\n", sum / T(hax.size()));
    for (std::size_t i : {std::size_t(0), hax.size() / 3, 2 * hax.size() / 3, hax.size() - 1})
        std::printf("row %zu %.17g %.17g %.17g %.17g\n", i, hax[i], hay[i], haz[i], hphi[i]);
    return 0;
}
