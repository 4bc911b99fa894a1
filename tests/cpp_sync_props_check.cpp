// Stand-alone check for tests/test_cpp_sync_props.py: the single-rank Domain::sync of the C++ host layer with THREE
// properties.  The library exchanges buffers among x, y, z, h, the scratch vector and the properties, and the layer
// rebinds every vector to the buffer it got back: each property must come back in its own vector, following its
// particle.  Property a holds the particle's index, b = 2 a + 0.5, c = -a.
#include <cstdio>
#include <random>
#include <vector>

#include "cstone_amd/cstone_amd.hpp"

using namespace cstone_amd;

int main()
{
    using KeyType = std::uint64_t;
    using T       = double;
    const std::size_t n = 5000;
    std::mt19937 rng(7);
    std::uniform_real_distribution<T> uni(0.0, 1.0);
    std::vector<T> hx(n), hy(n), hz(n), hh(n, 0.01), ha(n), hb(n), hc(n);
    for (std::size_t i = 0; i < n; ++i)
    {
        hx[i] = uni(rng), hy[i] = uni(rng), hz[i] = uni(rng);
        ha[i] = T(i), hb[i] = 2 * T(i) + 0.5, hc[i] = -T(i);
    }
    auto dev = [n](const std::vector<T>& v) { return DeviceVector<T>(v.data(), v.data() + n); };
    DeviceVector<T> x = dev(hx), y = dev(hy), z = dev(hz), h = dev(hh), a = dev(ha), b = dev(hb), c = dev(hc), scratch;
    DeviceVector<KeyType> keys(n);
    Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");
    Box<T> box(0, 1);
    Domain<KeyType, T> domain(0, 1, 1024, 64, 0.5f, box);
    unsigned bad = 0;
    for (int step = 0; step < 2; ++step) // (the second sync takes the exchanged buffers as its input)
    {
        domain.sync(keys, x, y, z, h, std::tie(a, b, c), scratch);
        const auto px = toHost(x), pa = toHost(a), pb = toHost(b), pc = toHost(c);
        bad += px.size() != n || pa.size() != n || pb.size() != n || pc.size() != n;
        bad += a.data() == b.data() || a.data() == c.data() || b.data() == c.data();
        for (std::size_t i = 0; i < n && !bad; ++i)
        {
            const std::size_t j = std::size_t(pa[i]);
            bad += j >= n || px[i] != hx[j] || pb[i] != 2 * pa[i] + 0.5 || pc[i] != -pa[i];
        }
    }
    std::printf(bad ? "SYNC_PROPS FAIL\n" : "SYNC_PROPS OK: 3 properties, 2 syncs\n");
    return bad ? 1 : 0;
}
