// Friends-of-friends groups with GLOBAL labels through the C++20 host layer: Domain::friendsOfFriendsGlobal, the call
// for a multi-rank domain, here on a communicator of one rank (which needs no collectives), beside the single-rank
// Domain::friendsOfFriends on the same cloud.  With one rank the global id of a particle is its index minus
// startIndex(), so the two must agree label by label and size by size, and two lowering passes are made.
//   g++ -std=c++20 -I include -I cornerstone-octree_amd/include examples/fof_mr_example.cpp \
//       -L cornerstone-octree_amd/lib -lcstone_hip -Wl,-rpath,$PWD/cornerstone-octree_amd/lib -o fof_mr_example
// With an application's collectives in cstone_hip_comm_ops (examples/domain_mpi_example.cpp shows MPI) the same call joins
// the groups across the ranks.  Exits non-zero if the two disagree.
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

    std::mt19937 rng(7);
    std::uniform_real_distribution<T> uni(0.0, 1.0);
    std::vector<T> hx(n), hy(n), hz(n);
    for (std::size_t i = 0; i < n; ++i)
        hx[i] = uni(rng), hy[i] = uni(rng), hz[i] = uni(rng);
    const double b = 0.9 * std::cbrt(1.0 / double(n));
    std::vector<T> hh(n, 0.6 * b); // halos (on several ranks) out to 2 h = 1.2 b: the linking length is covered

    auto synced = [&](auto& domain, DeviceVector<T>& x, DeviceVector<T>& y, DeviceVector<T>& z)
    {
        x = DeviceVector<T>(hx.data(), hx.data() + n), y = DeviceVector<T>(hy.data(), hy.data() + n);
        z = DeviceVector<T>(hz.data(), hz.data() + n);
        DeviceVector<T> h(hh.data(), hh.data() + n), scratch;
        DeviceVector<KeyType> keys(n);
        Context::check(cstone_hip_memset(Context::get(), keys.data(), 0, n * sizeof(KeyType)), "memset");
        domain.sync(keys, x, y, z, h, std::tie(), scratch);
    };

    Box<T> box(0, 1, BoundaryType::periodic);
    DeviceVector<T> x, y, z, x1, y1, z1;

    // the multi-rank domain on one rank: no collective is ever called
    cstone_hip_comm_ops noComm{};
    Domain<KeyType, T> global(0, 1, /*bucketSize*/ 1024, /*bucketSizeFocus*/ 64, /*theta*/ 0.5f, box, noComm);
    synced(global, x, y, z);
    DeviceVector<std::uint64_t> labels, sizes;
    unsigned rounds = 0;
    const std::uint64_t numGroups = global.friendsOfFriendsGlobal(x, y, z, b, labels, &sizes, &rounds);

    // the single-rank domain and its 32-bit labels
    Domain<KeyType, T> local(0, 1, 1024, 64, 0.5f, box);
    synced(local, x1, y1, z1);
    DeviceVector<LocalIndex> labels1;
    DeviceVector<unsigned> sizes1;
    const unsigned numGroups1 = local.friendsOfFriends(x1, y1, z1, b, labels1, &sizes1);

    const auto hl = toHost(labels), hs = toHost(sizes);
    const auto hl1 = toHost(labels1);
    const auto hs1 = toHost(sizes1);
    const LocalIndex s = global.startIndex(), s1 = local.startIndex();
    bool same = numGroups == numGroups1 && global.nParticles() == local.nParticles() && toHost(x) == toHost(x1);
    std::uint64_t largest = 0;
    for (std::size_t i = 0; same && i < hl1.size(); ++i)
    {
        same    = hl[s + i] == hl1[i] - s1 && hs[s + i] == hs1[i];
        largest = std::max<std::uint64_t>(largest, hs[s + i]);
    }
    std::printf("fof_mr: particles %zu, linking length %.6f, groups %llu, largest %llu, rounds %u\n", hl1.size(), b,
                (unsigned long long)numGroups, (unsigned long long)largest, rounds);
    std::printf("global labels against Domain::friendsOfFriends: %s\n", same ? "identical" : "DIFFERENT");
    return (same && rounds == 2) ? 0 : 1;
}
