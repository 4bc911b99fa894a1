// The host-only rules of the k-nearest-neighbour calls (csrc/knn.hpp: the refusals of cstone_hip_knn, the list registers
// per k, the chunk rule of cstone_hip_domain_mr_knn) and the absolute margin of the node tests (csrc/node_margin.hpp)
// called from a plain host program, so that they can run under the sanitizers without a GPU:
//   g++ -std=c++20 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I cornerstone-octree_amd/csrc \
//       tools/knn_rules_check.cpp -o knn_rules_check && ./knn_rules_check
// Exits non-zero at the first rule that does not hold.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "knn.hpp"

using namespace cship;

static int failures = 0;
static void expect(bool ok, const char* what)
{
    if (!ok) std::printf("FAILED: %s\n", what), ++failures;
}

int main()
{
    // refusals, in the order the header gives them; nothing is looked at behind the first that applies
    expect(knnRefusal(32, 1, 0, 0, 0, false) == nullptr, "no queries: pointers are not looked at");
    expect(knnRefusal(64, CSTONE_KNN_MAX_K, 5, 5, 9, true) == nullptr, "k = max, empty range");
    expect(knnRefusal(16, 8, 0, 1, 1, true) != nullptr && knnRefusal(0, 8, 0, 1, 1, true) != nullptr, "real_bits");
    expect(knnRefusal(32, 0, 0, 1, 1, true) != nullptr && knnRefusal(32, CSTONE_KNN_MAX_K + 1, 0, 1, 1, true) != nullptr &&
               knnRefusal(32, 0xFFFFFFFFu, 0, 1, 0, true) != nullptr,
           "k out of range, also without queries");
    expect(knnRefusal(32, 8, 10, 9, 0, true) != nullptr, "last < first");
    expect(knnRefusal(32, 8, 0, 1, 1, false) != nullptr, "null pointer with queries");
    expect(std::strcmp(knnRefusal(16, 0, 10, 9, 1, false), "real_bits unsupported") == 0, "real_bits is judged first");

    for (uint32_t k = 1; k <= CSTONE_KNN_MAX_K; ++k)
    {
        const int r = knnListRegisters(k);
        expect((r == 1 || r == 2 || r == 4) && 64u * r >= k && (r == 1 || 64u * (r / 2) < k || (r == 4 && k > 128)), "list registers");
    }

    // the chunk rule: never 0 with queries, never above Q, under the cap unless one query alone exceeds it, and maximal
    const uint64_t caps[] = {1, 16, 47, 4096, 16384, 1ull << 20, CSTONE_KNN_MR_GATHER_BYTES, 1ull << 40,
                             std::numeric_limits<uint64_t>::max()};
    const uint32_t qs[] = {1, 2, 40, 65, 1000000, std::numeric_limits<uint32_t>::max()};
    const int ps[]      = {1, 2, 3, 64, 4096, std::numeric_limits<int>::max()};
    for (uint64_t cap : caps)
        for (uint32_t q : qs)
            for (int p : ps)
                for (uint32_t k : {1u, 8u, 100u, 256u})
                {
                    const uint32_t per = knnChunkQueries(q, k, p, cap);
                    const __uint128_t one = __uint128_t(16) * k * uint64_t(p);
                    expect(per >= 1 && per <= q, "chunk within 1 .. Q");
                    expect(per * one <= cap || per == 1, "chunk under the cap");
                    expect(per == q || (per + __uint128_t(1)) * one > cap, "chunk maximal");
                }
    expect(knnChunkQueries(0, 8, 2, 4096) == 0 && knnChunkQueries(5, 0, 2, 4096) == 0 && knnChunkQueries(5, 8, 0, 4096) == 0,
           "degenerate arguments give 0");
    expect(knnChunkQueries(40, 100, 3, 16384) == 3 && knnChunkQueries(40, 256, 3, 4096) == 1, "the chunks of the tests");

    cstone_box box{};
    const double lim[6] = {-1.3, 2.1, 0.2, 0.9, -5, 7};
    std::memcpy(box.lim, lim, sizeof lim);
    expect(nodeAbsMargin<float>(box, 64) == float(64.0 * 1.1920928955078125e-07 * 12.0), "margin f32: L = the z length");
    expect(nodeAbsMargin<double>(box, 64) == 64.0 * 2.220446049250313e-16 * 12.0, "margin f64");
    expect(nodeAbsMargin<float>(box, 256) == float(256.0 * 1.1920928955078125e-07 * 12.0) &&
               nodeAbsMargin<double>(box, 256) == 256.0 * 2.220446049250313e-16 * 12.0,
           "margin of the pair counts: the factor 256");

    std::printf("knn rules: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
