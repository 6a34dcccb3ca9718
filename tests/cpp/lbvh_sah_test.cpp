// lbvh_sah_test.cpp — the serial restatement of the SAH pass of the device BVH builds
// (ARK_DDGI_FLAG_GPU_REBUILD_SAH; lbvh_host.cpp build_lbvh_host with the pass, through
// ark_ddgi_debug_lbvh_check_sah and ark_ddgi_debug_sun_lbvh_check_sah) on 257 and 4,099
// triangles of a soup (two treelets under one upper node; many) and on 300 coincident
// triangles (equal boxes: the tie rule). Stand-alone: built with the host BVH sources under
// AddressSanitizer + UndefinedBehaviorSanitizer and run as a program
// (tests/test_lbvh_sah_sanitizers.py). No GPU.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/ark_ddgi_debug.h"

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

namespace {

std::vector<float> soup(size_t n, bool coincident)
{
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> pos(-31.0f, 31.0f), edge(-0.3f, 0.3f);
    std::vector<float> t(9 * n);
    for (size_t i = 0; i < n; ++i) {
        if (coincident && i > 0) {
            for (int k = 0; k < 9; ++k) t[9 * i + k] = t[k];
            continue;
        }
        for (int a = 0; a < 3; ++a) {
            t[9 * i + a] = pos(rng);
            t[9 * i + 3 + a] = t[9 * i + a] + edge(rng);
            t[9 * i + 6 + a] = t[9 * i + a] + edge(rng);
        }
    }
    return t;
}

int run(const char* name, size_t n, bool coincident)
{
    const std::vector<float> t = soup(n, coincident);
    uint64_t plain[9] = {}, sah[9] = {};
    CHECK(ark_ddgi_debug_lbvh_check_sah(t.data(), n, 1, 0, plain) == 0);
    CHECK(ark_ddgi_debug_lbvh_check_sah(t.data(), n, 1, 1, sah) == 0);
    CHECK(sah[3] == 0 && sah[4] == n && sah[8] >= 2 && plain[8] == 0);
    if (coincident) CHECK(sah[2] <= 16);
    // a sun shadow ray from a vertex of every 7th triangle
    std::vector<float> origins;
    for (size_t i = 0; i < n; i += 7) origins.insert(origins.end(), t.begin() + 9 * i, t.begin() + 9 * i + 3);
    const float sun[3] = { 0.3f, -1.0f, -0.4f };
    uint64_t ls[17] = {};
    CHECK(ark_ddgi_debug_sun_lbvh_check_sah(t.data(), n, sun, origins.data(), origins.size() / 3, 1e30f, -1, 1, ls) == 0);
    CHECK(ls[3] == 0 && ls[8] == 0 && ls[9] == 0 && ls[16] >= 2);
    std::printf("%s: %llu nodes, depth %llu, %llu treelets, BVH8 SAH cost %.3f (%.3f without the pass); sun tree %llu nodes, %llu treelets\n", name,
                static_cast<unsigned long long>(sah[0]), static_cast<unsigned long long>(sah[2]), static_cast<unsigned long long>(sah[8]), sah[7] / 1e6,
                plain[7] / 1e6, static_cast<unsigned long long>(ls[6]), static_cast<unsigned long long>(ls[16]));
    return 0;
}

} // namespace

int main()
{
    if (run("257", 257, false)) return 1;
    if (run("4099", 4099, false)) return 1;
    if (run("coincident", 300, true)) return 1;
    std::printf("OK\n");
    return 0;
}
