// lbvh_plan_test.cpp — the collapse plan of the device BVH builds
// (ARK_DDGI_FLAG_GPU_REBUILD_PLAN; lbvh_build.h planCosts / planCut and their serial
// restatement in lbvh_host.cpp). Stand-alone: built with the host BVH sources under
// AddressSanitizer + UndefinedBehaviorSanitizer and run as a program
// (tests/test_lbvh_plan_sanitizers.py). No GPU.
//  1. the plan against a brute force that enumerates every cut, on every binary tree over
//     2 .. 10 primitives, for a few random box sets and one coincident set: the eight costs of
//     the root equal by bits, and the cost of the members planCut emits, summed in the plan's
//     operand order (left then right, up the tree), equal to the root's word
//  2. the 257- and 4,099-triangle builds and the coincident build of lbvh_sah_test.cpp, world
//     and light, with the plan on
//  3. the rounds above the treelets on a class of one treelet, on a class with no upper node
//     and no treelet, and on a class with a single primitive outside every treelet
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "../../include/ark_ddgi_debug.h"
#include "lbvh_build.h"

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

namespace {
using namespace ark;

uint32_t bitsOf(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// every binary tree over the primitives [f, l] as split[] under the numbering (node: the range's node)
std::vector<std::vector<uint32_t>> trees(uint32_t f, uint32_t l, uint32_t node, uint32_t n)
{
    std::vector<std::vector<uint32_t>> out;
    if (f == l) {
        out.emplace_back(n, 0u);
        return out;
    }
    for (uint32_t s = f; s < l; ++s) {
        const auto A = trees(f, s, s, n), B = trees(s + 1u, l, s + 1u, n);
        for (const auto& a : A)
            for (const auto& b : B) {
                std::vector<uint32_t> t(n, 0u);
                for (uint32_t i = 0; i < n; ++i) t[i] = a[i] | b[i]; // disjoint node indices; index 0 is only ever the root's
                t[node] = s;
                out.push_back(t);
            }
    }
    return out;
}

struct Tree {
    uint32_t n;
    const std::vector<uint32_t>* split;
    const std::vector<uint32_t>* pbox; // 6 ordered words per primitive
    std::vector<uint32_t> picks;
    std::vector<float> cost; // [node][8]
    mutable std::vector<std::vector<std::pair<int, float>>> memo = {}; // cuts() by node
    void box(uint32_t f, uint32_t l, uint32_t b[6]) const
    {
        for (int c = 0; c < 6; ++c) b[c] = c < 3 ? ~0u : 0u;
        for (uint32_t p = f; p <= l; ++p)
            for (int c = 0; c < 3; ++c) {
                b[c] = std::min(b[c], (*pbox)[6 * p + c]);
                b[3 + c] = std::max(b[3 + c], (*pbox)[6 * p + 3 + c]);
            }
    }
    // the plan, bottom-up (what k_lbvh_treelet_sah's rounds and treeletSahHost do)
    void plan(uint32_t f, uint32_t l, uint32_t node, float C[8])
    {
        uint32_t b[6];
        box(f, l, b);
        if (f == l) return lbvh::planLeafCosts(b, C);
        const uint32_t s = (*split)[node];
        float L[8], R[8];
        plan(f, s, s, L);
        plan(s + 1u, l, s + 1u, R);
        picks[node] = lbvh::planCosts(lbvh::halfArea(b), l - f + 1u, L, R, C) | lbvh::kPlanDone;
        std::copy(C, C + 8, &cost[8 * node]);
    }
    // brute force: every cut below the range as (members, cost); a member's cost by memberCost
    float memberCost(uint32_t f, uint32_t l, uint32_t node) const
    {
        uint32_t b[6];
        box(f, l, b);
        const uint32_t cnt = l - f + 1u;
        if (cnt <= static_cast<uint32_t>(kBvh8MaxLeafSize)) return cnt == 1u ? lbvh::halfArea(b) * lbvh::kPlanTriCost : lbvh::halfArea(b) * lbvh::kPlanTriCost * static_cast<float>(cnt);
        const uint32_t s = (*split)[node];
        float best = __builtin_inff();
        for (const auto& a : cuts(f, s, s))
            for (const auto& c : cuts(s + 1u, l, s + 1u))
                if (a.first + c.first <= 8) best = std::min(best, a.second + c.second);
        return lbvh::halfArea(b) * lbvh::kPlanNodeCost + best;
    }
    std::vector<std::pair<int, float>> cuts(uint32_t f, uint32_t l, uint32_t node) const
    {
        if (memo.empty()) memo.resize(n);
        if (f != l && !memo[node].empty()) return memo[node];
        std::vector<std::pair<int, float>> out(1, { 1, memberCost(f, l, node) });
        if (f == l) return out;
        const uint32_t s = (*split)[node];
        for (const auto& a : cuts(f, s, s))
            for (const auto& c : cuts(s + 1u, l, s + 1u))
                if (a.first + c.first <= 8) out.push_back({ a.first + c.first, a.second + c.second });
        memo[node] = out;
        return out;
    }
    // the cost of a cut given as members in range order, summed up the tree: left then right
    float cutCost(uint32_t f, uint32_t l, uint32_t node, const lbvh::Member* m, int members, bool top, bool& ok) const
    {
        if (!top)
            for (int k = 0; k < members; ++k)
                if (m[k].r.first == f && m[k].r.last == l) {
                    uint32_t b[6];
                    box(f, l, b);
                    return f == l ? lbvh::halfArea(b) * lbvh::kPlanTriCost : cost[8 * node];
                }
        if (f == l) {
            ok = false; // a primitive no member covers
            return 0.0f;
        }
        const uint32_t s = (*split)[node];
        const float a = cutCost(f, s, s, m, members, false, ok);
        return a + cutCost(s + 1u, l, s + 1u, m, members, false, ok);
    }
};

int bruteForce()
{
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> pos(-4.0f, 4.0f), size(0.0f, 1.5f);
    uint64_t checked = 0;
    for (int set = 0; set < 4; ++set) {
        std::vector<uint32_t> pbox(6 * 10);
        for (uint32_t p = 0; p < 10; ++p)
            for (int c = 0; c < 3; ++c) {
                const float lo = set == 3 ? 1.0f + static_cast<float>(c) : pos(rng), hi = set == 3 ? 2.0f + 2.0f * static_cast<float>(c) : lo + size(rng);
                pbox[6 * p + c] = lbvh::ordered(lo);
                pbox[6 * p + 3 + c] = lbvh::ordered(hi);
            }
        for (uint32_t n = 2; n <= 10; ++n) {
            const auto all = trees(0u, n - 1u, 0u, n);
            for (const auto& split : all) {
                Tree t { n, &split, &pbox, std::vector<uint32_t>(n, 0u), std::vector<float>(8 * n, 0.0f) };
                float C[8];
                t.plan(0u, n - 1u, 0u, C);
                // the root's eight costs against the least cost of every cut of at most i members
                const auto cuts = t.cuts(0u, n - 1u, 0u);
                for (int i = 1; i <= 8; ++i) {
                    float best = __builtin_inff();
                    for (const auto& c : cuts)
                        if (c.first <= i) best = std::min(best, c.second);
                    CHECK(bitsOf(best) == bitsOf(C[i - 1]));
                }
                // the cut of the root as a BVH8 node
                lbvh::Member top, out[8];
                top.r.first = 0u;
                top.r.last = n - 1u;
                top.node = 0u;
                const int members = lbvh::planCut(split.data(), t.picks.data(), top, out);
                CHECK(members >= 1 && members <= 8);
                uint32_t next = 0;
                for (int k = 0; k < members; ++k) {
                    CHECK(out[k].r.first == next && out[k].r.last >= out[k].r.first && out[k].r.last < n);
                    next = out[k].r.last + 1u;
                }
                CHECK(next == n);
                if (n <= static_cast<uint32_t>(kBvh8MaxLeafSize)) {
                    CHECK(members == 1);
                } else {
                    CHECK(members >= 2);
                    bool ok = true;
                    uint32_t b[6];
                    t.box(0u, n - 1u, b);
                    const float sum = lbvh::halfArea(b) * lbvh::kPlanNodeCost + t.cutCost(0u, n - 1u, 0u, out, members, true, ok);
                    CHECK(ok);
                    CHECK(bitsOf(sum) == bitsOf(C[0]));
                }
                checked++;
            }
        }
    }
    std::printf("brute force: %llu trees\n", static_cast<unsigned long long>(checked));
    return 0;
}

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

int run(const char* name, const std::vector<float>& t, uint64_t minTreelets, bool coincident)
{
    const size_t n = t.size() / 9;
    uint64_t sah[11] = {}, plan[11] = {};
    CHECK(ark_ddgi_debug_lbvh_check_plan(t.data(), n, 1, 1, 0, sah) == 0);
    CHECK(ark_ddgi_debug_lbvh_check_plan(t.data(), n, 1, 1, 1, plan) == 0);
    CHECK(plan[3] == 0 && plan[4] == n && plan[8] >= minTreelets && plan[10] == 0 && sah[9] == 0);
    CHECK((plan[9] != 0) == (n > 3));
    if (coincident) CHECK(plan[2] <= 16);
    std::vector<float> origins;
    for (size_t i = 0; i < n; i += 7) origins.insert(origins.end(), t.begin() + 9 * i, t.begin() + 9 * i + 3);
    const float sun[3] = { 0.3f, -1.0f, -0.4f };
    uint64_t ls[19] = {};
    CHECK(ark_ddgi_debug_sun_lbvh_check_plan(t.data(), n, sun, origins.data(), origins.size() / 3, 1e30f, -1, 1, 1, ls) == 0);
    CHECK(ls[3] == 0 && ls[8] == 0 && ls[9] == 0 && ls[16] >= minTreelets && ls[18] == 0);
    std::printf("%s: %llu nodes, depth %llu, %llu treelets, BVH8 SAH cost %.3f (%.3f with the SAH pass alone); sun tree %llu nodes, %llu treelets\n", name,
                static_cast<unsigned long long>(plan[0]), static_cast<unsigned long long>(plan[2]), static_cast<unsigned long long>(plan[8]), plan[7] / 1e6,
                sah[7] / 1e6, static_cast<unsigned long long>(ls[6]), static_cast<unsigned long long>(ls[16]));
    return 0;
}

} // namespace

int main()
{
    if (bruteForce()) return 1;
    if (run("257", soup(257, false), 2, false)) return 1;
    if (run("4099", soup(4099, false), 2, false)) return 1;
    if (run("coincident", soup(300, true), 2, true)) return 1;
    // the rounds above the treelets
    if (run("one treelet", soup(200, false), 1, false)) return 1;
    if (run("no upper node, no treelet", soup(1, false), 0, false)) return 1;
    {
        // 256 triangles in one corner of the scene box and one in the opposite corner: the root
        // of the radix tree has the 256 (one treelet) and the single primitive as its children
        std::vector<float> t = soup(257, false);
        for (size_t i = 0; i < 256; ++i)
            for (int k = 0; k < 9; ++k) t[9 * i + k] = t[9 * i + k] / 64.0f - 30.0f;
        for (int k = 0; k < 9; ++k) t[9 * 256 + k] = 30.0f + 0.1f * static_cast<float>(k % 3) * static_cast<float>(k / 3);
        if (run("stray primitive", t, 1, false)) return 1;
    }
    std::printf("OK\n");
    return 0;
}
