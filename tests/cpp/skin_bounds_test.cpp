// skin_bounds_test.cpp — csrc/skinning_host.cpp on its own (tests/test_skin_bounds_sanitizers.py
// builds both with -fsanitize=address,undefined): the host bound of a pose holds every
// position the restatement of k_skin_vertices produces, for random and adversarial poses,
// and every refusal of registration and of a pose returns its error and leaves the
// registry as it was.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "skinning_host.h"

using namespace ark;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++failures;                                      \
        }                                                    \
    } while (0)

struct SkinData {
    std::vector<float> positions;
    std::vector<ArkRTVertex> vertices;
    std::vector<ArkSkinningVertex> skinning;
    std::vector<ArkMorphTargetVertex> morph;
    uint32_t n = 0, joints = 0, K = 0;
    bool skeleton = true;
    ArkDdgiSkinDesc desc() const
    {
        ArkDdgiSkinDesc d {};
        d.struct_size = sizeof(d);
        d.vertex_count = n;
        d.joint_count = skeleton ? joints : 0;
        d.morph_target_count = K;
        d.positions = positions.data();
        d.vertices = vertices.data();
        d.skinning = skeleton ? skinning.data() : nullptr;
        d.morph_targets = K ? morph.data() : nullptr;
        return d;
    }
};

static std::mt19937_64 rng(0x5eed);
static float uni(float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }

// weightSum: every vertex's weights sum to it; influences: non-zero weights per vertex
static SkinData makeSkin(uint32_t n, uint32_t joints, uint32_t K, bool skeleton, float weightSum, int influences, uint32_t unusedJoint = ~0u)
{
    SkinData s;
    s.n = n, s.joints = joints, s.K = K, s.skeleton = skeleton;
    s.positions.resize(3 * n);
    s.vertices.resize(n);
    s.skinning.resize(n);
    s.morph.resize(static_cast<size_t>(K) * n);
    for (float& p : s.positions) p = uni(-2.0f, 2.0f);
    for (ArkRTVertex& v : s.vertices) {
        v = ArkRTVertex {};
        v.normal[1] = 1.0f;
        v.tangent[0] = v.tangent[3] = 1.0f;
    }
    for (ArkMorphTargetVertex& m : s.morph)
        for (int a = 0; a < 3; ++a) m.position[a] = uni(-0.5f, 0.5f), m.normal[a] = uni(-0.1f, 0.1f), m.tangent[a] = uni(-0.1f, 0.1f);
    for (ArkSkinningVertex& k : s.skinning) {
        float sum = 0.0f;
        for (int q = 0; q < 4; ++q) {
            uint32_t j = static_cast<uint32_t>(rng() % joints);
            if (j == unusedJoint) j = (j + 1u) % joints;
            k.joint_indices[q] = j;
            k.joint_weights[q] = q < influences ? uni(0.1f, 1.0f) : 0.0f;
            sum += k.joint_weights[q];
        }
        for (int q = 0; q < 4; ++q) k.joint_weights[q] = k.joint_weights[q] / sum * weightSum;
    }
    return s;
}

// a random rotation (about a random axis) times `scale`, translated by up to `translate`, as 12 floats
static void randomJoint(float* J, float scale, float translate)
{
    float k[3] = { uni(-1, 1), uni(-1, 1), uni(-1, 1) };
    const float len = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]) + 1e-6f;
    for (float& x : k) x /= len;
    const float a = uni(-3.1f, 3.1f), c = std::cos(a), s = std::sin(a);
    const float R[9] = { c + k[0] * k[0] * (1 - c),        k[0] * k[1] * (1 - c) - k[2] * s, k[0] * k[2] * (1 - c) + k[1] * s,
                         k[1] * k[0] * (1 - c) + k[2] * s, c + k[1] * k[1] * (1 - c),        k[1] * k[2] * (1 - c) - k[0] * s,
                         k[2] * k[0] * (1 - c) - k[1] * s, k[2] * k[1] * (1 - c) + k[0] * s, c + k[2] * k[2] * (1 - c) };
    for (int r = 0; r < 3; ++r) {
        for (int col = 0; col < 3; ++col) J[4 * r + col] = R[3 * r + col] * scale;
        J[4 * r + 3] = uni(-translate, translate);
    }
}

// the bound of the pose holds every restated position; returns the bound's largest extent
static void checkPose(const char* what, const SkinData& d, float scale, float translate, float morphLo, float morphHi)
{
    const ArkDdgiSkinDesc desc = d.desc();
    std::unique_ptr<skin::SkinHost> h;
    std::string why;
    CHECK(skin::buildSkin(&desc, h, why) == 0, "%s: %s", what, why.c_str());
    if (!h) return;
    std::vector<float> J(12 * std::max<uint32_t>(1, d.joints)), mw(std::max<uint32_t>(1, d.K));
    for (uint32_t j = 0; j < d.joints; ++j) randomJoint(&J[12 * j], scale, translate);
    for (float& m : mw) m = uni(morphLo, morphHi);
    float b[6];
    CHECK(skin::poseBound(*h, J.data(), mw.data(), b, why), "%s: %s", what, why.c_str());
    std::vector<float> P(3 * d.n), V(9 * d.n), vel(3 * d.n);
    skin::skinRun(*h, J.data(), mw.data(), nullptr, P.data(), V.data(), vel.data());
    uint32_t outside = 0;
    for (uint32_t i = 0; i < d.n; ++i)
        for (int a = 0; a < 3; ++a) outside += !(P[3 * i + a] >= b[a] && P[3 * i + a] <= b[3 + a]);
    CHECK(outside == 0, "%s: %u coordinates outside [%g %g %g, %g %g %g]", what, outside, b[0], b[1], b[2], b[3], b[4], b[5]);
    // a second run's velocity is the difference
    std::vector<float> P2(3 * d.n);
    skin::skinRun(*h, J.data(), mw.data(), P.data(), P2.data(), V.data(), vel.data());
    for (float v : vel) CHECK(v == 0.0f, "%s: the same pose twice has a velocity", what);
}

static void bounds()
{
    for (int round = 0; round < 20; ++round) {
        checkPose("random", makeSkin(257, 7, 2, true, 1.0f, 4), uni(0.5f, 2.0f), 3.0f, -1.0f, 1.0f);
        checkPose("random, no morph targets", makeSkin(100, 3, 0, true, 1.0f, 3), uni(0.5f, 2.0f), 3.0f, 0.0f, 0.0f);
        checkPose("translations of 1e4", makeSkin(129, 5, 1, true, 1.0f, 4), 1.0f, 1e4f, -1.0f, 1.0f);
        checkPose("scales of 1e-3", makeSkin(129, 5, 1, true, 1.0f, 4), 1e-3f, 1.0f, -1.0f, 1.0f);
        checkPose("scales of 1e3", makeSkin(129, 5, 1, true, 1.0f, 4), 1e3f, 1.0f, -1.0f, 1.0f);
        checkPose("weight sums of 0.9", makeSkin(129, 5, 1, true, 0.9f, 4), 1.5f, 2.0f, -1.0f, 1.0f);
        checkPose("weight sums of 1.1", makeSkin(129, 5, 1, true, 1.1f, 4), 1.5f, 2.0f, -1.0f, 1.0f);
        checkPose("negative morph weights", makeSkin(129, 5, 3, true, 1.0f, 4), 1.0f, 2.0f, -3.0f, -0.5f);
        checkPose("a vertex on one joint only", makeSkin(129, 5, 1, true, 1.0f, 1), 1.5f, 50.0f, -1.0f, 1.0f);
        checkPose("a joint no vertex uses", makeSkin(129, 5, 1, true, 1.0f, 4, 2u), 1.5f, 50.0f, -1.0f, 1.0f);
        checkPose("morph only", makeSkin(129, 1, 3, false, 1.0f, 4), 1.0f, 0.0f, -2.0f, 2.0f);
    }
    // mixed weight sums in one skin, and a vertex whose weights are all zero (it lands on the origin)
    SkinData d = makeSkin(64, 4, 1, true, 1.0f, 4);
    for (uint32_t i = 0; i < d.n; ++i)
        for (float& w : d.skinning[i].joint_weights) w *= (i & 1u) ? 0.9f : 1.1f;
    for (float& w : d.skinning[5].joint_weights) w = 0.0f;
    for (int round = 0; round < 20; ++round) checkPose("weight sums from 0 to 1.1", d, 1.5f, 100.0f, -1.0f, 1.0f);
}

static void refusals()
{
    skin::Registry reg;
    std::string why;
    uint32_t h = 77;
    const SkinData good = makeSkin(40, 4, 2, true, 1.0f, 4);
    ArkDdgiSkinDesc gd = good.desc();
    CHECK(reg.add(&gd, &h, why) == 0 && h == 0 && reg.live() == 1, "a good skin registers");

    auto refused = [&](const char* what, const SkinData& s, uint32_t structSize = sizeof(ArkDdgiSkinDesc)) {
        ArkDdgiSkinDesc d = s.desc();
        d.struct_size = structSize;
        uint32_t out = 99;
        why.clear();
        const int rc = reg.add(&d, &out, why);
        CHECK(rc == ARK_DDGI_E_INVALID_ARGUMENT && !why.empty(), "%s: rc %d", what, rc);
        CHECK(out == 99 && reg.live() == 1 && reg.skins.size() == 1 && reg.get(0), "%s: the registry changed", what);
    };
    SkinData s = good;
    s.skinning[7].joint_weights[2] = NAN;
    refused("a NaN weight", s);
    s = good;
    s.skinning[7].joint_weights[0] = INFINITY;
    refused("an infinite weight", s);
    s = good;
    s.skinning[9].joint_weights[1] = -0.01f;
    refused("a negative weight", s);
    s = good;
    s.skinning[39].joint_indices[3] = 4;
    refused("a joint index = joint_count", s);
    s = good;
    s.skinning[0].joint_indices[0] = 0xffffffffu;
    refused("a joint index of ~0", s);
    s = good;
    s.positions[17] = INFINITY;
    refused("a non-finite bind position", s);
    s = good;
    s.vertices[3].normal[1] = NAN;
    refused("a non-finite bind normal", s);
    s = good;
    s.morph[41].position[2] = NAN;
    refused("a non-finite morph delta", s);
    s = good;
    s.morph[79].tangent[0] = -INFINITY;
    refused("a non-finite morph tangent", s);
    s = good;
    s.joints = 0;
    refused("a skeleton without joints", s);
    s = good;
    s.skeleton = false;
    s.K = 0;
    refused("neither skeleton nor morph targets", s);
    refused("a wrong struct_size", good, 16);
    s = good;
    s.n = 0;
    refused("no vertices", s);
    {
        uint32_t out = 99;
        CHECK(reg.add(nullptr, &out, why) == ARK_DDGI_E_INVALID_ARGUMENT && reg.live() == 1, "a null desc");
        CHECK(reg.add(&gd, nullptr, why) == ARK_DDGI_E_INVALID_ARGUMENT && reg.live() == 1 && reg.skins.size() == 1, "a null handle");
    }

    // poses: non-finite joint matrices or morph weights, a bound that is not finite
    const skin::SkinHost* sk = reg.get(0);
    std::vector<float> J(12 * 4), mw(2, 0.5f);
    for (uint32_t j = 0; j < 4; ++j) randomJoint(&J[12 * j], 1.0f, 1.0f);
    float b[6];
    CHECK(skin::poseBound(*sk, J.data(), mw.data(), b, why), "a good pose");
    std::vector<float> bad = J;
    bad[12 * 3 + 7] = NAN;
    CHECK(!skin::poseBound(*sk, bad.data(), mw.data(), b, why), "a NaN joint matrix");
    bad = J;
    bad[0] = INFINITY;
    CHECK(!skin::poseBound(*sk, bad.data(), mw.data(), b, why), "an infinite joint matrix");
    std::vector<float> badw = mw;
    badw[1] = NAN;
    CHECK(!skin::poseBound(*sk, J.data(), badw.data(), b, why), "a NaN morph weight");
    bad = J;
    for (float& x : bad) x *= 3e38f; // finite matrices whose bound overflows fp32
    CHECK(!skin::poseBound(*sk, bad.data(), mw.data(), b, why), "a bound that is not finite");
    CHECK(reg.live() == 1 && reg.get(0) == sk, "poses do not touch the registry");

    // handles are not reused; removing twice fails
    uint32_t h2 = 0;
    CHECK(reg.add(&gd, &h2, why) == 0 && h2 == 1 && reg.live() == 2, "a second skin");
    CHECK(reg.remove(0) && !reg.get(0) && reg.get(1) && reg.live() == 1, "remove");
    CHECK(!reg.remove(0) && !reg.remove(5), "remove twice / unknown");
    uint32_t h3 = 0;
    CHECK(reg.add(&gd, &h3, why) == 0 && h3 == 2, "handles are not reused");
}

int main()
{
    bounds();
    refusals();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
