// rt_shadows_test.cpp — csrc/rt_shadows_host.cpp on its own (tests/test_rt_shadows_sanitizers.py
// builds both with -fsanitize=address,undefined): the host restatement of the local-light
// shadow masks over random depth planes, 1 x 1 and 1 x 97 images, 16 lights, a light at a
// shading point (the NaN rule: not traced, lit), an all-sky plane, hole records and
// instances outside the class table; every mask byte is written, inside its plane only,
// and the counts add up to the pixels.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rt_shadows.h"
#include "rt_shadows_host.h"

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

static const float kIdentity[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };

struct Case {
    uint32_t w = 0, h = 0;
    std::vector<float> depth;
    std::vector<ArkRtShadowLight> lights;
    std::vector<std::vector<uint8_t>> masks; // each h * w bytes between two guard bytes
    ArkRtShadowsDesc desc(uint32_t frame)
    {
        masks.assign(lights.size(), std::vector<uint8_t>(static_cast<size_t>(w) * h + 2, 0x5a));
        for (size_t l = 0; l < lights.size(); ++l) lights[l].out_mask = masks[l].data() + 1;
        ArkRtShadowsDesc d {};
        d.struct_size = sizeof(d);
        d.width = w;
        d.height = h;
        d.frame_index = frame;
        std::memcpy(d.world_from_view, kIdentity, sizeof(kIdentity));
        std::memcpy(d.view_from_projection, kIdentity, sizeof(kIdentity));
        d.depth = depth.data();
        d.lights = lights.data();
        d.light_count = static_cast<uint32_t>(lights.size());
        return d;
    }
};

static ArkRtShadowLight light(float x, float y, float z, float dx, float dy, float dz, float cone, float radius)
{
    ArkRtShadowLight l {};
    l.position[0] = x, l.position[1] = y, l.position[2] = z;
    l.direction[0] = dx, l.direction[1] = dy, l.direction[2] = dz;
    l.outer_cone_angle_cos = cone;
    l.source_radius = radius;
    return l;
}

// records: a quad at z = 0.7 over [-0.5, 0.5]^2 per class (instances 0, 1, 2), a hole and a
// record of an instance past the class table
static std::vector<uint32_t> records()
{
    std::vector<uint32_t> r;
    auto add = [&](const float v0[3], const float e1[3], const float e2[3], uint32_t inst) {
        uint32_t w[12] = {};
        std::memcpy(w, v0, 12);
        std::memcpy(w + 3, e1, 12);
        std::memcpy(w + 6, e2, 12);
        w[9] = inst;
        w[10] = static_cast<uint32_t>(r.size() / 12);
        r.insert(r.end(), w, w + 12);
    };
    for (uint32_t c = 0; c < 3; ++c) {
        const float z = 0.7f + 0.05f * c, x0 = -0.5f + 0.4f * c;
        const float a[3] = { x0, -0.5f, z }, b[3] = { x0 + 0.3f, 0.5f, z }, e1[3] = { 0.3f, 0.0f, 0.0f }, e2[3] = { 0.0f, 1.0f, 0.0f }, m1[3] = { -0.3f, 0.0f, 0.0f },
                    m2[3] = { 0.0f, -1.0f, 0.0f };
        add(a, e1, e2, c);
        add(b, m1, m2, c);
    }
    const float zero[3] = { 0, 0, 0 };
    add(zero, zero, zero, 0xffffffffu);
    const float big[3] = { 100.0f, 0.0f, 0.0f }, bigm[3] = { -100.0f, -100.0f, 0.0f };
    add(bigm, big, big, 7u);
    return r;
}

static void run(Case& c, uint32_t frame, uint32_t classMask, const char* name, std::vector<uint64_t>* countsOut = nullptr)
{
    const std::vector<uint32_t> rec = records();
    const int32_t classOf[3] = { 0, 1, 2 };
    ArkRtShadowsDesc d = c.desc(frame);
    std::vector<uint64_t> counts(4 * c.lights.size() + 1, 0xdeadbeefull);
    const int rc = rtshadow::hostShadows(rec.data(), rec.size() / 12, classOf, 3, classMask, d, counts.data());
    CHECK(rc == 0, "%s: rc %d", name, rc);
    CHECK(counts.back() == 0xdeadbeefull, "%s: counts overrun", name);
    const uint64_t pixels = static_cast<uint64_t>(c.w) * c.h;
    for (size_t l = 0; l < c.lights.size(); ++l) {
        CHECK(c.masks[l].front() == 0x5a && c.masks[l].back() == 0x5a, "%s: light %zu wrote outside its mask", name, l);
        uint64_t lit = 0;
        for (uint64_t p = 0; p < pixels; ++p) {
            const uint8_t b = c.masks[l][1 + p];
            CHECK(b == 0 || b == 255, "%s: light %zu pixel %llu byte %u", name, l, static_cast<unsigned long long>(p), b);
            lit += b == 255;
        }
        const uint64_t* k = &counts[4 * l];
        CHECK(k[0] + k[1] + k[2] + k[3] == pixels, "%s: light %zu counts %llu", name, l, static_cast<unsigned long long>(k[0] + k[1] + k[2] + k[3]));
        CHECK(k[2] == lit, "%s: light %zu lit %llu, mask has %llu", name, l, static_cast<unsigned long long>(k[2]), static_cast<unsigned long long>(lit));
    }
    counts.pop_back();
    if (countsOut) *countsOut = counts;
}

int main()
{
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    // random depth planes: with identity matrices the shading point is (ndc.xy, depth)
    for (int it = 0; it < 6; ++it) {
        Case c;
        c.w = 5 + static_cast<uint32_t>(rng() % 40);
        c.h = 3 + static_cast<uint32_t>(rng() % 70);
        c.depth.resize(static_cast<size_t>(c.w) * c.h);
        for (float& v : c.depth) v = uni(rng) < 0.1f ? 1.0f : 0.5f * uni(rng);
        c.lights = { light(0.0f, 0.0f, 2.0f, 0.0f, 0.0f, -1.0f, 0.5f, 0.05f), light(0.8f, 0.1f, 1.5f, -0.5f, 0.0f, -0.86f, 0.9f, 0.3f) };
        std::vector<uint64_t> c1, c7;
        run(c, static_cast<uint32_t>(it), 1u, "random planes, opaque only", &c1);
        run(c, static_cast<uint32_t>(it), 7u, "random planes, every class", &c7);
        CHECK(c7[3] >= c1[3] && c7[7] >= c1[7], "more occluding classes, fewer occluded pixels");
        if (it == 0) CHECK(c1[3] > 0 && c7[3] > c1[3] && c1[2] > 0 && c1[0] > 0, "the planes do not exercise every class: %llu %llu", static_cast<unsigned long long>(c1[3]), static_cast<unsigned long long>(c7[3]));
    }
    { // 1 x 1 and 1 x 97
        Case c;
        c.w = c.h = 1;
        c.depth = { 0.25f };
        c.lights = { light(0.0f, 0.0f, 2.0f, 0.0f, 0.0f, -1.0f, 0.5f, 0.05f) };
        run(c, 3, 1u, "1 x 1");
        c.w = 1;
        c.h = 97;
        c.depth.assign(97, 0.3f);
        c.depth[40] = 1.0f;
        run(c, 3, 7u, "1 x 97");
    }
    { // 16 lights
        Case c;
        c.w = 16;
        c.h = 16;
        c.depth.resize(256);
        for (float& v : c.depth) v = 0.5f * uni(rng);
        for (int l = 0; l < 16; ++l) c.lights.push_back(light(-0.8f + 0.1f * l, 0.3f, 1.5f + 0.05f * l, 0.0f, 0.0f, -1.0f, 0.3f, 0.02f * (l + 1)));
        run(c, 7, 1u, "16 lights");
        ArkRtShadowsDesc d = c.desc(0);
        d.light_count = 17;
        CHECK(rtshadow::descProblem(d) != nullptr, "17 lights accepted");
    }
    { // a light at a shading point: normalize(0) is NaN, the ray is not traced and is lit
        Case c;
        c.w = c.h = 1;
        c.depth = { 0.25f };
        c.lights = { light(0.0f, 0.0f, 0.25f, 0.0f, 0.0f, -1.0f, 0.5f, 0.05f) };
        std::vector<uint64_t> k;
        run(c, 0, 7u, "light at the shading point", &k);
        CHECK(k[2] == 1 && c.masks[0][1] == 255, "the NaN rule: counts %llu %llu %llu %llu", static_cast<unsigned long long>(k[0]), static_cast<unsigned long long>(k[1]),
              static_cast<unsigned long long>(k[2]), static_cast<unsigned long long>(k[3]));
        // n.z == 0: the basis is not finite, the same rule
        c.lights = { light(0.7f, 0.0f, 0.25f, -1.0f, 0.0f, 0.0f, 0.5f, 0.05f) };
        run(c, 0, 7u, "light level with the shading point", &k);
        CHECK(k[2] == 1, "n.z == 0: counts %llu %llu %llu %llu", static_cast<unsigned long long>(k[0]), static_cast<unsigned long long>(k[1]), static_cast<unsigned long long>(k[2]),
              static_cast<unsigned long long>(k[3]));
    }
    { // all sky, and NaN depth (not sky: the comparison is false)
        Case c;
        c.w = 9;
        c.h = 20;
        c.depth.assign(180, 1.0f);
        c.lights = { light(0.0f, 0.0f, 2.0f, 0.0f, 0.0f, -1.0f, 0.5f, 0.05f), light(0.5f, 0.0f, 2.0f, 0.0f, 0.0f, -1.0f, 0.5f, 0.05f) };
        std::vector<uint64_t> k;
        run(c, 1, 1u, "all sky", &k);
        CHECK(k[0] == 180 && k[4] == 180, "all sky: %llu", static_cast<unsigned long long>(k[0]));
        c.depth.assign(180, std::nanf(""));
        run(c, 1, 1u, "NaN depth", &k);
        CHECK(k[0] == 0, "NaN depth counted as sky");
    }
    { // refusals
        Case c;
        c.w = c.h = 2;
        c.depth.assign(4, 0.5f);
        c.lights = { light(0, 0, 2, 0, 0, -1, 0.5f, 0.05f), light(0, 0, 2, 0, 0, -1, 0.5f, 0.05f) };
        ArkRtShadowsDesc d = c.desc(0);
        CHECK(rtshadow::descProblem(d) == nullptr, "a good descriptor refused");
        c.lights[1].out_mask = c.lights[0].out_mask;
        CHECK(rtshadow::descProblem(d) != nullptr, "repeated mask accepted");
        d = c.desc(0);
        c.lights[0].source_radius = INFINITY;
        CHECK(rtshadow::descProblem(d) != nullptr, "infinite radius accepted");
        d = c.desc(0);
        c.lights[0].source_radius = 0.05f;
        d.depth = nullptr;
        CHECK(rtshadow::hostShadows(nullptr, 0, nullptr, 0, 1, d, nullptr) == -1, "no depth accepted");
        d = c.desc(0);
        d.width = 1u << 14;
        d.height = 1u << 14;
        CHECK(rtshadow::descProblem(d) != nullptr, "2^28 pixels accepted");
    }
    std::printf(failures ? "%d failures\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
