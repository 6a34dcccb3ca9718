// sun_policy_test.cpp — the rebuild policy with ARK_DDGI_FLAG_GPU_REBUILD_SUN
// (scene_rebuild_policy.h: SunDevice, the sun's settle rule, the turns with the world
// BVHs) as a table of rebuildToStart cases, against a copy of the policy as it stood before
// the flag for states without it; and the serial restatement of the device build of the
// sun's light-space BVH8 (ark_ddgi_debug_sun_lbvh_check) on 2,000 triangles. Stand-alone:
// built and run under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_sun_rebuild_policy.py. No GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scene_rebuild_policy.h"
#include "../../include/ark_ddgi.h"
#include "../../include/ark_ddgi_debug.h"

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

using namespace ark;
using S = RebuildStart;

namespace {

constexpr uint32_t kNoBg = ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD, kGpu = ARK_DDGI_FLAG_GPU_REBUILD, kGpuSun = ARK_DDGI_FLAG_GPU_REBUILD_SUN;

// rebuildToStart as it stood before ARK_DDGI_FLAG_GPU_REBUILD_SUN: what states without
// the bit must still get
S policyBefore(const RebuildState& q)
{
    const bool background = !(q.flags & ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD);
    bool sunMissing = false, sunLoosened = false;
    if (q.sunWanted && q.hasSun && !q.sunJobRunning && q.requestStable && !q.sunFailedHere) {
        sunMissing = !q.sunInstalled;
        sunLoosened = q.sunInstalled && q.sunRefitsSinceBuild != 0 && background;
    }
    if (sunMissing) return S::Sun;
    if (q.sunJobRunning || q.worldJobRunning) return S::None;
    const bool worldOk = background && !q.worldRebuildFailed;
    const bool worldLoosened = worldOk && q.refitsSinceBuild != 0;
    const bool worldSettle = worldOk && (q.flags & ARK_DDGI_FLAG_GPU_REBUILD) && q.worldGpuBuilt && q.refitsSinceBuild == 0;
    const bool world = !q.sunOnly && (worldLoosened || worldSettle);
    if (world && (!sunLoosened || q.lastBackground != kBackgroundWorld)) return worldLoosened && (q.flags & ARK_DDGI_FLAG_GPU_REBUILD) ? S::WorldDevice : S::WorldHost;
    const bool sunYields = q.sunOnly ? worldLoosened : world;
    if (sunLoosened && (!sunYields || q.lastBackground != kBackgroundSun)) return S::Sun;
    return S::None;
}

int withoutTheBit()
{
    // every combination of the booleans, three refit counts each, the four flag sets
    // without the new bit, the three last-background values; sunGpuBuilt either way (it
    // must not matter)
    uint64_t cases = 0;
    for (uint32_t bits = 0; bits < (1u << 11); ++bits)
        for (uint32_t refits = 0; refits < 4; ++refits)
            for (uint32_t flags : { 0u, kNoBg, kGpu, kNoBg | kGpu })
                for (uint8_t last : { kBackgroundNone, kBackgroundWorld, kBackgroundSun }) {
                    RebuildState q;
                    q.sunWanted = bits & 1u;
                    q.hasSun = bits & 2u;
                    q.sunJobRunning = bits & 4u;
                    q.worldJobRunning = bits & 8u;
                    q.sunInstalled = bits & 16u;
                    q.requestStable = bits & 32u;
                    q.sunFailedHere = bits & 64u;
                    q.worldRebuildFailed = bits & 128u;
                    q.worldGpuBuilt = bits & 256u;
                    q.sunGpuBuilt = bits & 512u;
                    q.sunOnly = bits & 1024u;
                    q.refitsSinceBuild = (refits & 1u) ? 3u : 0u;
                    q.sunRefitsSinceBuild = (refits & 2u) ? 2u : 0u;
                    q.flags = flags;
                    q.lastBackground = last;
                    const S got = rebuildToStart(q);
                    CHECK(got == policyBefore(q));
                    CHECK(got != S::SunDevice);
                    ++cases;
                }
    std::printf("without the bit: %llu states as before\n", static_cast<unsigned long long>(cases));
    return 0;
}

int withTheBit()
{
    RebuildState base;
    base.sunWanted = base.hasSun = base.sunInstalled = base.requestStable = true;
    base.flags = kGpuSun;
    CHECK(rebuildToStart(base) == S::None); // a host build installed, nothing loosened
    // missing: on the device, at once, also beside a running world rebuild; under the
    // conditions of the host start
    {
        RebuildState q = base;
        q.sunInstalled = false;
        CHECK(rebuildToStart(q) == S::SunDevice);
        q.worldJobRunning = true;
        CHECK(rebuildToStart(q) == S::SunDevice);
        q.flags = kGpuSun | kNoBg; // (a missing one is not a rebuild after refits)
        CHECK(rebuildToStart(q) == S::SunDevice);
        q.sunJobRunning = true;
        CHECK(rebuildToStart(q) == S::None);
        q = base;
        q.sunInstalled = false;
        q.requestStable = false;
        CHECK(rebuildToStart(q) == S::None);
        q.requestStable = true;
        q.sunWanted = false;
        CHECK(rebuildToStart(q) == S::None);
        q.sunWanted = true;
        q.hasSun = false;
        CHECK(rebuildToStart(q) == S::None);
    }
    // failure memory: not again for this direction and version, missing or loosened or settled
    {
        RebuildState q = base;
        q.sunFailedHere = true;
        q.sunInstalled = false;
        CHECK(rebuildToStart(q) == S::None);
        q.sunInstalled = true;
        q.sunRefitsSinceBuild = 4;
        CHECK(rebuildToStart(q) == S::None);
        q.sunRefitsSinceBuild = 0;
        q.sunGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::None);
        q.sunFailedHere = false;
        CHECK(rebuildToStart(q) == S::Sun);
    }
    // loosened: on the device, whichever builder the installed one had; not beside a
    // running job; not with NO_BACKGROUND_REBUILD
    {
        RebuildState q = base;
        q.sunRefitsSinceBuild = 2;
        CHECK(rebuildToStart(q) == S::SunDevice);
        q.sunGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::SunDevice);
        q.worldJobRunning = true;
        CHECK(rebuildToStart(q) == S::None);
        q.worldJobRunning = false;
        q.flags = kGpuSun | kNoBg;
        CHECK(rebuildToStart(q) == S::None);
    }
    // settle: a device build for this direction with no refit since its snapshot is
    // replaced by one host build, exactly once
    {
        RebuildState q = base;
        q.sunGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::Sun);
        q.sunJobRunning = true; // ... running
        CHECK(rebuildToStart(q) == S::None);
        q.sunJobRunning = false; // ... installed: a host build
        q.sunGpuBuilt = false;
        CHECK(rebuildToStart(q) == S::None);
        CHECK(rebuildToStart(q) == S::None);
        // a device build for another direction (not installed for the caller) is not settled but missing
        q.sunGpuBuilt = false;
        q.sunInstalled = false;
        CHECK(rebuildToStart(q) == S::SunDevice);
        // without the bit a device-built tree left from before stays
        q = base;
        q.flags = 0;
        q.sunGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::None);
    }
    // both bits, both loosened: the device builds take turns
    {
        RebuildState q = base;
        q.flags = kGpu | kGpuSun;
        q.refitsSinceBuild = q.sunRefitsSinceBuild = 3;
        for (int round = 0; round < 6; ++round) {
            const S got = rebuildToStart(q);
            CHECK(got == (round % 2 == 0 ? S::WorldDevice : S::SunDevice));
            q.lastBackground = got == S::SunDevice ? kBackgroundSun : kBackgroundWorld;
        }
        // the sun bit alone: the world's turn is a host build
        q.flags = kGpuSun;
        q.lastBackground = kBackgroundSun;
        CHECK(rebuildToStart(q) == S::WorldHost);
        q.lastBackground = kBackgroundWorld;
        CHECK(rebuildToStart(q) == S::SunDevice);
        // both settled: the two host rebuilds take turns too
        q = base;
        q.flags = kGpu | kGpuSun;
        q.worldGpuBuilt = q.sunGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::WorldHost);
        q.lastBackground = kBackgroundWorld;
        CHECK(rebuildToStart(q) == S::Sun);
        q.lastBackground = kBackgroundSun;
        CHECK(rebuildToStart(q) == S::WorldHost);
        // a settled sun beside a loosened world
        q.refitsSinceBuild = 2;
        q.sunRefitsSinceBuild = 0;
        q.lastBackground = kBackgroundWorld;
        CHECK(rebuildToStart(q) == S::Sun);
        q.lastBackground = kBackgroundSun;
        CHECK(rebuildToStart(q) == S::WorldDevice);
    }
    // sunOnly (set_lights): never a world build
    {
        RebuildState q = base;
        q.flags = kGpu | kGpuSun;
        q.sunOnly = true;
        q.refitsSinceBuild = 3;
        CHECK(rebuildToStart(q) == S::None);
        q.sunRefitsSinceBuild = 3;
        q.lastBackground = kBackgroundWorld;
        CHECK(rebuildToStart(q) == S::SunDevice);
        q.lastBackground = kBackgroundSun; // the sun's turn yields to the loosened world, which the next update starts
        CHECK(rebuildToStart(q) == S::None);
        q.sunInstalled = false;
        CHECK(rebuildToStart(q) == S::SunDevice);
        q = base;
        q.sunOnly = true;
        q.sunGpuBuilt = true;
        q.flags = kGpu | kGpuSun;
        q.worldGpuBuilt = true; // a world settle rebuild does not hold the sun's back there
        q.lastBackground = kBackgroundSun;
        CHECK(rebuildToStart(q) == S::Sun);
    }
    std::printf("with the bit: OK\n");
    return 0;
}

// 2,000 triangles through the serial restatement of the device build, both suns
int sunLbvh()
{
    const uint64_t n = 2000;
    std::vector<float> tris(9 * n), origins;
    uint64_t x = 0x2545F4914F6CDD1Dull;
    auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return static_cast<float>((x >> 11) * 0x1p-53);
    };
    for (uint64_t i = 0; i < n; ++i) {
        float v0[3];
        for (int a = 0; a < 3; ++a) v0[a] = -20.0f + 40.0f * next();
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) tris[9 * i + 3 * k + a] = v0[a] + (k ? -0.8f + 1.6f * next() : 0.0f);
        if (i % 8 == 0)
            for (int a = 0; a < 3; ++a) origins.push_back((tris[9 * i + a] + tris[9 * i + 3 + a] + tris[9 * i + 6 + a]) / 3.0f);
    }
    const float suns[2][3] = { { 0.3f, -1.0f, -0.4f }, { 0.0f, -1.0f, 0.0f } };
    for (const float* sun : { suns[0], suns[1] }) {
        uint64_t out[12] = {};
        const int rc = ark_ddgi_debug_sun_lbvh_check(tris.data(), n, sun, origins.data(), origins.size() / 3, 1e30f, out);
        CHECK(rc == 0);
        CHECK(out[0] == origins.size() / 3 && out[3] == 0 && out[8] == 0 && out[9] == 0 && out[6] > 1);
        std::printf("sun LBVH, 2,000 triangles: %llu nodes, %.2f steps per ray (host build %.2f)\n", static_cast<unsigned long long>(out[6]), out[10] * 1e-6, out[11] * 1e-6);
    }
    return 0;
}

} // namespace

int main()
{
    CHECK(withoutTheBit() == 0);
    CHECK(withTheBit() == 0);
    CHECK(sunLbvh() == 0);
    std::printf("OK\n");
    return 0;
}
