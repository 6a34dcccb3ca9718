// ASan + UBSan run of the host-side code on the path (SURVEY §5 "race detection /
// sanitizers"): the CPU oracle (frames with offsets, the blend alone on planted surfels, the
// AO bake, lighting compose),
// the synthetic soup generator and the BVH2 -> BVH8 builder with its structural check,
// the three hit-mask classes' build (build_world_bvh8) and the refit's level order, the
// LBVH restatement with the canonical tree comparison (compare_bvh8_canonical), and
// the background rebuilds' scheduling and what follows a job's device build
// (scene_rebuild_policy.h, two tables of cases).
// Built by tests/test_sanitizers.py with g++ -fsanitize=address,undefined
// -fno-sanitize-recover=all; any report aborts with a non-zero status.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh8_check.h"
#include "bvh_builder.h"
#include "scene_rebuild_policy.h"
#include "../../include/ark_ddgi.h"
#include "../../include/ark_ddgi_debug.h"
#include "../../include/ark_scene.h"

extern "C" {
void* oracle_create(const ArkDdgiDesc* desc);
void oracle_destroy(void* ctx);
int oracle_set_scene(void* ctx, const ArkDdgiScene* s, int threads);
int oracle_update(void* ctx, const ArkDdgiFrameParams* p, int threads);
int oracle_blend(void* ctx, const ArkDdgiFrameParams* p, int threads);
struct OracleShadeHit {
    uint32_t instance, primitive;
    float u, v, t;
};
int oracle_shade(void* ctx, const ArkDdgiFrameParams* p, const OracleShadeHit* hits, int threads);
int oracle_write(void* ctx, int which, const void* src, uint64_t bytes);
int oracle_read(void* ctx, int which, void* dst, uint64_t bytes);
int oracle_bake_ao(void* ctx, uint32_t instance, uint32_t W, uint32_t H, uint32_t samples, int bent, uint32_t row0, uint32_t row1,
                   uint32_t* triOut, uint16_t* baryOut, uint8_t* out, int threads);
}

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// build_world_bvh8 over the first `n` soup triangles dealt to the hit-mask classes:
// triangle 0 alone in class `single`, the others alternating between the two other
// classes, or all in one of them (`emptyClass`: the other stays empty); 4 threads.
static int worldBvh8Case(const std::vector<float>& tri, uint32_t n, int single, bool emptyClass)
{
    using namespace ark;
    std::vector<BuildTriangle> cls[3];
    std::vector<int> classOf(n);
    const int other[2] = { (single + 1) % 3, (single + 2) % 3 };
    for (uint32_t i = 0; i < n; ++i) {
        BuildTriangle t;
        std::memcpy(t.v0, &tri[9 * i], 12);
        std::memcpy(t.v1, &tri[9 * i + 3], 12);
        std::memcpy(t.v2, &tri[9 * i + 6], 12);
        t.instance = i; // one instance per triangle: classOf by record
        t.primitive = i;
        t.flip_facing = 0;
        classOf[i] = i == 0 ? single : other[emptyClass ? 0 : i & 1];
        cls[classOf[i]].push_back(t);
    }
    uint64_t count[3];
    for (int c = 0; c < 3; ++c) count[c] = cls[c].size();
    BvhBuildOptions opt;
    opt.threads = 4;
    Bvh8CollapseOptions copt;
    copt.threads = 4;
    WorldBvh8 w;
    std::string why;
    CHECK(build_world_bvh8(cls, opt, copt, w, why));
    CHECK(cls[0].empty() && cls[1].empty() && cls[2].empty()); // each class's input freed
    CHECK(w.triangles == n && w.maxLeaf >= 1 && w.maxLeaf <= static_cast<uint32_t>(kBvh8MaxLeafSize) && w.inflateAbs > 0.0f && !w.tooLarge);
    for (int c = 0; c < 3; ++c) CHECK((w.roots[c] >= 0) == (count[c] > 0));
    CHECK(checkBvh8Structure(w.nodes, w.tris, w.roots, 3, why));
    const Bvh8CheckResult chk = check_bvh8_full(w.nodes, w.tris, w.roots, 3, &classOf, nullptr);
    CHECK(chk.violations == 0 && chk.triangles == n && chk.nodes == w.nodes.size());
    // the refit's level order: every node once, the levels' offsets ascending to the count
    std::vector<uint32_t> order, offsets;
    CHECK(bvhLevelOrder(w.nodes.data(), w.nodes.size(), w.roots, 3, order, offsets));
    std::vector<uint8_t> seen(w.nodes.size(), 0);
    CHECK(order.size() == w.nodes.size());
    for (uint32_t node : order) {
        CHECK(node < seen.size() && !seen[node]);
        seen[node] = 1;
    }
    CHECK(offsets.size() == chk.maxDepth + 1u && offsets.front() == 0 && offsets.back() == order.size());
    for (size_t l = 0; l + 1 < offsets.size(); ++l) CHECK(offsets[l] < offsets[l + 1]);
    // the opaque class's nodes: from its root to the next root (or the end)
    if (w.roots[0] >= 0) {
        const int32_t next = w.roots[1] >= 0 ? w.roots[1] : w.roots[2] >= 0 ? w.roots[2] : static_cast<int32_t>(w.nodes.size());
        CHECK(w.opaqueNodes == static_cast<uint32_t>(next - w.roots[0]));
    } else {
        CHECK(w.opaqueNodes == 0);
    }
    std::printf("world bvh8: %u triangles in classes %llu/%llu/%llu, %zu nodes, depth %u\n", n, static_cast<unsigned long long>(count[0]),
                static_cast<unsigned long long>(count[1]), static_cast<unsigned long long>(count[2]), w.nodes.size(), w.depth);
    return 0;
}

// Which background BVH build a scene call starts (scene_rebuild_policy.h), case by case.
static int rebuildPolicyCases()
{
    using namespace ark;
    using S = RebuildStart;
    const uint32_t kNoBg = ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD, kGpu = ARK_DDGI_FLAG_GPU_REBUILD;
    // a context with a sun whose light-space BVH is installed, the request stable
    RebuildState base;
    base.sunWanted = base.hasSun = base.sunInstalled = base.requestStable = true;
    CHECK(rebuildToStart(base) == S::None); // nothing loosened
    RebuildState both = base; // world and sun both loosened
    both.refitsSinceBuild = both.sunRefitsSinceBuild = 3;

    // turn-taking: the world first, then strict alternation (each job collected before the next call)
    {
        RebuildState q = both;
        for (int round = 0; round < 6; ++round) {
            const S got = rebuildToStart(q);
            CHECK(got == (round % 2 == 0 ? S::WorldHost : S::Sun));
            q.lastBackground = got == S::Sun ? kBackgroundSun : kBackgroundWorld;
        }
        // only one of them loosened: it starts whatever started last
        for (uint8_t last : { kBackgroundNone, kBackgroundWorld, kBackgroundSun }) {
            q = both;
            q.lastBackground = last;
            q.sunRefitsSinceBuild = 0;
            CHECK(rebuildToStart(q) == S::WorldHost);
            q = both;
            q.lastBackground = last;
            q.refitsSinceBuild = 0;
            CHECK(rebuildToStart(q) == S::Sun);
        }
    }
    // a job is running: nothing loosened starts; a missing sun BVH starts beside a world
    // job, not beside a sun job
    for (int running = 0; running < 2; ++running) {
        RebuildState q = both;
        (running ? q.sunJobRunning : q.worldJobRunning) = true;
        CHECK(rebuildToStart(q) == S::None);
        q.sunInstalled = false;
        CHECK(rebuildToStart(q) == (running ? S::None : S::Sun));
    }
    // a missing sun BVH starts at once, ahead of a loosened world whose turn it is
    {
        RebuildState q = both;
        q.sunInstalled = false;
        q.lastBackground = kBackgroundSun;
        CHECK(rebuildToStart(q) == S::Sun);
        // ... but only on a stable request for this direction, with no remembered failure,
        // a sun, and a scene that chose the light-space BVH: else the world's turn
        RebuildState r = q;
        r.requestStable = false; // a streak below 2, or a request for another direction
        CHECK(rebuildToStart(r) == S::WorldHost);
        r.refitsSinceBuild = 0;
        CHECK(rebuildToStart(r) == S::None);
        r = q;
        r.sunFailedHere = true;
        CHECK(rebuildToStart(r) == S::WorldHost);
        r.refitsSinceBuild = 0;
        CHECK(rebuildToStart(r) == S::None);
        r = q;
        r.hasSun = false;
        CHECK(rebuildToStart(r) == S::WorldHost);
        r = q;
        r.sunWanted = false;
        CHECK(rebuildToStart(r) == S::WorldHost);
    }
    // an unstable request or a remembered failure also holds back a loosened sun BVH
    {
        RebuildState q = both;
        q.refitsSinceBuild = 0;
        q.requestStable = false;
        CHECK(rebuildToStart(q) == S::None);
        q = both;
        q.refitsSinceBuild = 0;
        q.sunFailedHere = true;
        CHECK(rebuildToStart(q) == S::None);
    }
    // ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD: nothing loosened starts, a missing sun BVH does
    {
        RebuildState q = both;
        q.flags = kNoBg;
        CHECK(rebuildToStart(q) == S::None);
        q.flags = kNoBg | kGpu;
        q.worldGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::None);
        q.refitsSinceBuild = 0; // (no settle rebuild either)
        CHECK(rebuildToStart(q) == S::None);
        q.sunInstalled = false;
        CHECK(rebuildToStart(q) == S::Sun);
    }
    // ARK_DDGI_FLAG_GPU_REBUILD: loosened world BVHs on the device; settled ones the device
    // built once on the host; neither after a failed rebuild
    {
        RebuildState q = base;
        q.flags = kGpu;
        q.refitsSinceBuild = 2;
        CHECK(rebuildToStart(q) == S::WorldDevice);
        q.worldGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::WorldDevice);
        q.refitsSinceBuild = 0;
        CHECK(rebuildToStart(q) == S::WorldHost); // the settle rebuild
        q.worldGpuBuilt = false;                  // ... installed: a host build, nothing more
        CHECK(rebuildToStart(q) == S::None);
        q = base;
        q.flags = kGpu;
        q.worldRebuildFailed = true;
        q.refitsSinceBuild = 2;
        CHECK(rebuildToStart(q) == S::None);
        q.refitsSinceBuild = 0;
        q.worldGpuBuilt = true;
        CHECK(rebuildToStart(q) == S::None);
        // without the flag a loosened world builds on the host
        q = base;
        q.refitsSinceBuild = 2;
        CHECK(rebuildToStart(q) == S::WorldHost);
        q.worldRebuildFailed = true;
        CHECK(rebuildToStart(q) == S::None);
        // a settle rebuild takes turns with a loosened sun BVH like a loosened world
        q = base;
        q.flags = kGpu;
        q.worldGpuBuilt = true;
        q.sunRefitsSinceBuild = 1;
        q.lastBackground = kBackgroundWorld;
        CHECK(rebuildToStart(q) == S::Sun);
        q.lastBackground = kBackgroundSun;
        CHECK(rebuildToStart(q) == S::WorldHost);
    }
    // sunOnly (set_lights): the world never starts; the sun's loosened turn yields to a
    // loosened world as in the full path: not twice in a row (there the world, offered
    // the turn first, also takes it when nothing has started yet)
    for (uint8_t last : { kBackgroundNone, kBackgroundWorld, kBackgroundSun }) {
        RebuildState q = both;
        q.lastBackground = last;
        CHECK(rebuildToStart(q) == (last == kBackgroundWorld ? S::Sun : S::WorldHost));
        q.sunOnly = true;
        CHECK(rebuildToStart(q) == (last == kBackgroundSun ? S::None : S::Sun));
        q.sunRefitsSinceBuild = 0; // only the world loosened
        CHECK(rebuildToStart(q) == S::None);
        q.flags = kGpu;
        CHECK(rebuildToStart(q) == S::None);
        q.sunInstalled = false; // a missing sun BVH
        CHECK(rebuildToStart(q) == S::Sun);
        q.worldJobRunning = true;
        CHECK(rebuildToStart(q) == S::Sun);
    }
    std::printf("rebuild policy: OK\n");
    return 0;
}

// How a rebuild job goes on after its device build (scene_rebuild_policy.h), all eight
// inputs: installed only when every HIP call succeeded and the build declined nothing (a
// fault flag beside a success cannot come from a hipError_t and changes nothing then);
// else a device fault fails the job; everything else - a decline, a HIP error that is not
// a device fault, both - is the host's.
static int deviceBuildOutcomeCases()
{
    using namespace ark;
    using O = DeviceBuildOutcome;
    const struct {
        bool hipOk, deviceFault, declined;
        O want;
    } cases[] = {
        { true, false, false, O::Installed },
        { true, false, true, O::HostBuild },  // no records, 4 GiB, depth, node scratch
        { false, false, false, O::HostBuild }, // e.g. out of memory
        { false, false, true, O::HostBuild },
        { false, true, false, O::Failed },
        { false, true, true, O::Failed },
        { true, true, false, O::Installed },
        { true, true, true, O::Failed },
    };
    int seen = 0;
    for (const auto& c : cases) {
        CHECK(deviceBuildOutcome(c.hipOk, c.deviceFault, c.declined) == c.want);
        seen |= 1 << (c.hipOk * 4 + c.deviceFault * 2 + c.declined);
    }
    CHECK(seen == 0xff); // every combination once
    std::printf("device build outcome: OK\n");
    return 0;
}

int main()
{
    CHECK(rebuildPolicyCases() == 0);
    CHECK(deviceBuildOutcomeCases() == 0);
    ArkSoupParams sp;
    ark_soup_default_params(&sp);
    sp.triangle_count = 4096;
    sp.extent = 6.0f;
    ArkSoupScene* soup = nullptr;
    CHECK(ark_soup_generate(&sp, &soup) == 0);
    const ArkDdgiScene* scene = ark_soup_scene_view(soup);

    // BVH8 build + structural check over the soup's world-space triangles
    std::vector<float> tri(static_cast<size_t>(scene->index_count) * 3);
    uint64_t nTri = 0;
    for (uint32_t mi = 0; mi < scene->mesh_count; ++mi) {
        const ArkRTTriangleMesh& m = scene->meshes[mi];
        const uint64_t end = mi + 1 < scene->mesh_count ? static_cast<uint64_t>(scene->meshes[mi + 1].first_index) : scene->index_count;
        for (uint64_t k = static_cast<uint64_t>(m.first_index); k < end; ++k) {
            const uint32_t v = static_cast<uint32_t>(m.first_vertex) + scene->indices[k];
            for (int a = 0; a < 3; ++a) tri[nTri * 3 + a] = scene->positions[3 * static_cast<size_t>(v) + a];
            ++nTri;
        }
    }
    nTri /= 3;
    uint64_t stats[8] = {};
    CHECK(ark_ddgi_debug_bvh8_check(tri.data(), nTri, stats) == 0);
    CHECK(stats[3] == 0 && stats[4] == nTri); // no violations, every triangle in a leaf
    std::printf("bvh8: %llu triangles, %llu nodes\n", static_cast<unsigned long long>(nTri), static_cast<unsigned long long>(stats[0]));

    // the three hit-mask classes' shared host build (set_scene, the background rebuild):
    // each class in turn holding a single triangle, and a run with an empty class
    CHECK(nTri >= 301);
    for (int single = 0; single < 3; ++single) CHECK(worldBvh8Case(tri, 301, single, false) == 0);
    CHECK(worldBvh8Case(tri, 301, 0, true) == 0);
    CHECK(worldBvh8Case(tri, 301, 1, true) == 0);

    // the device-build parity tests' tree comparison (compare_bvh8_canonical) over the LBVH
    // restatement's trees, three classes and the sun's: a renumbered twin compares clean,
    // six mutations of it are reported (tests/test_bvh8_compare.py, here under the sanitizers)
    {
        const float sunDir[3] = { 0.3f, -1.0f, -0.4f };
        uint64_t cmp[16] = {};
        CHECK(ark_ddgi_debug_bvh8_compare_selftest(tri.data(), nTri, nullptr, 5, cmp) == 0);
        CHECK(cmp[2] == 0 && cmp[3] == cmp[0] && cmp[11] == 0 && cmp[12] == 0);
        CHECK(ark_ddgi_debug_bvh8_compare_selftest(tri.data(), nTri, sunDir, 5, cmp) == 0);
        CHECK(cmp[2] == 0 && cmp[3] == cmp[0] && cmp[11] == 0 && cmp[12] == 0);
        std::printf("bvh8 compare: %llu nodes\n", static_cast<unsigned long long>(cmp[0]));
    }

    // oracle: 4x4x4 probes x 64 rays, offsets on, three frames
    ArkDdgiDesc d;
    std::memset(&d, 0, sizeof(d));
    d.struct_size = sizeof(d);
    d.grid_dims[0] = d.grid_dims[1] = d.grid_dims[2] = 4;
    for (int k = 0; k < 3; ++k) {
        d.probe_spacing[k] = 1.5f;
        d.offset_to_first[k] = 0.5f;
    }
    d.max_rays_per_probe = 64;
    d.max_probe_updates = 64;
    d.z_far = 100.0f;
    d.clear_overflow_mode = ARK_DDGI_CLEAR_OVERFLOW_INF;
    d.shard_count = 1;
    void* o = oracle_create(&d);
    CHECK(o != nullptr);
    CHECK(oracle_set_scene(o, scene, 2) == 0);
    for (uint32_t frame = 0; frame < 3; ++frame) {
        ArkDdgiFrameParams p;
        std::memset(&p, 0, sizeof(p));
        p.struct_size = sizeof(p);
        p.rays_per_probe = 64;
        p.probe_updates = 64;
        p.first_probe_index = 0;
        p.frame_index = frame;
        p.hysteresis_irradiance = frame ? 0.98f : 0.0f;
        p.hysteresis_visibility = frame ? 0.98f : 0.0f;
        p.visibility_sharpness = 50.0f;
        p.environment_multiplier = 1.0f;
        p.ambient_amount = 0.0f;
        p.delta_time = 1.0f / 60.0f;
        p.update_offsets = 1;
        CHECK(oracle_update(o, &p, 2) == 0);
    }
    {
        // the blend alone on planted surfels: a ragged window that wraps past N = 64, 37 of 64 rays
        std::vector<uint16_t> surfels(64 * 64 * 4);
        for (size_t i = 0; i < surfels.size(); ++i) surfels[i] = static_cast<uint16_t>((i * 2654435761u) >> 17); // finite fp16 codes
        CHECK(oracle_write(o, ARK_DDGI_SURFELS, surfels.data(), surfels.size() * 2) == 0);
        ArkDdgiFrameParams p;
        std::memset(&p, 0, sizeof(p));
        p.struct_size = sizeof(p);
        p.rays_per_probe = 37;
        p.probe_updates = 7;
        p.first_probe_index = 60;
        p.frame_index = 700;
        p.hysteresis_irradiance = 0.98f;
        p.hysteresis_visibility = 0.98f;
        p.visibility_sharpness = 7.3f;
        p.delta_time = 1.0f / 60.0f;
        p.update_offsets = 1;
        CHECK(oracle_blend(o, &p, 2) == 0);
        p.rays_per_probe = 65; // more than max_rays_per_probe: refused
        CHECK(oracle_blend(o, &p, 2) != 0);
    }
    {
        // shading alone on planted hits: the same ragged window; front hits, back faces and
        // misses over the soup's first instances, shadow rays traced from the hit points
        ArkDdgiFrameParams p;
        std::memset(&p, 0, sizeof(p));
        p.struct_size = sizeof(p);
        p.rays_per_probe = 37;
        p.probe_updates = 7;
        p.first_probe_index = 60;
        p.frame_index = 700;
        p.environment_multiplier = 1.0f;
        p.ambient_amount = 0.1f;
        std::vector<OracleShadeHit> hits(7 * 37);
        for (size_t i = 0; i < hits.size(); ++i) {
            const uint32_t inst = static_cast<uint32_t>(i % scene->instance_count);
            hits[i] = { inst, static_cast<uint32_t>(i % scene->instances[inst].triangle_count), 0.25f, 0.5f, i % 3 == 1 ? -1.5f : 0.75f };
            if (i % 5 == 4) hits[i].instance = 0xffffffffu; // a miss
        }
        CHECK(oracle_shade(o, &p, hits.data(), 2) == 0);
        std::vector<uint32_t> bits(64 * 64);
        CHECK(oracle_read(o, 201, bits.data(), bits.size() * 4) == 0);
        hits[3].primitive = scene->instances[hits[3].instance].triangle_count; // past the instance: refused
        CHECK(oracle_shade(o, &p, hits.data(), 2) != 0);
        hits[3].primitive = 0;
        hits[3].u = 0.75f; // u + v > 1: refused
        CHECK(oracle_shade(o, &p, hits.data(), 2) != 0);
    }
    std::vector<uint16_t> irr(4 * 10 * 4 * 4 * 10 * 4);
    CHECK(oracle_read(o, ARK_DDGI_ATLAS_IRRADIANCE, irr.data(), irr.size() * 2) == 0);
    // AO bake of the soup's first instance, a small texture
    const uint32_t W = 32, H = 32;
    std::vector<uint32_t> bt(W * H);
    std::vector<uint16_t> bb(W * H * 4);
    std::vector<uint8_t> bo(W * H * 4);
    CHECK(oracle_bake_ao(o, 0, W, H, 4, 1, 0, H, bt.data(), bb.data(), bo.data(), 2) == 0);
    oracle_destroy(o);
    ark_soup_free(soup);
    std::printf("OK\n");
    return 0;
}
