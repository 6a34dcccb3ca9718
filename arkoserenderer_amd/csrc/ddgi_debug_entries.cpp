// ddgi_debug_entries.cpp — the ark_ddgi_debug_* entries of a context
// (include/ark_ddgi_debug.h): what the tests read back or force, none of it on an update's path.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "ddgi_context.h"
#include "path_tracer_host.h"
#include "refl_denoise_host.h"
#include "rt_shadows_host.h"
#include "sun_bvh.h"
#include "sun_cover_build.h"

extern "C" {

int ark_ddgi_debug_geometry_update_info(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "geometry update info before ark_ddgi_set_scene");
    const SceneStore& st = *ctx->sceneStore;
    out[0] = st.recordMapAllocs;
    out[1] = st.recordMapFills;
    out[2] = st.recordMap.bytes + st.triBase.bytes + st.stageCounters.bytes;
    out[3] = st.book.vtx.seq;
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_scene_digest(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "scene digest before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return sceneDigest(*ctx->sceneStore, ctx, out);
}

int ark_ddgi_debug_world_bvh_check(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "world BVH check before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return sceneWorldBvhCheck(*ctx->sceneStore, ctx, out);
}

int ark_ddgi_debug_sun_bvh_installed_check(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "sun BVH check before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return sceneSunBvhCheck(*ctx->sceneStore, ctx, out);
}

int ark_ddgi_debug_refit_reach(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "refit reach before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return sceneRefitReach(*ctx->sceneStore, ctx, out);
}

int ark_ddgi_debug_refit_inflation(ArkDdgiCtx* ctx, float* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "refit inflation before ark_ddgi_set_scene");
    out[0] = ctx->sceneStore->world.boxesInflate;
    out[1] = ctx->sceneStore->sun.boxesInflate;
    return ARK_DDGI_OK;
}

static int sunCoverCounts(ArkDdgiCtx* ctx, uint64_t* out, bool hostRestatement);
int ark_ddgi_debug_sun_cover_counts(ArkDdgiCtx* ctx, uint64_t* out) { return sunCoverCounts(ctx, out, true); }
int ark_ddgi_debug_sun_cover_counts_device(ArkDdgiCtx* ctx, uint64_t* out) { return sunCoverCounts(ctx, out, false); }

static int sunCoverCounts(ArkDdgiCtx* ctx, uint64_t* out, bool hostRestatement)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "cover counts before ark_ddgi_set_scene");
    if (!ctx->coverCountsValid) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "cover counts: the last update was not a counting one (ark_ddgi_set_counting)");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    std::fill(out, out + 12, 0ull);
    const SceneStore& st = *ctx->sceneStore;
    const FrameArgs& f = ctx->coverFrame;
    uint32_t dc[3] = { 0, 0, 0 };
    ARK_HIP(hipMemcpy(dc, f.cover_counts, sizeof(dc), hipMemcpyDeviceToHost));
    const bool inUse = ctx->scene.sun_map != nullptr;
    for (int k = 0; k < 3; ++k) out[k] = dc[k];
    out[3] = inUse ? 1 : 0;
    if (inUse) {
        out[4] = st.coverMap.grid.nx;
        out[5] = st.coverMap.grid.ny;
        out[6] = st.coverMap.buf.bytes;
        out[7] = static_cast<uint64_t>(st.coverMap.buildMs * 1000.0f);
    }
    if (!hostRestatement || !ctx->hasSun || f.window_rays == 0) return ARK_DDGI_OK;
    // the host restatement: the update's sun-ray origins, the map of the installed records
    DeviceBuffer pts;
    ARK_HIP(pts.alloc(static_cast<size_t>(f.window_rays) * sizeof(float4)));
    hipError_t e = launch_sun_points(f, pts.as<float4>(), nullptr);
    std::vector<float> P(static_cast<size_t>(f.window_rays) * 4u);
    if (e == hipSuccess) e = hipMemcpy(P.data(), pts.ptr, P.size() * 4u, hipMemcpyDeviceToHost);
    pts.release();
    ARK_HIP(e);
    cover::Grid grid {};
    std::vector<float> map;
    bool ok = false;
    float F[9] {};
    if (inUse) {
        std::vector<GpuTriangle> rec(st.world.records);
        ARK_HIP(hipMemcpy(rec.data(), st.world.tris(st.world.buf), rec.size() * sizeof(GpuTriangle), hipMemcpyDeviceToHost));
        double frame[3][3];
        sun_frame(ctx->sunDir, frame);
        float L[3];
        sunRayDirection(ctx->sunDir, L);
        ok = hostBuildCoverMap(rec.data(), rec.size(), &frame[0][0], L, cover::kDefaultBudget, grid, map) && 2.0f * ctx->desc.z_far >= grid.wExtent;
        for (int k = 0; k < 9; ++k) F[k] = static_cast<float>((&frame[0][0])[k]);
        if (ok) {
            if (std::memcmp(&grid, &st.coverMap.grid, sizeof(grid)) != 0) {
                out[11] = ~0ull;
            } else {
                std::vector<float> dmap(map.size());
                ARK_HIP(hipMemcpy(dmap.data(), st.coverMap.buf.ptr, dmap.size() * 4u, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < map.size(); ++i) out[11] += cover::floatBits(map[i]) != cover::floatBits(dmap[i]);
            }
        }
    }
    const float lift = cover::kTmin + grid.margin, reach = cover::kTmin - grid.margin;
    for (uint32_t i = 0; i < f.window_rays; ++i) {
        const float* o = &P[4u * i];
        if (o[3] == 0.0f) continue;
        int vd = cover::kUndecided;
        if (ok) {
            // sunCoords
            const float pl[3] = { std::fma(o[0], F[0], std::fma(o[1], F[1], o[2] * F[2])), std::fma(o[0], F[3], std::fma(o[1], F[4], o[2] * F[5])),
                                  std::fma(o[0], F[6], std::fma(o[1], F[7], o[2] * F[8])) };
            const int64_t c = cover::cellIndex(grid, pl[0], pl[1]);
            if (c >= 0) vd = cover::verdict(pl[2], lift, reach, map[2 * c], map[2 * c + 1]);
        }
        out[vd == cover::kOccluded ? 8 : vd == cover::kLit ? 9 : 10]++;
    }
    return ARK_DDGI_OK;
}

// One pass of ark_ddgi_rt_reflections_denoise on its own (tools/refl_denoise_cost.py times each).
int ark_ddgi_debug_refl_denoise_pass(ArkDdgiCtx* ctx, const ArkReflDenoiseDesc* desc, int pass, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkReflDenoiseDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkReflDenoiseDesc");
    if (const char* why = refl::descProblem(*desc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "refl_denoise_pass: %s", why);
    if (pass < 0 || pass > 4) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "refl_denoise_pass: pass %d", pass);
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(launch_refl_denoise_pass(refl::argsOf(*desc), pass, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

// The local-light shadow masks' host restatement over the front copy's records (whatever
// the refits and vertex updates so far made of them) and the instances' classes.
int ark_ddgi_debug_rt_shadows_host_ctx(ArkDdgiCtx* ctx, uint32_t class_mask, const ArkRtShadowsDesc* desc, uint64_t* counts)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkRtShadowsDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkRtShadowsDesc");
    if (const char* why = rtshadow::descProblem(*desc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_shadows_host_ctx: %s", why);
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "rt_shadows_host_ctx before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    if (ctx->sceneVersion != ctx->sceneStore->version)
        if (const int rc = refreshScene(ctx)) return rc;
    std::vector<uint32_t> rec;
    std::vector<int32_t> cls;
    if (const int rc = sceneRecordsAndClasses(*ctx->sceneStore, ctx, rec, cls)) return rc;
    const int rc = rtshadow::hostShadows(rec.data(), rec.size() / 12u, cls.data(), cls.size(), class_mask, *desc, counts);
    return rc == 0 ? ARK_DDGI_OK : ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_shadows_host_ctx: bad arguments");
}

int ark_ddgi_debug_path_tracer_host_ctx(ArkDdgiCtx* ctx, const ArkPathTracerDesc* desc, void* vertices, uint64_t* counts)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkPathTracerDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkPathTracerDesc");
    if (const char* why = pt::descProblem(*desc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "path_tracer_host_ctx: %s", why);
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "path_tracer_host_ctx before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    if (ctx->sceneVersion != ctx->sceneStore->version)
        if (const int rc = refreshScene(ctx)) return rc;
    pt::HostScene hs;
    if (const int rc = sceneHostCopy(*ctx->sceneStore, ctx, hs)) return rc;
    // the context's lights (ark_ddgi_set_lights), as the entry's kernels get them
    hs.hasSun = ctx->scene.has_sun;
    for (int k = 0; k < 3; ++k) {
        hs.sunColor[k] = ctx->scene.sun_color[k];
        hs.sunDir[k] = ctx->scene.sun_dir[k];
    }
    hs.spots = ctx->spotHost;
    const int rc = pt::hostPathTrace(hs.view(), hs.tris.size(), *desc, static_cast<pt::Vertex*>(vertices), counts);
    return rc == 0 ? ARK_DDGI_OK : ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "path_tracer_host_ctx: bad arguments");
}

int ark_ddgi_debug_path_tracer_set_segments(ArkDdgiCtx* ctx, uint32_t segments)
{
    if (!ctx || segments == 0 || segments > pt::kMaxSegments) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->ptSegments = segments;
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_path_tracer_last_counts(ArkDdgiCtx* ctx, uint32_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(uint32_t) * 2 * pt::kMaxSegments);
    if (ctx->ptWork.bytes < kPtCounterWords * 4u) return ARK_DDGI_OK; // no path_trace call yet
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    std::vector<uint32_t> words(kPtCounterWords);
    ARK_HIP(hipMemcpy(words.data(), ctx->ptWork.ptr, words.size() * 4u, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < pt::kMaxSegments; ++s) {
        out[s] = words[s * kPtSegmentWords + kPtListCountWord];
        out[pt::kMaxSegments + s] = words[s * kPtSegmentWords + kPtShadowCountWord];
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_set_sun_only_small_windows(ArkDdgiCtx* ctx, int enabled)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->sunOnlySmallWindows = enabled != 0;
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_shade_schedule(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    out[0] = out[1] = 0;
    if (!ctx->lastSunOnly) return ARK_DDGI_OK;
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    uint32_t n = 0;
    ARK_HIP(hipMemcpy(&n, ctx->lastDeferredCount, sizeof(n), hipMemcpyDeviceToHost));
    out[0] = 1;
    out[1] = n;
    return ARK_DDGI_OK;
}

// The probe update's launches alone over planted surfels and hit records (ddgi_frame.cpp: it
// shares the update's arguments and its book of the frames in flight).
int ark_ddgi_debug_probe_update(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* params, const ArkDdgiDebugHit* hits, void* hipStream)
{
    return debugProbeUpdate(ctx, params, hits, hipStream);
}

int ark_ddgi_debug_probe_update_layout(uint32_t* out, int n)
{
    const uint32_t words[] = { sizeof(ArkDdgiDebugHit), offsetof(ArkDdgiDebugHit, t), offsetof(ArkDdgiDebugHit, tri) };
    const int m = static_cast<int>(sizeof(words) / sizeof(words[0]));
    if (!out) return 0;
    for (int i = 0; i < n && i < m; ++i) out[i] = words[i];
    return m < n ? m : n;
}

// Hit shading alone over planted hit records (ddgi_frame.cpp, beside the update it shares its
// launches with).
int ark_ddgi_debug_shade(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* params, const ArkDdgiDebugShadeHit* hits, void* hipStream)
{
    return debugShade(ctx, params, hits, hipStream);
}

int ark_ddgi_debug_world_records(ArkDdgiCtx* ctx, uint32_t* out_words, uint64_t capacity, uint64_t* out_records)
{
    if (!ctx || !out_records) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "world_records before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    if (ctx->sceneVersion != ctx->sceneStore->version)
        if (const int rc = refreshScene(ctx)) return rc;
    std::vector<uint32_t> rec;
    std::vector<int32_t> cls;
    if (const int rc = sceneRecordsAndClasses(*ctx->sceneStore, ctx, rec, cls)) return rc;
    *out_records = rec.size() / 12u;
    if (out_words && capacity >= *out_records) std::memcpy(out_words, rec.data(), rec.size() * 4u);
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_shade_map(const uint32_t* record_words, uint64_t records, uint32_t instances, float z_far, const ArkDdgiDebugShadeHit* hits, uint64_t n,
                             uint32_t* out_tri)
{
    return debugShadeMap(record_words, records, instances, z_far, hits, n, out_tri);
}

int ark_ddgi_debug_shade_layout(uint32_t* out, int n)
{
    const uint32_t words[] = { sizeof(ArkDdgiDebugShadeHit), offsetof(ArkDdgiDebugShadeHit, instance), offsetof(ArkDdgiDebugShadeHit, primitive),
                               offsetof(ArkDdgiDebugShadeHit, u), offsetof(ArkDdgiDebugShadeHit, v), offsetof(ArkDdgiDebugShadeHit, t) };
    const int m = static_cast<int>(sizeof(words) / sizeof(words[0]));
    if (!out) return 0;
    for (int i = 0; i < n && i < m; ++i) out[i] = words[i];
    return m < n ? m : n;
}

uint32_t ark_ddgi_debug_seed_texel(float x, float y, float z) { return seed::texelOf(x, y, z); }
int ark_ddgi_debug_seed_candidate_ok(uint32_t word, uint32_t first, uint32_t end) { return seed::candidateOk(word, first, end) ? 1 : 0; }

int ark_ddgi_debug_seed_info(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    out[0] = ctx->seeds.ptr ? 1u : 0u;
    out[1] = seed::kTexels;
    out[2] = ctx->hasScene ? ctx->sceneStore->args.opaque_tri_first : 0u;
    out[3] = ctx->hasScene ? ctx->sceneStore->args.opaque_tri_end : 0u;
    out[4] = 0;
    if (ctx->seeds.ptr && ctx->countersPending) {
        uint32_t n = 0;
        ARK_HIP(hipSetDevice(ctx->device));
        ARK_HIP(hipDeviceSynchronize());
        ARK_HIP(hipMemcpy(&n, ctx->counters.as<uint32_t>() + ctx->counters.bytes / 4u - 4u, sizeof(n), hipMemcpyDeviceToHost));
        out[4] = n;
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_seed_fill(ArkDdgiCtx* ctx, int mode, uint64_t value)
{
    if (!ctx || mode < 0 || mode > 2) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "seed fill before ark_ddgi_set_scene");
    if (!ctx->seeds.ptr) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "the context keeps no seed cache (ARK_DDGI_FLAG_NO_RAY_SEEDS)");
    const uint32_t first = ctx->sceneStore->args.opaque_tri_first, end = ctx->sceneStore->args.opaque_tri_end;
    std::vector<uint32_t> words(ctx->seeds.bytes / 4, seed::kNone);
    if (mode != 0 && end > first) {
        uint64_t x = value * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull; // splitmix64
        for (uint32_t& w : words) {
            if (mode == 2) {
                w = static_cast<uint32_t>(value);
            } else {
                x += 0x9e3779b97f4a7c15ull;
                uint64_t z = x;
                z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
                z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
                z ^= z >> 31;
                w = first + static_cast<uint32_t>(z % (end - first));
            }
            // only words the lookup would accept ever reach the device
            if (!seed::candidateOk(w, first, end)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "seed fill: record %u outside the opaque class [%u, %u)", w, first, end);
        }
    }
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(ctx->seeds.ptr, words.data(), ctx->seeds.bytes, hipMemcpyHostToDevice));
    ctx->seedStale = false; // (a whole cache of this record order's words)
    ctx->seedTopologySeen = ctx->sceneStore->worldTopologySeq;
    return ARK_DDGI_OK;
}

} // extern "C"
