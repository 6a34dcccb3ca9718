// ddgi_context.h — the C-ABI context of the MI355X DDGI path (include/ark_ddgi.h) and the
// helpers its files share. Internal to libark_ddgi.so:
//   ark_ddgi.cpp            context lifetime, scene, lights and resources
//   ddgi_frame.cpp          the update (frames in flight: frame_book.h), sequencing, exchanges
//   ddgi_passes.cpp         AO bake, lighting compose, RT reflections, probe debug
//   ddgi_debug_entries.cpp  the ark_ddgi_debug_* entries (include/ark_ddgi_debug.h)
// Their kernels and launchers (ddgi_kernels.h), one unit per pass: ddgi_kernels.hip +
// ddgi_update.hip (the update), ddgi_bake.hip, ddgi_compose.hip (compose, probe debug),
// ddgi_reflections.hip, ddgi_rt_shadows.hip, ddgi_path_tracer.hip; the traversal they share
// is ddgi_traversal.h and ddgi_trace_kernels.h.
// A context owns the device memory of one DDGI node instance on one GPU: the persistent
// atlases/offsets (the DDGISamplingSet, DDGINode.cpp:62-66), the per-update
// working set (slot table, hit records, surfels) and its lights, and holds the scene
// (scene_store.h: BVH + RT mesh data + materials, possibly shared with other
// contexts). Every update is enqueued on one HIP stream.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/ark_ddgi.h"
#include "../../include/ark_ddgi_debug.h"
#include "ddgi_kernels.h"
#include "frame_book.h"
#include "scene_store.h"

using namespace ark; // (an internal header: every file that includes it is of the context)

// pipelined windows below this many probe rays trace at half occupancy (ctx->pipeTraceBlocks)
constexpr uint32_t kPipeHalfRays = 5u << 20;
constexpr int kPipeTracePerCu = 3; // traversal workgroups per CU of such a window (ctx->pipeTraceBlocks; 2, 4, 5 measured slower)
// Idle traversal lanes are refilled in batches of >= kRefillMin (the refill then stalls
// a wave once per 16 finished rays, and the rays it starts descend from the root
// together: C4 2.98 vs 3.30 ms at 1 in round 1; with the fetches outside branches 16
// is the best: step 3.53 -> 3.46 ms against 4, 24 and 32, profiles/r03_as, r03_at; with
// k_trace's refills reading staged records from LDS, measured again: C4 2,566 / 2,580 /
// 2,589 / 2,565 Mrays/s at 8 / 12 / 16 / 24, means of three interleaved runs,
// EXPERIMENTS.md "LDS ray pool"). The
// sun's any-hit rays in the light-space BVH are short: 32 (profiles/r05_q: C4 shadow
// phase 0.648 -> 0.630 ms, K = 2048 0.327 -> 0.320 ms; the world BVHs' shadow rays keep
// 16: 32 there made C5's shadow phase 1.92 -> 2.07 ms). kGrabChunk: rays per
// partition-head grab, 64 = a probe quarter of direction-clustered rays per wave pool
// (16 and 8 measured slower on 1/8 slabs).
constexpr uint32_t kRefillMin = 16, kSunRefillMin = 32, kGrabChunk = 64;
static_assert(kGrabChunk <= 64, "a wave stages one ray of a chunk per lane (k_trace's pool, the shadow traversal's refill)");

struct ArkDdgiCtx : ErrorSink {
    ArkDdgiDesc desc {};
    hipStream_t stream = nullptr; // internal (clears); synchronous use only
    // Call order across streams: every operation records evOrder on its stream when
    // enqueued, and the next one waits for it when given another stream (orderBegin).
    hipEvent_t evOrder = nullptr;
    hipStream_t orderStream = nullptr;
    bool orderValid = false;
    // traversal refill batch (probe and shadow rays, the sun's), rays per partition-head grab
    uint32_t refillMin = kRefillMin, sunRefillMin = kSunRefillMin, grabChunk = kGrabChunk;
    int device = 0;
    int cuCount = 0;
    int X = 0, Y = 0, Z = 0, N = 0;
    int Wi = 0, Hi = 0, Wv = 0, Hv = 0;
    int Kmax = 0, Rmax = 0;
    int slabZ0 = 0, slabZ1 = 0;
    // persistent resources
    DeviceBuffer irr, vis, offsets;
    // working set
    DeviceBuffer slots, slotOrder, fib, fibOrder, order, hits, surfels, spill, rayCounter, counters, shadeWork, reflWork, rtShadowWork, ptWork;
    DeviceBuffer raySteps; // counting updates: u16 traversal iterations per probe ray (ARK_DDGI_DEBUG_RAY_STEPS)
    // The probe rays' hit candidates (seed_cache.h; none with ARK_DDGI_FLAG_NO_RAY_SEEDS):
    // [N][seed::kProbeWords] triangle records of the world BVHs' opaque class, or seed::kNone.
    // The words are record indices, so they belong to one record order: the cache is
    // refilled with kNone on the traversal stream, ahead of the next traversal, whenever the
    // scene's worldTopologySeq has moved or the context has taken another scene (seedStale).
    DeviceBuffer seeds;
    bool seedStale = true;
    uint32_t seedTopologySeen = 0;
    std::vector<uint32_t> orderHost; // traversal order of the samples for orderR
    uint32_t orderR = 0;
    uint32_t lightCount = 0;
    uint32_t traceBlocks = 0, shadeBlocks = 0, shadowBlocks = 0, shadowBlocksPerCu = 1;
    // Frames in flight: which stream each part of an update runs on and what it waits for is
    // decided by `frames` (frame_book.h) and executed by updateImpl (ddgi_frame.cpp) with
    // the handles below. Frame n's slot table, primary traversal and probe offsets run on
    // traceStream when pipelined, beside frame n - 1's shadow rays, shading and probe update.
    FrameBook frames;
    int sunBvh = -1;               // ArkDdgiDesc.sun_bvh: 0 the sun's shadow rays traverse the world BVHs, 1 the light-space BVH, -1: by cost (sun_bvh_pays)
    uint32_t pipeTraceBlocks = 0; // primary-traversal grid of a pipelined window below kPipeHalfRays rays
    hipStream_t traceStream = nullptr;
    hipEvent_t evTraced = nullptr, evFrameDone[2] = {};
    // Device-side frame sequencing of pipelined frames (k_seq_signal / k_seq_wait
    // instead of cross-queue event waits): seqWords [0] = the last frame whose
    // traversal-stream part (slot table, traversal, offsets) is done, [32] = the last
    // frame whose caller-stream part is done, [64] = a wait timed out, [96] = the last
    // exchange completed on the caller's exchange stream (a signal folded
    // into the last kernel - its last workgroup storing the word after a device-scope
    // fence per workgroup - measured slower: the fences write back L2, K = 2048 frames
    // 0.371 -> 0.387 ms, profiles/r03_y).
    DeviceBuffer seqWords;
    uint64_t seqTimeoutTicks = 0;
    uint32_t seqTimeoutMs = 10000;
    uint64_t wallClockKhz = 100000;
    // fail-closed sequencing: a k_seq_wait that gives up sets seqWords[64] (every path
    // kernel then skips: frameAborted) and this host-mapped word, which the next
    // update / exchange_begin / synchronize polls (checkSequencing)
    uint32_t* hostAbort = nullptr;    // host pointer (hipHostMalloc, coherent)
    uint32_t* hostAbortDev = nullptr; // its device address
    // Z-slab exchanges (ark_ddgi_exchange_begin/_end, ark_ddgi_update_exchanged)
    hipStream_t lastStream = nullptr; // the last update's stream
    hipEvent_t evExchangeSrc = nullptr; // exchange_begin after an unsequenced update
    hipEvent_t evExchangeDone = nullptr; // exchange_end without sequence words
    uint64_t spillRegionWords = 0; // spill region 1 = the primary traversal's
    // scene
    bool hasScene = false;
    std::shared_ptr<SceneStore> sceneStore; // device scene (possibly shared with other contexts)
    uint32_t sceneVersion = 0;              // sceneStore->version that `scene` was derived at
    // Per-frame lights (ark_ddgi_set_lights; set_scene / share_scene start them with the
    // scene's): the sun travels in `scene` (kernel arguments), the spots in `lights` on
    // the device, stored there in stream order ahead of the next operation that reads
    // them (flushLights) when lightsDirty
    DeviceBuffer lights; // GpuSpotLight[kMaxLights - 1]
    std::vector<GpuSpotLight> spotHost;
    int32_t hasSun = 0;
    float sunColor[3] { 0, 0, 0 }, sunDir[3] { 0, 0, 0 };
    bool lightsDirty = false;
    // AO bake results (ark_ddgi_bake_ao)
    DeviceBuffer bakeTri, bakeBary, bakeOut, bakePixels, bakeCounters;
    uint32_t bakeW = 0, bakeH = 0;
    int bakeBent = 0;
    SceneArgs scene {};          // = sceneStore->args
    ArkDdgiBvhStats bvhStats {}; // = sceneStore->bvhStats
    uint32_t bvhMaxDepth = 0;
    // instrumentation
    bool counting = false;
    bool lastSunOnly = false;          // the last update ran the sun-only shading schedule (shade_schedule.h) ...
    const uint32_t* lastDeferredCount = nullptr; // ... and this device word holds the rays it deferred
    bool sunOnlySmallWindows = false;  // ark_ddgi_debug_set_sun_only_small_windows
    bool coverCountsValid = false; // the last update was a counting one (ark_ddgi_debug_sun_cover_counts) ...
    FrameArgs coverFrame {};       // ... and its shading arguments
    bool timing = false;
    hipEvent_t ev[6] = {};
    bool timingValid = false;
    bool countersPending = false;
    uint64_t lastRays = 0, lastProbes = 0;
    uint32_t ptSegments = 16; // ark_ddgi_debug_path_tracer_set_segments (timing only)
    uint32_t nextProbeIndex = 0; // (first + K) % N of the last update, or of a loaded state
    uint32_t lastFirst = 0, lastK = 0; // the last update's window (ark_ddgi_window_exchange_info)
    // the refits and installed rebuilds of the scene (by any context sharing it) that this
    // context's traversal stream has waited for: SceneStore::geometrySeq at its last wait
    // for the store's evGeometry (updateImpl). The ordering of the scene's geometry
    // copies itself belongs to the store.
    uint32_t geometrySeen = 0;
};

#define ARK_HIP(expr) ARK_HIP_TO(ctx, expr)

namespace ark {

// The stream of an asynchronous entry point: NULL is the legacy default (null)
// stream, which orders against every blocking stream of the process (torch's
// default stream among them), like any other HIP API taking a stream.
inline hipStream_t streamOf(void* h) { return static_cast<hipStream_t>(h); }

// Operations of one context execute in call order, whatever streams they are given
// (they share the traversal spill area, the hit records and the atlases): an
// operation on another stream than the previous one first waits for it.
inline hipError_t orderBegin(ArkDdgiCtx* ctx, hipStream_t s)
{
    if (ctx->orderValid && ctx->orderStream != s) return hipStreamWaitEvent(s, ctx->evOrder, 0);
    return hipSuccess;
}

inline hipError_t orderEnd(ArkDdgiCtx* ctx, hipStream_t s)
{
    const hipError_t e = hipEventRecord(ctx->evOrder, s);
    ctx->orderStream = s;
    ctx->orderValid = e == hipSuccess;
    return e;
}

// Shading work set for the largest window and `lightCount` lights: per-ray light bits, then
// k_shadow_gen's shadow-ray list (at most one ray per probe ray and light).
struct ShadeWorkLayout {
    uint64_t bits, list, total;
};

inline ShadeWorkLayout shadeWorkLayout(const ArkDdgiCtx* ctx, uint32_t lightCount)
{
    auto al = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t rays = static_cast<uint64_t>(ctx->Kmax) * ctx->Rmax;
    const uint64_t entries = rays * lightCount;
    ShadeWorkLayout w {};
    w.bits = 0;
    w.list = al(rays * 4);
    w.total = w.list + al(entries * sizeof(ShadowRay));
    return w;
}

// Workgroups of the persistent shadow traversal for `rays` closest-hit rays (~0.25
// shadow rays each on C4): the launch is a tail of the longest shadow rays when
// there are few, and fewer co-resident waves shorten each one's iterations
// (measured on C4: K = 2048 windows 0.228 -> 0.180 ms at 3 workgroups per CU,
// K = 4096 0.246 -> 0.225, the full grid (8.4 M rays) unchanged from 5 to 6).
constexpr uint64_t kShadowMinPerCu = 3; // 1 and 2 measured slower or within noise (profiles/r04_p)
inline uint32_t shadowBlocksFor(const ArkDdgiCtx* ctx, uint64_t rays)
{
    const uint64_t perCu = std::min<uint64_t>(ctx->shadowBlocksPerCu, std::max<uint64_t>(kShadowMinPerCu, rays >> 20));
    return static_cast<uint32_t>(perCu * ctx->cuCount);
}

// The DDGISamplingSet (DDGINode.cpp:45-66) as kernel arguments: grid constants + both atlases
inline FrameArgs samplingSetArgs(const ArkDdgiCtx* ctx)
{
    FrameArgs f {};
    f.X = ctx->X; f.Y = ctx->Y; f.Z = ctx->Z;
    f.Wi = ctx->Wi; f.Hi = ctx->Hi; f.Wv = ctx->Wv; f.Hv = ctx->Hv;
    for (int k = 0; k < 3; ++k) {
        f.spacing[k] = ctx->desc.probe_spacing[k];
        f.origin[k] = ctx->desc.offset_to_first[k];
    }
    f.irr = ctx->irr.as<uint16_t>();
    f.vis = ctx->vis.as<uint16_t>();
    return f;
}

// ark_ddgi.cpp
int ensureSpill(ArkDdgiCtx* ctx);                        // a traversal spill area deep enough for the context's BVHs
int refreshScene(ArkDdgiCtx* ctx);                       // the context's kernel view of its scene re-derived, ensureSpill
hipError_t flushLights(ArkDdgiCtx* ctx, hipStream_t s);  // changed spot lights stored on `s`
hipError_t drainContext(ArkDdgiCtx* ctx);                // waits for every operation of the context enqueued so far
SceneCall sceneCall(ArkDdgiCtx* ctx);                    // what the scene's calls take from the calling context
// ddgi_frame.cpp
int checkSequencing(ArkDdgiCtx* ctx); // reports a sequence-word wait that gave up (fail closed), once
int debugProbeUpdate(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, const ArkDdgiDebugHit* hits, void* hipStream); // ark_ddgi_debug_probe_update
int debugShade(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, const ArkDdgiDebugShadeHit* hits, void* hipStream);     // ark_ddgi_debug_shade
int debugShadeMap(const uint32_t* words, uint64_t n, uint32_t instances, float zFar, const ArkDdgiDebugShadeHit* hits, uint64_t count, uint32_t* outTri); // ark_ddgi_debug_shade_map

} // namespace ark
