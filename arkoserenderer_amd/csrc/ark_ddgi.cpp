// ark_ddgi.cpp — the C-ABI context of the MI355X DDGI path (include/ark_ddgi.h).
//
// Owns the device memory of one DDGI node instance on one GPU: the persistent
// atlases/offsets (the DDGISamplingSet, DDGINode.cpp:62-66), the per-update
// working set (slot table, hit records, surfels) and its lights, and holds the scene
// (scene_store.h: BVH + RT mesh data + materials, possibly shared with other
// contexts). Every update is enqueued on one HIP stream.
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ark_ddgi.h"
#include "../../include/ark_ddgi_debug.h"
#include "ark_fmath.h"
#include "ddgi_kernels.h"
#include "scene_store.h"
#include "shade_schedule.h"
#include "sun_bvh.h"
#include "sun_cover_build.h"

using namespace ark;

namespace {

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

// roctx range over a scope (host-side enqueue markers, named after the reference's
// ScopedDebugZone labels, DDGINode.cpp:152-247); end() closes it early.
class RoctxRange {
public:
    explicit RoctxRange(const char* name) { roctxRangePushA(name); }
    ~RoctxRange() { end(); }
    void end()
    {
        if (m_open) roctxRangePop();
        m_open = false;
    }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;

private:
    bool m_open { true };
};

uint16_t f32_to_f16_host(float f)
{
    // host-side RNE conversion for the clear values (matches v_cvt_f16_f32)
    _Float16 h = static_cast<_Float16>(f);
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

// Traversal order of a probe's R samples: groups of 64 (one wave's refill pool)
// with nearby directions, so the lanes of a wave descend similar BVH paths.
// Balanced greedy clustering around ceil(R/64) spherical-Fibonacci centres.
// Only the lane -> sample assignment changes; every sample is traced exactly
// once and its hit record is stored at its own index, so results do not depend
// on the order.
void sampleTraversalOrder(uint32_t R, std::vector<uint32_t>& order)
{
    order.resize(R);
    for (uint32_t i = 0; i < R; ++i) order[i] = i;
    const uint32_t G = (R + 63) / 64;
    if (G <= 1) return;
    auto fib = [](uint32_t i, uint32_t n, double* d) { // same point set as sphericalFibonacci (math accuracy irrelevant here)
        const double phi = 2.0 * M_PI * std::fmod(i * 0.6180339887498949, 1.0);
        const double z = 1.0 - (2.0 * i + 1.0) / n, r = std::sqrt(std::max(0.0, 1.0 - z * z));
        d[0] = std::cos(phi) * r; d[1] = std::sin(phi) * r; d[2] = z;
    };
    std::vector<double> pts(3 * R), ctr(3 * G);
    for (uint32_t i = 0; i < R; ++i) fib(i, R, &pts[3 * i]);
    for (uint32_t g = 0; g < G; ++g) fib(g, G, &ctr[3 * g]);
    struct Pair { double d; uint32_t i, g; };
    std::vector<Pair> pairs;
    pairs.reserve(static_cast<size_t>(R) * G);
    for (uint32_t i = 0; i < R; ++i)
        for (uint32_t g = 0; g < G; ++g)
            pairs.push_back({ pts[3 * i] * ctr[3 * g] + pts[3 * i + 1] * ctr[3 * g + 1] + pts[3 * i + 2] * ctr[3 * g + 2], i, g });
    std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return a.d > b.d; });
    std::vector<int> groupOf(R, -1);
    std::vector<uint32_t> room(G, 64u);
    room[G - 1] = R - 64u * (G - 1);
    for (const Pair& q : pairs)
        if (groupOf[q.i] < 0 && room[q.g] > 0) { groupOf[q.i] = static_cast<int>(q.g); room[q.g]--; }
    uint32_t k = 0;
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t i = 0; i < R; ++i)
            if (groupOf[i] == static_cast<int>(g)) order[k++] = i;
}

} // namespace

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
    DeviceBuffer slots, slotOrder, fib, fibOrder, order, hits, surfels, spill, rayCounter, counters, shadeWork, reflWork;
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
    uint32_t spillEntries = 0;
    uint32_t traceBlocks = 0, shadeBlocks = 0, shadowBlocks = 0, shadowBlocksPerCu = 1;
    // Frames in flight (updateImpl): the per-frame buffers the traversal writes come in
    // two sets (slot table, slot order, sample directions, hit records, work counters);
    // frame n uses set n & 1. Frame n's slot table, primary traversal and probe offsets
    // run on traceStream as soon as frame n - 2 (the previous user of the set) is done,
    // after frame n - 1's offsets (same stream), overlapping frame n - 1's shadow
    // rays, shading and probe update on the caller's stream.
    bool pipelining = true;        // ARK_DDGI_FLAG_SERIAL_FRAMES: every update runs serially
    int sunBvh = -1;               // ArkDdgiDesc.sun_bvh: 0 the sun's shadow rays traverse the world BVHs, 1 the light-space BVH, -1: by cost (sun_bvh_pays)
    uint32_t pipeTraceBlocks = 0; // primary-traversal grid of a pipelined window below kPipeHalfRays rays
    bool pipeReady = false;        // the previous context operation was an update
    uint32_t parity = 0;           // buffer set of the next update
    uint32_t prevR = 0;
    bool prevPipelined = false;    // the previous update's offsets ran on traceStream
    hipStream_t traceStream = nullptr;
    hipEvent_t evTraced = nullptr, evFrameDone[2] = {};
    bool frameDoneValid[2] = { false, false };
    // Device-side frame sequencing of pipelined frames (k_seq_signal / k_seq_wait
    // instead of cross-queue event waits): seqWords [0] = the last frame whose
    // traversal-stream part (slot table, traversal, offsets) is done, [32] = the last
    // frame whose caller-stream part is done, [64] = a wait timed out (a signal folded
    // into the last kernel - its last workgroup storing the word after a device-scope
    // fence per workgroup - measured slower: the fences write back L2, K = 2048 frames
    // 0.371 -> 0.387 ms, profiles/r03_y). setSeq[b] = the
    // frame that last used buffer set b, when that frame was sequenced this way
    // (else its evFrameDone[b] is recorded). ark_ddgi_set_sequencing(ctx, 0, ...): events throughout.
    bool seqSync = true;
    DeviceBuffer seqWords;
    uint32_t frameSeq = 0;
    uint32_t setSeq[2] = { 0, 0 };
    bool setSeqValid[2] = { false, false };
    uint64_t seqTimeoutTicks = 0;
    uint32_t seqTimeoutMs = 10000;
    uint64_t wallClockKhz = 100000;
    // fail-closed sequencing: a k_seq_wait that gives up sets seqWords[64] (every path
    // kernel then skips: frameAborted) and this host-mapped word, which the next
    // update / exchange_begin / synchronize polls (checkSequencing)
    uint32_t* hostAbort = nullptr;    // host pointer (hipHostMalloc, coherent)
    uint32_t* hostAbortDev = nullptr; // its device address
    uint32_t seqTimeouts = 0;         // timeouts reported so far
    // Z-slab exchange sequencing (ark_ddgi_exchange_begin/_end, ark_ddgi_update_exchanged):
    // seqWords [96] = the last exchange completed on the caller's exchange stream
    uint32_t lastMainSeq = 0;        // the last update's caller-stream sequence number (0: not sequenced)
    hipStream_t lastStream = nullptr; // the last update's stream
    hipEvent_t evExchangeSrc = nullptr; // exchange_begin after an unsequenced update
    hipEvent_t evExchangeDone = nullptr; // exchange_end without sequence words (seqSync off)
    uint32_t exchSeq = 0;            // exchanges ended so far
    uint32_t pendingExchange = 0;    // the exchange the next update_exchanged waits for before shading
    uint32_t lastParity = 0;       // buffer set of the last update (debug hit records)
    uint32_t fibR[2] = { 0, 0 };
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
    float lastMs[5] = {};
    bool timingValid = false;
    ArkDdgiCounters lastCounters {};
    bool countersPending = false;
    uint64_t lastRays = 0, lastProbes = 0;
    uint32_t nextProbeIndex = 0; // (first + K) % N of the last update, or of a loaded state
    uint32_t lastFirst = 0, lastK = 0; // the last update's window (ark_ddgi_window_exchange_info)
    // the refits and installed rebuilds of the scene (by any context sharing it) that this
    // context's traversal stream has waited for: SceneStore::geometrySeq at its last wait
    // for the store's evGeometry (updateImpl). The ordering of the scene's geometry
    // copies itself belongs to the store.
    uint32_t geometrySeen = 0;
};

#define ARK_HIP(expr) ARK_HIP_TO(ctx, expr)

namespace {

int clearHistory(ArkDdgiCtx* ctx)
{
    // DDGINode.cpp:50-55: irradiance cleared to 0, visibility to (zFar, zFar^2) in RG16F;
    // zFar^2 = 1e8 overflows fp16: +inf by RNE, or 65504 if saturating.
    uint16_t zf = f32_to_f16_host(ctx->desc.z_far);
    uint16_t zf2 = f32_to_f16_host(ctx->desc.z_far * ctx->desc.z_far);
    if (ctx->desc.clear_overflow_mode == ARK_DDGI_CLEAR_OVERFLOW_MAX_FINITE) {
        if ((zf & 0x7fffu) == 0x7c00u) zf = static_cast<uint16_t>((zf & 0x8000u) | 0x7bffu);
        if ((zf2 & 0x7fffu) == 0x7c00u) zf2 = static_cast<uint16_t>((zf2 & 0x8000u) | 0x7bffu);
    }
    ARK_HIP(hipMemsetAsync(ctx->irr.ptr, 0, ctx->irr.bytes, ctx->stream));
    ARK_HIP(launch_fill_u32(ctx->vis.ptr, ctx->vis.bytes / 4, static_cast<uint32_t>(zf) | (static_cast<uint32_t>(zf2) << 16), ctx->stream));
    ARK_HIP(hipMemsetAsync(ctx->offsets.ptr, 0, ctx->offsets.bytes, ctx->stream));
    ARK_HIP(hipMemsetAsync(ctx->surfels.ptr, 0, ctx->surfels.bytes, ctx->stream));
    ARK_HIP(hipStreamSynchronize(ctx->stream));
    return ARK_DDGI_OK;
}

hipError_t drainContext(ArkDdgiCtx* ctx);

int ensureSpill(ArkDdgiCtx* ctx)
{
    // a node group is pushed at most once per BVH8 level: depth + 2 entries of 2 words
    uint32_t need = std::max<uint32_t>(1u, ctx->bvhMaxDepth + 2u > static_cast<uint32_t>(kStackLds) ? ctx->bvhMaxDepth + 2u - kStackLds : 1u);
    uint32_t threads = std::max(ctx->traceBlocks, ctx->shadowBlocks) * kTraceBlock; // the traversal kernels
    const uint64_t words = static_cast<uint64_t>(need) * 2 * threads;
    const size_t bytes = 2 * words * sizeof(uint32_t); // region 0: all but the primary traversal
    if (ctx->spill.bytes >= bytes) {
        ctx->spillRegionWords = words;
        return ARK_DDGI_OK;
    }
    if (ctx->spill.ptr) ARK_HIP(drainContext(ctx)); // a deeper BVH (a rebuilt sun BVH): frames in flight use it
    ctx->spillRegionWords = words;
    ARK_HIP(ctx->spill.alloc(bytes));
    ctx->spillEntries = need;
    return ARK_DDGI_OK;
}

// The stream of an asynchronous entry point: NULL is the legacy default (null)
// stream, which orders against every blocking stream of the process (torch's
// default stream among them), like any other HIP API taking a stream.
hipStream_t streamOf(void* h) { return static_cast<hipStream_t>(h); }

// Operations of one context execute in call order, whatever streams they are given
// (they share the traversal spill area, the hit records and the atlases): an
// operation on another stream than the previous one first waits for it.
hipError_t orderBegin(ArkDdgiCtx* ctx, hipStream_t s)
{
    if (ctx->orderValid && ctx->orderStream != s) return hipStreamWaitEvent(s, ctx->evOrder, 0);
    return hipSuccess;
}

hipError_t orderEnd(ArkDdgiCtx* ctx, hipStream_t s)
{
    const hipError_t e = hipEventRecord(ctx->evOrder, s);
    ctx->orderStream = s;
    ctx->orderValid = e == hipSuccess;
    return e;
}

// Shading work set for the largest window: per-ray light bits, then k_shadow_gen's
// shadow-ray list (at most one ray per probe ray and light).
struct ShadeWorkLayout {
    uint64_t bits, list, total;
};

ShadeWorkLayout shadeWorkLayout(const ArkDdgiCtx* ctx)
{
    auto al = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t rays = static_cast<uint64_t>(ctx->Kmax) * ctx->Rmax;
    const uint64_t entries = rays * ctx->lightCount;
    ShadeWorkLayout w {};
    w.bits = 0;
    w.list = al(rays * 4);
    w.total = w.list + al(entries * sizeof(ShadowRay));
    return w;
}

int ensureShadeWork(ArkDdgiCtx* ctx)
{
    const uint64_t rays = static_cast<uint64_t>(ctx->Kmax) * ctx->Rmax;
    if (rays >= (1ull << 28) && ctx->lightCount > 0)
        return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "%llu rays per update: shadow-ray owners pack (ray << 4) | light in 32 bits", static_cast<unsigned long long>(rays));
    const ShadeWorkLayout w = shadeWorkLayout(ctx);
    if (ctx->shadeWork.bytes < w.total) ARK_HIP(ctx->shadeWork.alloc(w.total));
    return ARK_DDGI_OK;
}

// RT reflections' ray-list work set for `pixels` rays (ark_ddgi_rt_reflections)
// Workgroups of the persistent shadow traversal for `rays` closest-hit rays (~0.25
// shadow rays each on C4): the launch is a tail of the longest shadow rays when
// there are few, and fewer co-resident waves shorten each one's iterations
// (measured on C4: K = 2048 windows 0.228 -> 0.180 ms at 3 workgroups per CU,
// K = 4096 0.246 -> 0.225, the full grid (8.4 M rays) unchanged from 5 to 6).
constexpr uint64_t kShadowMinPerCu = 3; // 1 and 2 measured slower or within noise (profiles/r04_p)
uint32_t shadowBlocksFor(const ArkDdgiCtx* ctx, uint64_t rays)
{
    const uint64_t perCu = std::min<uint64_t>(ctx->shadowBlocksPerCu, std::max<uint64_t>(kShadowMinPerCu, rays >> 20));
    return static_cast<uint32_t>(perCu * ctx->cuCount);
}

int ensureReflWork(ArkDdgiCtx* ctx, uint64_t pixels)
{
    if (pixels >= (1ull << 28) && ctx->lightCount > 0)
        return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "%llu reflection rays: shadow-ray owners pack (ray << 4) | light in 32 bits", static_cast<unsigned long long>(pixels));
    auto al = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t bytes = al(pixels * 32) + al(pixels * sizeof(GpuHit)) + al(pixels * 4) + al((kRayCounterWords + kRayCounterStride) * 4) +
                           al(pixels * ctx->lightCount * sizeof(ShadowRay));
    if (ctx->reflWork.bytes < bytes) ARK_HIP(ctx->reflWork.alloc(bytes));
    return ARK_DDGI_OK;
}

static_assert(ARK_DDGI_MAX_SPOT_LIGHTS == kMaxLights - 1, "spot light capacity");

// The context's kernel view of its scene: the store's world BVHs, pools and tables with
// the context's own lights (sun by value, spots in its light buffer); the light-space
// sun BVH only while it is valid and the sun points the way it was built for (any other
// direction traces the sun's shadow rays through the world BVHs: same results).
void deriveSceneArgs(ArkDdgiCtx* ctx)
{
    const SceneStore& st = *ctx->sceneStore;
    SceneArgs sc = st.args;
    sc.has_sun = ctx->hasSun;
    for (int k = 0; k < 3; ++k) {
        sc.sun_color[k] = ctx->sunColor[k];
        sc.sun_dir[k] = ctx->sunDir[k];
    }
    sc.spot_count = static_cast<int32_t>(ctx->spotHost.size());
    sc.spots = ctx->lights.as<GpuSpotLight>();
    const bool sunOk = ctx->hasSun && st.sunArgs.sun_root >= 0 && std::memcmp(ctx->sunDir, st.sunDirBuilt, sizeof(ctx->sunDir)) == 0;
    sc.sun_nodes = sunOk ? st.sunArgs.sun_nodes : nullptr;
    sc.sun_tris = sunOk ? st.sunArgs.sun_tris : nullptr;
    sc.sun_root = sunOk ? st.sunArgs.sun_root : -1;
    std::memcpy(sc.sun_frame, st.sunArgs.sun_frame, sizeof(sc.sun_frame));
    // The sun's cover map only while it is the map of what this context traces: the front
    // copy's geometry (valid), this sun direction bit for bit, and shadow rays long enough
    // to reach every covering triangle (tmax = 2 zFar, shadowRayOf). Its frame is
    // sun_frame(dir): the light-space BVH's when that one is used too.
    const SceneStore::CoverMap& cm = st.coverMap;
    const bool mapOk = ctx->hasSun && !(ctx->desc.flags & ARK_DDGI_FLAG_NO_SUN_COVER_MAP) && cm.valid && cm.buf.ptr &&
                       std::memcmp(ctx->sunDir, cm.dir, sizeof(ctx->sunDir)) == 0 && 2.0f * ctx->desc.z_far >= cm.grid.wExtent;
    sc.sun_map = mapOk ? cm.buf.as<float2>() : nullptr;
    if (mapOk) {
        sc.sun_grid = cm.grid;
        sc.map_lift = cover::kTmin + cm.grid.margin;
        sc.map_reach = cover::kTmin - cm.grid.margin;
        std::memcpy(sc.sun_frame, cm.frame, sizeof(sc.sun_frame));
    }
    ctx->scene = sc;
    ctx->lightCount = (ctx->hasSun ? 1u : 0u) + static_cast<uint32_t>(ctx->spotHost.size());
    ctx->bvhStats = st.bvhStats;
    ctx->bvhMaxDepth = st.bvhMaxDepth;
    ctx->sceneVersion = st.version;
}

// deriveSceneArgs plus a traversal spill area deep enough for every BVH the derived
// args reach. Every caller goes through here: a sharing context may
// have installed a deeper sun BVH, and marking the store's version as seen without
// growing the spill area would let the next traversal overrun it.
int refreshScene(ArkDdgiCtx* ctx)
{
    deriveSceneArgs(ctx);
    return ensureSpill(ctx);
}

// The context's spot lights reach the device in stream order on `s`, ahead of the
// operation that reads them (a by-value kernel argument: no host buffer to keep alive).
hipError_t flushLights(ArkDdgiCtx* ctx, hipStream_t s)
{
    if (!ctx->lightsDirty) return hipSuccess;
    LightBlock b {};
    b.count = static_cast<uint32_t>(ctx->spotHost.size());
    std::copy(ctx->spotHost.begin(), ctx->spotHost.end(), b.spots);
    const hipError_t e = launch_store_lights(b, ctx->lights.as<GpuSpotLight>(), s);
    if (e == hipSuccess) ctx->lightsDirty = false;
    return e;
}

// Waits for every operation of the context enqueued so far (both of its streams).
hipError_t drainContext(ArkDdgiCtx* ctx)
{
    hipError_t e = hipStreamSynchronize(ctx->traceStream);
    if (e == hipSuccess && ctx->orderValid) e = hipEventSynchronize(ctx->evOrder);
    return e;
}

// What the scene's calls (scene_store.h) take from the calling context
SceneCall sceneCall(ArkDdgiCtx* ctx)
{
    SceneCall c {};
    c.err = ctx;
    c.flags = ctx->desc.flags;
    c.hasSun = ctx->hasSun != 0;
    std::copy(ctx->sunDir, ctx->sunDir + 3, c.sunDir);
    c.shared = ctx->sceneStore.use_count() > 1;
    return c;
}

// Makes `st` the context's scene with the scene's lights: the per-context work sets
// follow its light count and BVH depth. The device is idle (set_scene, share_scene):
// every refit and install of `st` so far is done.
int adoptScene(ArkDdgiCtx* ctx, std::shared_ptr<SceneStore> st)
{
    ctx->geometrySeen = st->geometrySeq;
    ctx->seedStale = true; // another scene's records
    ctx->hasSun = st->hasSunScene;
    for (int k = 0; k < 3; ++k) {
        ctx->sunColor[k] = st->sunScene.color[k];
        ctx->sunDir[k] = st->sunScene.world_space_direction[k];
    }
    ctx->spotHost = st->spotsScene;
    ctx->sceneStore = std::move(st);
    if (!ctx->lights.ptr) ARK_HIP(ctx->lights.alloc((kMaxLights - 1) * sizeof(GpuSpotLight)));
    if (!ctx->spotHost.empty()) ARK_HIP(hipMemcpy(ctx->lights.ptr, ctx->spotHost.data(), ctx->spotHost.size() * sizeof(GpuSpotLight), hipMemcpyHostToDevice));
    ctx->lightsDirty = false;
    deriveSceneArgs(ctx);
    int rc;
    if ((rc = ensureShadeWork(ctx)) != 0) return rc;
    if ((rc = ensureSpill(ctx)) != 0) return rc;
    ctx->hasScene = true;
    return ARK_DDGI_OK;
}

} // namespace

extern "C" {

int32_t ark_ddgi_abi_version(void) { return ARK_DDGI_ABI_VERSION; }

int ark_ddgi_create(const ArkDdgiDesc* desc, ArkDdgiCtx** outCtx)
{
    if (!desc || !outCtx || desc->struct_size != sizeof(ArkDdgiDesc)) return ARK_DDGI_E_INVALID_ARGUMENT;
    *outCtx = nullptr;
    if (desc->grid_dims[0] <= 0 || desc->grid_dims[1] <= 0 || desc->grid_dims[2] <= 0) return ARK_DDGI_E_NO_PROBE_GRID;
    auto* ctx = new ArkDdgiCtx();
    ctx->desc = *desc;
    ctx->X = desc->grid_dims[0];
    ctx->Y = desc->grid_dims[1];
    ctx->Z = desc->grid_dims[2];
    ctx->N = ctx->X * ctx->Y * ctx->Z;
    ctx->Rmax = desc->max_rays_per_probe > 0 ? desc->max_rays_per_probe : ARK_DDGI_MAX_RAYS_PER_PROBE;
    ctx->Kmax = desc->max_probe_updates > 0 ? desc->max_probe_updates : ARK_DDGI_REFERENCE_MAX_PROBE_UPDATES;
    const int shards = desc->shard_count > 0 ? desc->shard_count : 1;
    if (ctx->Rmax > ARK_DDGI_MAX_RAYS_PER_PROBE || ctx->Z % shards != 0 || desc->shard_rank < 0 || desc->shard_rank >= shards ||
        desc->sun_bvh < ARK_DDGI_SUN_BVH_AUTO || desc->sun_bvh > ARK_DDGI_SUN_BVH_LIGHT_SPACE || (desc->flags & ~(ARK_DDGI_FLAG_SERIAL_FRAMES | ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD | ARK_DDGI_FLAG_GPU_REBUILD | ARK_DDGI_FLAG_GPU_REBUILD_SUN | ARK_DDGI_FLAG_GPU_REBUILD_SAH | ARK_DDGI_FLAG_GPU_REBUILD_PLAN | ARK_DDGI_FLAG_NO_SUN_COVER_MAP | ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE | ARK_DDGI_FLAG_NO_RAY_SEEDS)) ||
        desc->build_threads < 0) {
        delete ctx;
        return ARK_DDGI_E_INVALID_ARGUMENT;
    }
    ctx->desc.shard_count = shards;
    ctx->slabZ0 = desc->shard_rank * (ctx->Z / shards);
    ctx->slabZ1 = ctx->slabZ0 + ctx->Z / shards;
    const int si = ARK_DDGI_IRRADIANCE_RES + 2 * ARK_DDGI_ATLAS_PADDING;
    const int sv = ARK_DDGI_VISIBILITY_RES + 2 * ARK_DDGI_ATLAS_PADDING;
    ctx->Wi = ctx->X * si * ctx->Y;
    ctx->Hi = ctx->Z * si;
    ctx->Wv = ctx->X * sv * ctx->Y;
    ctx->Hv = ctx->Z * sv;
    auto bad = [&](hipError_t e, const char* what) {
        std::fprintf(stderr, "ark_ddgi_create: %s: %s\n", what, hipGetErrorString(e));
        delete ctx;
        return ARK_DDGI_E_DEVICE;
    };
    hipError_t e = hipSetDevice(desc->device);
    if (e != hipSuccess) return bad(e, "hipSetDevice");
    ctx->device = desc->device;
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, desc->device);
    if (e != hipSuccess) return bad(e, "hipGetDeviceProperties");
    ctx->cuCount = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return bad(e, "hipStreamCreate");
    if ((e = hipEventCreateWithFlags(&ctx->evOrder, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    // the desc's options (ArkDdgiDesc.sun_bvh / flags); the traversal's refill and grab
    // sizes are the constants kRefillMin / kSunRefillMin / kGrabChunk
    ctx->pipelining = (desc->flags & ARK_DDGI_FLAG_SERIAL_FRAMES) == 0;
    ctx->sunBvh = desc->sun_bvh == ARK_DDGI_SUN_BVH_WORLD ? 0 : desc->sun_bvh == ARK_DDGI_SUN_BVH_LIGHT_SPACE ? 1 : -1;
    // a counter-collecting profiler (rocprofv3 --pmc) runs one kernel at a time across
    // queues: a polling wait could then hold the GPU while the kernel it waits for queues
    // behind it: it would give up after its bound and fail closed (checkSequencing),
    // dropping frames; such a context starts with events instead (the profiler's own
    // environment, not a tuning knob; ark_ddgi_set_sequencing overrides it)
    if (const char* pc = std::getenv("ROCPROF_COUNTER_COLLECTION"))
        if (*pc && std::strcmp(pc, "0") != 0 && std::strcmp(pc, "false") != 0) ctx->seqSync = false;
    if ((e = hipStreamCreateWithFlags(&ctx->traceStream, hipStreamNonBlocking)) != hipSuccess) return bad(e, "hipStreamCreate");
    // stream-order events of the frames in flight
    const unsigned syncFlags = hipEventDisableTiming;
    if ((e = hipEventCreateWithFlags(&ctx->evTraced, syncFlags)) != hipSuccess) return bad(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&ctx->evExchangeSrc, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&ctx->evExchangeDone, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    for (auto& ev : ctx->evFrameDone)
        if ((e = hipEventCreateWithFlags(&ev, syncFlags)) != hipSuccess) return bad(e, "hipEventCreate");
    for (auto& ev : ctx->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return bad(e, "hipEventCreate");
    const size_t K = static_cast<size_t>(ctx->Kmax), R = static_cast<size_t>(ctx->Rmax);
    if ((e = ctx->irr.alloc(static_cast<size_t>(ctx->Wi) * ctx->Hi * 8)) != hipSuccess) return bad(e, "alloc irradiance");
    if ((e = ctx->vis.alloc(static_cast<size_t>(ctx->Wv) * ctx->Hv * 4)) != hipSuccess) return bad(e, "alloc visibility");
    if ((e = ctx->offsets.alloc(static_cast<size_t>(ctx->N) * 16)) != hipSuccess) return bad(e, "alloc offsets");
    if ((e = ctx->slots.alloc(2 * K * sizeof(GpuProbeSlot))) != hipSuccess) return bad(e, "alloc slots");
    if ((e = ctx->slotOrder.alloc(2 * K * 4)) != hipSuccess) return bad(e, "alloc slot order");
    if ((e = ctx->fib.alloc(2 * R * 16)) != hipSuccess) return bad(e, "alloc fib");
    if ((e = ctx->order.alloc(R * 4)) != hipSuccess) return bad(e, "alloc order");
    if ((e = ctx->fibOrder.alloc(2 * R * 16)) != hipSuccess) return bad(e, "alloc fib order");
    if ((e = ctx->hits.alloc(2 * K * R * sizeof(GpuHit))) != hipSuccess) return bad(e, "alloc hits");
    if ((e = ctx->surfels.alloc(K * R * 8)) != hipSuccess) return bad(e, "alloc surfels");
    if ((e = ctx->rayCounter.alloc(2 * kRayCounterWords * 4)) != hipSuccess) return bad(e, "alloc counter");
    if ((e = ctx->counters.alloc(10 * sizeof(unsigned long long))) != hipSuccess) return bad(e, "alloc counters");
    if (!(desc->flags & ARK_DDGI_FLAG_NO_RAY_SEEDS)) {
        // (filled with seed::kNone by the first update: seedStale)
        if ((e = ctx->seeds.alloc(static_cast<size_t>(ctx->N) * seed::kProbeWords * 4)) != hipSuccess) return bad(e, "alloc seed cache");
    }
    if ((e = ctx->seqWords.alloc(128 * 4)) != hipSuccess) return bad(e, "alloc sequence words");
    if ((e = hipMemset(ctx->seqWords.ptr, 0, ctx->seqWords.bytes)) != hipSuccess) return bad(e, "clear sequence words");
    {
        // k_seq_wait's bound: 10 s of the device wall clock (kHz attribute)
        int rateKhz = 0;
        if (hipDeviceGetAttribute(&rateKhz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || rateKhz <= 0) rateKhz = 100000;
        ctx->wallClockKhz = static_cast<uint64_t>(rateKhz);
        ctx->seqTimeoutTicks = ctx->wallClockKhz * ctx->seqTimeoutMs;
    }
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&ctx->hostAbort), 64, hipHostMallocCoherent | hipHostMallocMapped)) != hipSuccess)
        return bad(e, "hipHostMalloc sequencing flag");
    *reinterpret_cast<volatile uint32_t*>(ctx->hostAbort) = 0u;
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->hostAbortDev), ctx->hostAbort, 0)) != hipSuccess)
        return bad(e, "hipHostGetDevicePointer sequencing flag");
    // persistent grids: as many workgroups as are co-resident
    int occT = 0, occS = 0, occW = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occT, kernel_trace_ptr(false), kTraceBlock, 0)) != hipSuccess) return bad(e, "occupancy trace");
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occS, kernel_shade_ptr(false), kShadeBlock, 0)) != hipSuccess) return bad(e, "occupancy shade");
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occW, kernel_trace_shadow_ptr(false), kTraceBlock, 0)) != hipSuccess) return bad(e, "occupancy shadow");
    ctx->traceBlocks = static_cast<uint32_t>(std::max(1, occT) * ctx->cuCount);
    // a pipelined update's traversal shares the GPU with the previous frame's shadow
    // rays, shading and probe update: below kPipeHalfRays rays, 3 workgroups per CU
    // (half the occupancy) leave them room (tools/shard_proxy.py,
    // tools/window_proxy.py, profiles/r02_m13-15: Z-slab steps P = 8 0.705 -> 0.640 ms,
    // P = 4 1.21 -> 1.11, P = 2 2.22 -> 2.10; K = 4096 windows 0.72 -> 0.65, K = 2048
    // 0.43 unchanged; 2 per CU: P = 8 0.72, 4 per CU: 0.69). The whole C4 grid (8.4 M
    // rays) keeps the full grid: 4.059 vs 4.067 ms per step at 3 (profiles/r02_m17_ab).
    ctx->pipeTraceBlocks = static_cast<uint32_t>(std::min(kPipeTracePerCu, std::max(1, occT)) * ctx->cuCount);
    ctx->shadeBlocks = static_cast<uint32_t>(std::max(1, occS) * ctx->cuCount);
    ctx->shadowBlocks = static_cast<uint32_t>(std::max(1, occW) * ctx->cuCount);
    ctx->shadowBlocksPerCu = static_cast<uint32_t>(std::max(1, occW));
    if (clearHistory(ctx) != ARK_DDGI_OK) {
        std::fprintf(stderr, "ark_ddgi_create: %s\n", ctx->lastError.c_str());
        delete ctx;
        return ARK_DDGI_E_DEVICE;
    }
    *outCtx = ctx;
    return ARK_DDGI_OK;
}

void ark_ddgi_destroy(ArkDdgiCtx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (DeviceBuffer* b : { &ctx->irr, &ctx->vis, &ctx->offsets, &ctx->slots, &ctx->slotOrder, &ctx->fib, &ctx->fibOrder, &ctx->order, &ctx->hits, &ctx->surfels, &ctx->spill, &ctx->rayCounter, &ctx->seqWords, &ctx->shadeWork, &ctx->reflWork,
                             &ctx->raySteps, &ctx->seeds, &ctx->counters, &ctx->lights, &ctx->bakeTri, &ctx->bakeBary, &ctx->bakeOut, &ctx->bakePixels, &ctx->bakeCounters })
        b->release();
    ctx->sceneStore.reset();
    for (auto& ev : ctx->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->evOrder) (void)hipEventDestroy(ctx->evOrder);
    if (ctx->evTraced) (void)hipEventDestroy(ctx->evTraced);
    if (ctx->evExchangeSrc) (void)hipEventDestroy(ctx->evExchangeSrc);
    if (ctx->evExchangeDone) (void)hipEventDestroy(ctx->evExchangeDone);
    for (auto& ev : ctx->evFrameDone)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->traceStream) (void)hipStreamDestroy(ctx->traceStream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->hostAbort) (void)hipHostFree(ctx->hostAbort);
    delete ctx;
}

const char* ark_ddgi_last_error(const ArkDdgiCtx* ctx) { return ctx ? ctx->lastError.c_str() : "null context"; }

int ark_ddgi_set_scene(ArkDdgiCtx* ctx, const ArkDdgiScene* s)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->pipeReady = false; // the next update's traversal waits for this
    if (!s || s->struct_size != sizeof(ArkDdgiScene)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkDdgiScene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    // the previous scene goes first (its memory is reused), unless another context
    // shares it; a failure below leaves the context without a scene
    ctx->hasScene = false;
    ctx->sceneStore.reset();
    std::shared_ptr<SceneStore> st;
    if (const int rc = buildScene(ctx, s, ctx->device, ctx->desc.build_threads, ctx->sunBvh, (ctx->desc.flags & ARK_DDGI_FLAG_NO_SUN_COVER_MAP) == 0, st)) return rc;
    return adoptScene(ctx, std::move(st));
}

int ark_ddgi_share_scene(ArkDdgiCtx* ctx, const ArkDdgiCtx* src)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->pipeReady = false; // the next update's traversal waits for this
    if (!src || src == ctx || !src->hasScene || !src->sceneStore) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "share_scene: the source context has no scene");
    if (src->device != ctx->device) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "share_scene: contexts on devices %d and %d", src->device, ctx->device);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    std::shared_ptr<SceneStore> st = src->sceneStore;
    ctx->hasScene = false;
    ctx->sceneStore.reset();
    return adoptScene(ctx, std::move(st));
}

int ark_ddgi_set_lights(ArkDdgiCtx* ctx, const ArkDdgiLights* L)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!L || L->struct_size != sizeof(ArkDdgiLights)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkDdgiLights");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_set_lights before ark_ddgi_set_scene");
    if (L->spot_light_count > ARK_DDGI_MAX_SPOT_LIGHTS) return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "at most %d spot lights (GpuScene.cpp:430)", ARK_DDGI_MAX_SPOT_LIGHTS);
    if (L->spot_light_count && !L->spot_lights) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_lights: null spot_lights");
    std::vector<GpuSpotLight> spots(L->spot_light_count);
    for (uint32_t i = 0; i < L->spot_light_count; ++i) spots[i] = gpuSpotLight(L->spot_lights[i]);
    const uint32_t count = (L->has_directional_light ? 1u : 0u) + L->spot_light_count;
    ARK_HIP(hipSetDevice(ctx->device));
    if (count > ctx->lightCount) {
        // the shadow-ray list holds one ray per probe ray and light: grow it once the
        // frames in flight (which use it) are done
        const ShadeWorkLayout need = [&] {
            const uint32_t keep = ctx->lightCount;
            ctx->lightCount = count;
            const ShadeWorkLayout w = shadeWorkLayout(ctx);
            ctx->lightCount = keep;
            return w;
        }();
        if (ctx->shadeWork.bytes < need.total) {
            ARK_HIP(drainContext(ctx));
            const uint32_t keep = ctx->lightCount;
            ctx->lightCount = count;
            const int rc = ensureShadeWork(ctx);
            ctx->lightCount = keep;
            if (rc) return rc;
        }
    }
    ctx->hasSun = L->has_directional_light ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
        ctx->sunColor[k] = ctx->hasSun ? L->directional_light.color[k] : 0.0f;
        ctx->sunDir[k] = ctx->hasSun ? L->directional_light.world_space_direction[k] : 0.0f;
    }
    if (spots.size() != ctx->spotHost.size() || (!spots.empty() && std::memcmp(spots.data(), ctx->spotHost.data(), spots.size() * sizeof(GpuSpotLight)) != 0)) {
        ctx->spotHost = std::move(spots);
        ctx->lightsDirty = true;
    }
    if (const int rc = refreshScene(ctx)) return rc;
    // a sun rebuild to start or install: on the context's internal stream, in call order
    // (orderBegin / orderEnd) only when one is, so that a frame with no rebuild costs the
    // next update no cross-stream wait
    SceneStore& st = *ctx->sceneStore;
    const SceneCall c = sceneCall(ctx);
    if (!sunStepMayEnqueue(st, c)) return sceneSunStep(st, c, nullptr, false); // (enqueues nothing: no stream ordered)
    const uint32_t v = st.version;
    const bool hadJob = sunJobPending(st);
    ARK_HIP(orderBegin(ctx, ctx->stream));
    if (const int rc = sceneSunStep(st, c, ctx->stream, true)) return rc;
    if (st.version != v || sunJobPending(st) != hadJob) ARK_HIP(orderEnd(ctx, ctx->stream));
    if (ctx->sceneVersion != st.version) return refreshScene(ctx); // an installed sun BVH
    return ARK_DDGI_OK;
}

static int checkSequencing(ArkDdgiCtx* ctx);

int ark_ddgi_set_instances_async(ArkDdgiCtx* ctx, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_set_instances before ark_ddgi_set_scene");
    SceneStore& st = *ctx->sceneStore;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(orderBegin(ctx, s));
    // the refit of the next geometry copy on the store's stream, which `s` then follows;
    // finished background rebuilds installed and new ones started on `s`
    if (const int rc = sceneSetInstances(st, sceneCall(ctx), instances, count, s)) return rc;
    if (ctx->sceneVersion != st.version)
        if (const int rc = refreshScene(ctx)) return rc;
    ARK_HIP(orderEnd(ctx, s));
    st.bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ARK_DDGI_OK;
}

int ark_ddgi_update_geometry_async(ArkDdgiCtx* ctx, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_update_geometry before ark_ddgi_set_scene");
    SceneStore& st = *ctx->sceneStore;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(orderBegin(ctx, s));
    // set_instances' refit with the vertex ranges written first (scene_store.h)
    if (const int rc = sceneUpdateGeometry(st, sceneCall(ctx), updates, updateCount, instances, count, s)) return rc;
    if (ctx->sceneVersion != st.version)
        if (const int rc = refreshScene(ctx)) return rc;
    ARK_HIP(orderEnd(ctx, s));
    st.bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ARK_DDGI_OK;
}

int ark_ddgi_register_skin(ArkDdgiCtx* ctx, const ArkDdgiSkinDesc* desc, uint32_t* outSkin)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_register_skin before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    return sceneRegisterSkin(*ctx->sceneStore, ctx, desc, outSkin);
}

int ark_ddgi_unregister_skin(ArkDdgiCtx* ctx, uint32_t skin)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_unregister_skin before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    return sceneUnregisterSkin(*ctx->sceneStore, ctx, skin);
}

int ark_ddgi_skin_geometry_async(ArkDdgiCtx* ctx, const ArkDdgiSkinPose* poses, uint32_t poseCount, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_skin_geometry before ark_ddgi_set_scene");
    SceneStore& st = *ctx->sceneStore;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(orderBegin(ctx, s));
    // the skins' runs on `s`, then update_geometry's refit with their outputs as device sources
    if (const int rc = sceneSkinGeometry(st, sceneCall(ctx), poses, poseCount, instances, count, s)) return rc;
    if (ctx->sceneVersion != st.version)
        if (const int rc = refreshScene(ctx)) return rc;
    ARK_HIP(orderEnd(ctx, s));
    st.bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ARK_DDGI_OK;
}

int ark_ddgi_skin_geometry(ArkDdgiCtx* ctx, const ArkDdgiSkinPose* poses, uint32_t poseCount, const ArkRTInstance* instances, uint32_t count)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = ark_ddgi_skin_geometry_async(ctx, poses, poseCount, instances, count, ctx->stream)) return rc;
    ARK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sceneStore->bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->bvhStats = ctx->sceneStore->bvhStats;
    return ARK_DDGI_OK;
}

int ark_ddgi_get_skin_views(ArkDdgiCtx* ctx, uint32_t skin, ArkDdgiSkinViews* out)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_get_skin_views before ark_ddgi_set_scene");
    return sceneSkinViews(*ctx->sceneStore, ctx, skin, out);
}

int ark_ddgi_get_skin_stats(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::fill(out, out + 4, uint64_t(0));
    if (ctx->hasScene) sceneSkinStats(*ctx->sceneStore, out);
    return ARK_DDGI_OK;
}

int ark_ddgi_get_geometry_update_stats(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::fill(out, out + 4, uint64_t(0));
    if (!ctx->hasScene) return ARK_DDGI_OK;
    ARK_HIP(hipSetDevice(ctx->device));
    return sceneGeometryStats(*ctx->sceneStore, ctx, out);
}

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

int ark_ddgi_update_geometry(ArkDdgiCtx* ctx, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = ark_ddgi_update_geometry_async(ctx, updates, updateCount, instances, count, ctx->stream)) return rc;
    ARK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sceneStore->bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->bvhStats = ctx->sceneStore->bvhStats;
    return ARK_DDGI_OK;
}

int ark_ddgi_set_instances(ArkDdgiCtx* ctx, const ArkRTInstance* instances, uint32_t count)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = ark_ddgi_set_instances_async(ctx, instances, count, ctx->stream)) return rc;
    ARK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sceneStore->bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->bvhStats = ctx->sceneStore->bvhStats;
    return ARK_DDGI_OK;
}

static uint32_t countSlabProbes(const ArkDdgiCtx* ctx, uint32_t first, uint32_t K)
{
    if (ctx->desc.shard_count <= 1) return K;
    return slabRankOf(static_cast<uint32_t>(ctx->X), static_cast<uint32_t>(ctx->Y), static_cast<uint32_t>(ctx->Z), static_cast<uint32_t>(ctx->slabZ0),
                      static_cast<uint32_t>(ctx->slabZ1), first, K);
}

static int updateImpl(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, void* hipStream, void* shadeWaitEvent, void* doneEvent, uint32_t shadeWaitSeq = 0);

// Fail-closed frame sequencing (VERDICT r03 "do this" #3): a k_seq_wait that gave up
// has set the context's timed-out word, so every path kernel that starts after it
// skips (frameAborted) and leaves atlases, surfels and offsets as they were (a launch
// already running when the wait gave up completes). The first context
// call that sees the host-mapped flag drains the device (the late producer ends by
// itself), clears both words, switches the context to event sequencing (which no
// queue order can stall) and reports ARK_DDGI_E_DEVICE; the calls after it run.
static int checkSequencing(ArkDdgiCtx* ctx)
{
    if (!ctx->hostAbort || __atomic_load_n(ctx->hostAbort, __ATOMIC_ACQUIRE) == 0u) return ARK_DDGI_OK;
    ARK_HIP(hipSetDevice(ctx->device));
    // the whole device (ADVICE r04 low asked for the context's own streams only): the
    // late producer may sit on a caller's stream (an exchange stream) whose end the
    // context recorded as a sequence word; once the context switches to events, nothing
    // else would order the next frame's shading after it
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemset(ctx->seqWords.as<uint32_t>() + 64, 0, 4));
    __atomic_store_n(ctx->hostAbort, 0u, __ATOMIC_RELEASE);
    ctx->seqSync = false;
    ctx->pipeReady = false;
    ++ctx->seqTimeouts;
    return ctx->fail(ARK_DDGI_E_DEVICE,
                     "a frame-sequencing wait between the context's streams gave up after %u ms: every update kernel that started after it skipped "
                     "(its atlases, surfels and offsets left as they were); the context now orders its streams with events",
                     ctx->seqTimeoutMs);
}

int ark_ddgi_set_sequencing(ArkDdgiCtx* ctx, int device_sequence_words, uint32_t timeout_ms)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (timeout_ms > 3600u * 1000u) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "sequencing timeout %u ms above one hour", timeout_ms);
    ctx->seqSync = device_sequence_words != 0;
    if (timeout_ms) {
        ctx->seqTimeoutMs = timeout_ms;
        ctx->seqTimeoutTicks = ctx->wallClockKhz * timeout_ms;
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_get_sequencing(const ArkDdgiCtx* ctx, int* out_device_sequence_words, uint32_t* out_timeout_ms, uint32_t* out_timeouts)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (out_device_sequence_words) *out_device_sequence_words = ctx->seqSync ? 1 : 0;
    if (out_timeout_ms) *out_timeout_ms = ctx->seqTimeoutMs;
    if (out_timeouts) *out_timeouts = ctx->seqTimeouts;
    return ARK_DDGI_OK;
}


int ark_ddgi_update(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, void* hipStream)
{
    return updateImpl(ctx, p, hipStream, nullptr, nullptr);
}

int ark_ddgi_update_overlapped(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, void* hipStream, void* shadeWaitEvent, void* doneEvent)
{
    return updateImpl(ctx, p, hipStream, shadeWaitEvent, doneEvent);
}

int ark_ddgi_update_exchanged(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const uint32_t wait = ctx->pendingExchange;
    // without sequence words the exchange's end is an event (ark_ddgi_exchange_end)
    const int r = ctx->seqSync ? updateImpl(ctx, p, hipStream, nullptr, nullptr, wait)
                               : updateImpl(ctx, p, hipStream, wait ? ctx->evExchangeDone : nullptr, nullptr);
    if (r == ARK_DDGI_OK) ctx->pendingExchange = 0;
    return r;
}

int ark_ddgi_exchange_begin(ArkDdgiCtx* ctx, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const hipStream_t x = streamOf(hipStream);
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(hipSetDevice(ctx->device));
    if (ctx->lastMainSeq) {
        uint32_t* w = ctx->seqWords.as<uint32_t>();
        ARK_HIP(launch_seq_wait(w + 32, ctx->lastMainSeq, w + 64, ctx->hostAbortDev, ctx->seqTimeoutTicks, x));
    } else {
        // the last update was not sequenced: everything enqueued on its stream so far
        ARK_HIP(hipEventRecord(ctx->evExchangeSrc, ctx->lastStream));
        ARK_HIP(hipStreamWaitEvent(x, ctx->evExchangeSrc, 0));
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_exchange_end(ArkDdgiCtx* ctx, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ARK_HIP(hipSetDevice(ctx->device));
    const uint32_t n = ++ctx->exchSeq;
    if (ctx->seqSync) ARK_HIP(launch_seq_signal(ctx->seqWords.as<uint32_t>() + 96, n, streamOf(hipStream)));
    else ARK_HIP(hipEventRecord(ctx->evExchangeDone, streamOf(hipStream)));
    ctx->pendingExchange = n;
    return ARK_DDGI_OK;
}

static ArkDdgiWindowExchange windowExchangeInfo(const ArkDdgiCtx* ctx)
{
    ArkDdgiWindowExchange w {};
    w.struct_size = sizeof(w);
    w.first_probe = ctx->lastFirst;
    w.probe_updates = ctx->lastK;
    const uint32_t P = static_cast<uint32_t>(ctx->desc.shard_count), Zs = static_cast<uint32_t>(ctx->Z) / P;
    w.full_bands = ctx->lastK == static_cast<uint32_t>(ctx->N) ? 1u : 0u;
    for (uint32_t q = 0; q < P; ++q) {
        const uint32_t n = slabRankOf(static_cast<uint32_t>(ctx->X), static_cast<uint32_t>(ctx->Y), static_cast<uint32_t>(ctx->Z), q * Zs, (q + 1) * Zs, ctx->lastFirst,
                                      ctx->lastK);
        w.probes_per_rank = std::max(w.probes_per_rank, n);
        if (q == static_cast<uint32_t>(ctx->desc.shard_rank)) w.my_probes = n;
    }
    w.bytes_per_rank = w.full_bands ? 0u : static_cast<uint64_t>(w.probes_per_rank) * kWindowPacketBytes;
    return w;
}

int ark_ddgi_window_exchange_info(const ArkDdgiCtx* ctx, ArkDdgiWindowExchange* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    *out = windowExchangeInfo(ctx);
    return ARK_DDGI_OK;
}

static int windowPack(ArkDdgiCtx* ctx, void* buf, uint64_t bytes, void* hipStream, bool unpack)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const ArkDdgiWindowExchange w = windowExchangeInfo(ctx);
    if (w.full_bands) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "window exchange: the last window covered the grid (exchange the bands)");
    const uint64_t need = unpack ? w.bytes_per_rank * static_cast<uint64_t>(ctx->desc.shard_count) : w.bytes_per_rank;
    if (bytes != need) return ctx->fail(ARK_DDGI_E_SIZE_MISMATCH, "window exchange: %llu bytes, the window needs %llu", (unsigned long long)bytes, (unsigned long long)need);
    if (need && !buf) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "window exchange: null buffer");
    ARK_HIP(hipSetDevice(ctx->device));
    WindowExchangeArgs a {};
    a.X = ctx->X; a.Y = ctx->Y; a.Z = ctx->Z; a.N = ctx->N;
    a.first = ctx->lastFirst;
    a.K = ctx->lastK;
    a.Wi = ctx->Wi; a.Wv = ctx->Wv;
    a.slabDepth = static_cast<uint32_t>(ctx->Z / ctx->desc.shard_count);
    a.rank = static_cast<uint32_t>(ctx->desc.shard_rank);
    a.world = static_cast<uint32_t>(ctx->desc.shard_count);
    a.bytesPerRank = w.bytes_per_rank;
    a.irr = ctx->irr.as<uint16_t>();
    a.vis = ctx->vis.as<uint16_t>();
    a.buf = static_cast<uint8_t*>(buf);
    if (need) ARK_HIP(launch_window_pack(a, unpack, streamOf(hipStream)));
    return ARK_DDGI_OK;
}

int ark_ddgi_pack_window(ArkDdgiCtx* ctx, void* dst, uint64_t bytes, void* hipStream) { return windowPack(ctx, dst, bytes, hipStream, false); }

int ark_ddgi_unpack_window(ArkDdgiCtx* ctx, const void* src, uint64_t bytes, void* hipStream)
{
    return windowPack(ctx, const_cast<void*>(src), bytes, hipStream, true);
}

// The caller's stream s waits for the traversal stream's part of a pipelined frame
// (slot table, traversal, offsets): device-side sequencing, or an event.
static hipError_t tracedSync(ArkDdgiCtx* ctx, bool seq, uint32_t seqN, hipStream_t ts, hipStream_t s)
{
    if (seq) {
        uint32_t* w = ctx->seqWords.as<uint32_t>();
        hipError_t e = launch_seq_signal(w, seqN, ts);
        return e != hipSuccess ? e : launch_seq_wait(w, seqN, w + 64, ctx->hostAbortDev, ctx->seqTimeoutTicks, s);
    }
    hipError_t e = hipEventRecord(ctx->evTraced, ts);
    return e != hipSuccess ? e : hipStreamWaitEvent(s, ctx->evTraced, 0);
}

static int updateImpl(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, void* hipStream, void* shadeWaitEvent, void* doneEvent, uint32_t shadeWaitSeq)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!p || p->struct_size != sizeof(ArkDdgiFrameParams)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkDdgiFrameParams");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_update before ark_ddgi_set_scene");
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const uint32_t K = std::min(p->probe_updates, N);
    const uint32_t R = p->rays_per_probe;
    if (K == 0 || R == 0 || K > static_cast<uint32_t>(ctx->Kmax) || R > static_cast<uint32_t>(ctx->Rmax))
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "probe_updates %u / rays_per_probe %u outside [1,%d] / [1,%d]", K, R, ctx->Kmax, ctx->Rmax);
    const hipStream_t s = streamOf(hipStream);
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(hipSetDevice(ctx->device));
    FrameArgs f {};
    f.abort_word = ctx->seqWords.as<uint32_t>() + 64;
    f.X = ctx->X; f.Y = ctx->Y; f.Z = ctx->Z;
    f.Wi = ctx->Wi; f.Hi = ctx->Hi; f.Wv = ctx->Wv; f.Hv = ctx->Hv;
    for (int k = 0; k < 3; ++k) {
        f.spacing[k] = ctx->desc.probe_spacing[k];
        f.origin[k] = ctx->desc.offset_to_first[k];
    }
    f.z_far = ctx->desc.z_far;
    f.frame = p->frame_index;
    f.first = p->first_probe_index % N;
    f.window = K;
    f.sharded = ctx->desc.shard_count > 1 ? 1 : 0;
    f.slab_z0 = ctx->slabZ0;
    f.slab_z1 = ctx->slabZ1;
    f.window_probes = countSlabProbes(ctx, f.first, K);
    f.R = R;
    f.Rmax = static_cast<uint32_t>(ctx->Rmax);
    f.window_rays = f.window_probes * R;
    f.hysteresis_irradiance = p->hysteresis_irradiance;
    f.hysteresis_visibility = p->hysteresis_visibility;
    f.visibility_sharpness = p->visibility_sharpness;
    f.ambient_amount = p->ambient_amount;
    f.environment_multiplier = p->environment_multiplier;
    f.delta_time = p->delta_time;
    f.update_offsets = p->update_offsets;
    f.irr = ctx->irr.as<uint16_t>();
    f.vis = ctx->vis.as<uint16_t>();
    f.offsets = ctx->offsets.as<float4>();
    const bool timing = ctx->timing;
    const bool count = ctx->counting;
    // Frames in flight: this frame's slot table, traversal and probe offsets read the
    // scene, the sample order and the probe offsets only, which nothing of the
    // previous frame's shadow rays, shading or atlas update writes (its offsets ran
    // before them). They may start before the previous frame is done when the sample
    // order is the same and no other writing context operation came in between.
    // Instrumented updates (per-kernel events, counters) run serially.
    const bool pipe = ctx->pipelining && ctx->pipeReady && !timing && !count && R == ctx->prevR;
    const uint32_t b = ctx->parity;
    const uint64_t Kmax = static_cast<uint64_t>(ctx->Kmax), Rmax = static_cast<uint64_t>(ctx->Rmax);
    f.slots = ctx->slots.as<GpuProbeSlot>() + b * Kmax;
    f.fib = ctx->fib.as<float4>() + b * Rmax;
    RoctxRange ddgiZone("DDGI");
    ARK_HIP(orderBegin(ctx, s));
    // finished background rebuilds installed (and refitted forward) on s, new ones started
    if (const int rc = sceneMaintenance(*ctx->sceneStore, sceneCall(ctx), s)) return rc;
    if (ctx->sceneVersion != ctx->sceneStore->version) // a rebuild installed above, or a sharing context refitted the scene or installed one
        if (const int rc = refreshScene(ctx)) return rc;
    // lights changed since the last update: stored ahead of this frame's shadow rays and
    // shading on s (the traversal on the traversal stream reads no light)
    ARK_HIP(flushLights(ctx, s));
    if (ctx->orderR != R) {
        sampleTraversalOrder(R, ctx->orderHost);
        ARK_HIP(hipMemcpyAsync(ctx->order.ptr, ctx->orderHost.data(), R * 4, hipMemcpyHostToDevice, s));
        ctx->orderR = R;
    }
    f.order = ctx->order.as<uint32_t>();
    f.fib_order = ctx->fibOrder.as<float4>() + b * Rmax;
    f.hits = ctx->hits.as<GpuHit>() + b * Kmax * Rmax;
    f.surfels = ctx->surfels.as<uint16_t>();
    f.spill = ctx->spill.as<uint32_t>() + ctx->spillRegionWords; // region 1 (primary traversal)
    f.light_count = ctx->lightCount;
    f.refill_min = ctx->refillMin;
    f.sun_refill_min = ctx->sunRefillMin;
    // a half-occupancy window (below kPipeHalfRays) hands out 32 rays per partition-head
    // grab to the probe-ray and shadow-ray queues (K = 2048 windows 0.429 -> 0.420 ms;
    // the whole grid keeps 64: 4.13 vs 4.18 ms at 32, profiles/r02_m19)
    f.grab_chunk = (pipe && f.window_rays < kPipeHalfRays) ? std::min<uint32_t>(ctx->grabChunk, 32u) : ctx->grabChunk;
    f.ray_counter = ctx->rayCounter.as<uint32_t>() + b * kRayCounterWords;
    f.counters = ctx->counters.as<unsigned long long>();
    f.ray_steps = count ? ctx->raySteps.as<uint16_t>() : nullptr;
    // (counters.ptr is cleared below when counting: the cover map's counts are its last three
    // words, the seed candidates' count the word before them)
    f.seed_cache = ctx->seeds.as<uint32_t>();
    f.seed_offsets_write = f.seed_cache && f.update_offsets && ctx->scene.root_masked < 0 ? 1u : 0u;
    f.seed_counts = count && f.seed_cache ? ctx->counters.as<uint32_t>() + ctx->counters.bytes / 4u - 4u : nullptr;
    f.cover_counts = count ? ctx->counters.as<uint32_t>() + ctx->counters.bytes / 4u - 3u : nullptr;
    ctx->coverCountsValid = count;
    // shading work set (ensureShadeWork): per-ray light bits | shadow-ray list
    {
        const ShadeWorkLayout l = shadeWorkLayout(ctx);
        char* w = static_cast<char*>(ctx->shadeWork.ptr);
        f.shadow_bits = reinterpret_cast<uint32_t*>(w + l.bits);
        f.shadow_rays = reinterpret_cast<ShadowRay*>(w + l.list);
    }
    f.shadow_count = f.ray_counter + kShadowCountWord;
    f.shadow_heads = f.ray_counter + kShadowHeadWord;
    // the sun's shadow rays in their own list (the first Kmax x Rmax entries of the
    // list area, the other lights' after them) for the light-space BVH
    if (ctx->scene.sun_root >= 0) {
        f.sun_rays = f.shadow_rays;
        f.shadow_rays += Kmax * Rmax;
        f.sun_count = f.ray_counter + kSunCountWord;
        f.sun_heads = f.ray_counter + kSunHeadWord;
    }
    // the slot table and the primary traversal: on traceStream after frame n - 2 (the
    // last user of buffer set b) when pipelined, else in line on the caller's stream
    const hipStream_t ts = pipe ? ctx->traceStream : s;
    uint32_t* seqTrace = ctx->seqWords.as<uint32_t>();
    uint32_t* seqMain = seqTrace + 32;
    uint32_t* seqTimedOut = seqTrace + 64;
    const bool seq = pipe && ctx->seqSync;
    const uint32_t seqN = seq ? ++ctx->frameSeq : 0u;
    if (pipe && ctx->setSeqValid[b]) ARK_HIP(launch_seq_wait(seqMain, ctx->setSeq[b], seqTimedOut, ctx->hostAbortDev, ctx->seqTimeoutTicks, ts));
    else if (pipe && ctx->frameDoneValid[b]) ARK_HIP(hipStreamWaitEvent(ts, ctx->evFrameDone[b], 0));
    // a serial previous frame wrote its offsets on the caller's stream
    if (pipe && !ctx->prevPipelined && ctx->frameDoneValid[b ^ 1u]) ARK_HIP(hipStreamWaitEvent(ts, ctx->evFrameDone[b ^ 1u], 0));
    // a refit or an installed rebuild of the scene enqueued since this context's last
    // update (on any stream, by any context sharing the scene): the traversal reads the
    // BVH it writes
    if (ctx->geometrySeen != ctx->sceneStore->geometrySeq) {
        ARK_HIP(hipStreamWaitEvent(ts, ctx->sceneStore->evGeometry, 0));
        ctx->geometrySeen = ctx->sceneStore->geometrySeq;
    }
    // a new record order of the world BVHs (set_scene, an installed rebuild - this context's
    // above, or a sharing context's): the cached record indices are the old order's. The
    // traversals of a context run one after the other (they share a spill region), so on ts
    // the fill follows the last traversal that wrote old indices and precedes the first
    // that reads the new tree.
    if (f.seed_cache && (ctx->seedStale || ctx->seedTopologySeen != ctx->sceneStore->worldTopologySeq)) {
        ARK_HIP(launch_fill_u32(ctx->seeds.ptr, ctx->seeds.bytes / 4, seed::kNone, ts));
        ctx->seedStale = false;
        ctx->seedTopologySeen = ctx->sceneStore->worldTopologySeq;
    }
    if (count) ARK_HIP(hipMemsetAsync(ctx->counters.ptr, 0, ctx->counters.bytes, s));
    // (k_probe_slots zeroes f.ray_counter)
    if (timing) ARK_HIP(hipEventRecord(ctx->ev[0], s));
    f.slot_order = ctx->slotOrder.as<uint32_t>() + b * Kmax; // written by k_probe_slots
    ARK_HIP(launch_probe_slots(f, ts));
    if (f.window_probes > 0) {
        RoctxRange traceZone("Trace rays");
        const bool half = pipe && f.window_rays < kPipeHalfRays;
        ARK_HIP(launch_trace(ctx->scene, f, half ? ctx->pipeTraceBlocks : ctx->traceBlocks, count, ts));
        if (pipe) {
            // probeUpdateOffset (k_probe_offsets: from the hit records), so that the
            // next frame's slot table may follow on this stream. The rest of the frame
            // needs only the hit records, but waiting for the offsets too costs less
            // (7 us) than a second cross-stream wait for them at the end of the frame
            // (each wait ~11 us of queue latency, satisfied or not: profiles/r03_v)
            ARK_HIP(launch_probe_offsets(f, ts));
            ARK_HIP(tracedSync(ctx, seq, seqN, ts, s));
        }
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[1], s));
        FrameArgs fs = f;
        fs.spill = ctx->spill.as<uint32_t>(); // region 0
        if (count) ctx->coverFrame = fs;
        // the sun alone, with its cover map: shading resolves the sun's rays itself, and
        // only what the map leaves undecided is listed, traced and shaded in a second pass
        // (not beside a half-occupancy traversal: shade_schedule.h)
        const bool sunOnly = shadeScheduleOf({ f.light_count, ctx->scene.has_sun != 0, ctx->scene.sun_map != nullptr, ctx->desc.flags, half,
                                               ctx->sunOnlySmallWindows }) == ShadeSchedule::SunOnly;
        ctx->lastSunOnly = sunOnly;
        ctx->lastDeferredCount = fs.sun_rays ? fs.sun_count : fs.shadow_count;
        if (f.light_count > 0 && !sunOnly) {
            ARK_HIP(launch_shadow_gen(ctx->scene, fs, s));
            // (the grid stays sized by the window although the cover map leaves a few percent of
            // the sun's rays on the list: an eighth of it measured the same, EXPERIMENTS.md)
            ARK_HIP(launch_trace_shadow(ctx->scene, fs, count ? ctx->shadowBlocks : shadowBlocksFor(ctx, f.window_rays), count, s));
        }
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[5], s));
        // shading reads the previous frame's atlases at arbitrary probes: on a Z-slab
        // rank it waits here for the previous exchange (the traversal above did not)
        if (shadeWaitEvent) ARK_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(shadeWaitEvent), 0));
        if (shadeWaitSeq) ARK_HIP(launch_seq_wait(seqTrace + 96, shadeWaitSeq, seqTimedOut, ctx->hostAbortDev, ctx->seqTimeoutTicks, s));
        ARK_HIP(launch_shade(ctx->scene, fs, ctx->shadeBlocks, count, s, sunOnly));
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[2], s));
        if (sunOnly) {
            // (timings: "shade" is pass 1, "shadow" the traversal and the deferred pass)
            ARK_HIP(launch_trace_shadow(ctx->scene, fs, count ? ctx->shadowBlocks : shadowBlocksFor(ctx, f.window_rays), count, s));
            ARK_HIP(launch_shade_deferred(ctx->scene, fs, s));
        }
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[4], s));
        traceZone.end();
        // probeUpdateOffset (serial frames), probeUpdateIrradiance/Visibility + border
        // corners/edges, fused
        RoctxRange updateZone("Update probes");
        if (!pipe) ARK_HIP(launch_probe_offsets(fs, s));
        ARK_HIP(launch_probe_update(fs, s));
    } else {
        ctx->lastSunOnly = false;
        if (pipe) ARK_HIP(tracedSync(ctx, seq, seqN, ts, s));
        if (shadeWaitEvent) ARK_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(shadeWaitEvent), 0));
        if (shadeWaitSeq) ARK_HIP(launch_seq_wait(seqTrace + 96, shadeWaitSeq, seqTimedOut, ctx->hostAbortDev, ctx->seqTimeoutTicks, s));
        if (timing) {
            ARK_HIP(hipEventRecord(ctx->ev[1], s));
            ARK_HIP(hipEventRecord(ctx->ev[5], s));
            ARK_HIP(hipEventRecord(ctx->ev[2], s));
            ARK_HIP(hipEventRecord(ctx->ev[4], s));
        }
    }
    if (timing) ARK_HIP(hipEventRecord(ctx->ev[3], s));
    if (seq) {
        ARK_HIP(launch_seq_signal(seqMain, seqN, s));
        ctx->setSeq[b] = seqN;
        ctx->setSeqValid[b] = true;
    } else {
        ARK_HIP(hipEventRecord(ctx->evFrameDone[b], s));
        ctx->setSeqValid[b] = false;
    }
    ctx->frameDoneValid[b] = true;
    ctx->lastMainSeq = seq ? seqN : 0u;
    ctx->lastStream = s;
    if (doneEvent) ARK_HIP(hipEventRecord(static_cast<hipEvent_t>(doneEvent), s));
    ARK_HIP(orderEnd(ctx, s));
    ctx->parity = b ^ 1u;
    ctx->pipeReady = true;
    ctx->prevR = R;
    ctx->prevPipelined = pipe;
    ctx->lastParity = b;
    ctx->timingValid = timing;
    ctx->countersPending = count;
    ctx->lastRays = f.window_rays;
    ctx->lastProbes = f.window_probes;
    ctx->nextProbeIndex = (f.first + K) % N;
    ctx->lastFirst = f.first;
    ctx->lastK = K;
    return ARK_DDGI_OK;
}

int ark_ddgi_mark_external_write(ArkDdgiCtx* ctx)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->pipeReady = false; // the next update's traversal waits for this
    return ARK_DDGI_OK;
}

int ark_ddgi_synchronize(ArkDdgiCtx* ctx)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return checkSequencing(ctx);
}

static int resourceInfo(const ArkDdgiCtx* ctx, int which, void** ptr, uint64_t* bytes)
{
    switch (which) {
    case ARK_DDGI_ATLAS_IRRADIANCE: *ptr = ctx->irr.ptr; *bytes = ctx->irr.bytes; return 0;
    case ARK_DDGI_ATLAS_VISIBILITY: *ptr = ctx->vis.ptr; *bytes = ctx->vis.bytes; return 0;
    case ARK_DDGI_SURFELS: *ptr = ctx->surfels.ptr; *bytes = ctx->surfels.bytes; return 0;
    case ARK_DDGI_PROBE_OFFSETS: *ptr = ctx->offsets.ptr; *bytes = ctx->offsets.bytes; return 0;
    case ARK_DDGI_DEBUG_HITS: *ptr = ctx->hits.as<GpuHit>() + static_cast<uint64_t>(ctx->lastParity) * ctx->Kmax * ctx->Rmax; *bytes = ctx->hits.bytes / 2; return 0;
    case ARK_DDGI_DEBUG_RAY_STEPS: *ptr = ctx->raySteps.ptr; *bytes = ctx->raySteps.bytes; return ctx->raySteps.ptr ? 0 : ARK_DDGI_E_INVALID_ARGUMENT;
    default: return ARK_DDGI_E_INVALID_ARGUMENT;
    }
}

int ark_ddgi_resource_size(const ArkDdgiCtx* ctx, int which, uint64_t* outBytes)
{
    if (!ctx || !outBytes) return ARK_DDGI_E_INVALID_ARGUMENT;
    void* p;
    return resourceInfo(ctx, which, &p, outBytes);
}

int ark_ddgi_read(ArkDdgiCtx* ctx, int which, void* dst, uint64_t bytes)
{
    if (!ctx || !dst) return ARK_DDGI_E_INVALID_ARGUMENT;
    void* p;
    uint64_t n;
    if (resourceInfo(ctx, which, &p, &n) != 0) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "unknown resource %d", which);
    if (bytes != n) return ctx->fail(ARK_DDGI_E_SIZE_MISMATCH, "resource %d is %llu bytes, got %llu", which, (unsigned long long)n, (unsigned long long)bytes);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(dst, p, n, hipMemcpyDeviceToHost));
    return ARK_DDGI_OK;
}

int ark_ddgi_write(ArkDdgiCtx* ctx, int which, const void* src, uint64_t bytes)
{
    if (!ctx || !src) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->pipeReady = false; // the next update's traversal waits for this
    void* p;
    uint64_t n;
    if (resourceInfo(ctx, which, &p, &n) != 0) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "unknown resource %d", which);
    if (bytes != n) return ctx->fail(ARK_DDGI_E_SIZE_MISMATCH, "resource %d is %llu bytes, got %llu", which, (unsigned long long)n, (unsigned long long)bytes);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    return ARK_DDGI_OK;
}

// --- history checkpoint ------------------------------------------------------
namespace {
struct StateHeader {
    char magic[8];           // "ARKDDGI1"
    int32_t grid[3];
    float spacing[3], origin[3];
    float zFar;
    int32_t clearMode, shardRank, shardCount;
    uint32_t nextProbeIndex; // the rolling window's next first probe (m_probeUpdateIdx, DDGINode.h:32)
    uint64_t irrBytes, visBytes, offBytes;
};
static_assert(sizeof(StateHeader) == 88, "state header layout");

StateHeader stateHeaderOf(const ArkDdgiCtx* ctx)
{
    StateHeader h {};
    std::memcpy(h.magic, "ARKDDGI1", 8);
    h.grid[0] = ctx->X;
    h.grid[1] = ctx->Y;
    h.grid[2] = ctx->Z;
    for (int k = 0; k < 3; ++k) {
        h.spacing[k] = ctx->desc.probe_spacing[k];
        h.origin[k] = ctx->desc.offset_to_first[k];
    }
    h.zFar = ctx->desc.z_far;
    h.clearMode = ctx->desc.clear_overflow_mode;
    h.shardRank = ctx->desc.shard_rank;
    h.shardCount = ctx->desc.shard_count;
    h.nextProbeIndex = ctx->nextProbeIndex;
    h.irrBytes = ctx->irr.bytes;
    h.visBytes = ctx->vis.bytes;
    h.offBytes = ctx->offsets.bytes;
    return h;
}
} // namespace

int ark_ddgi_state_size(const ArkDdgiCtx* ctx, uint64_t* outBytes)
{
    if (!ctx || !outBytes) return ARK_DDGI_E_INVALID_ARGUMENT;
    *outBytes = sizeof(StateHeader) + ctx->irr.bytes + ctx->vis.bytes + ctx->offsets.bytes;
    return ARK_DDGI_OK;
}

int ark_ddgi_save_state(ArkDdgiCtx* ctx, void* dst, uint64_t bytes)
{
    if (!ctx || !dst) return ARK_DDGI_E_INVALID_ARGUMENT;
    uint64_t need = 0;
    ark_ddgi_state_size(ctx, &need);
    if (bytes != need) return ctx->fail(ARK_DDGI_E_SIZE_MISMATCH, "state is %llu bytes, got %llu", (unsigned long long)need, (unsigned long long)bytes);
    const StateHeader h = stateHeaderOf(ctx);
    char* o = static_cast<char*>(dst);
    std::memcpy(o, &h, sizeof(h));
    o += sizeof(h);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(o, ctx->irr.ptr, ctx->irr.bytes, hipMemcpyDeviceToHost));
    o += ctx->irr.bytes;
    ARK_HIP(hipMemcpy(o, ctx->vis.ptr, ctx->vis.bytes, hipMemcpyDeviceToHost));
    o += ctx->vis.bytes;
    ARK_HIP(hipMemcpy(o, ctx->offsets.ptr, ctx->offsets.bytes, hipMemcpyDeviceToHost));
    return ARK_DDGI_OK;
}

int ark_ddgi_load_state(ArkDdgiCtx* ctx, const void* src, uint64_t bytes)
{
    if (!ctx || !src) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->pipeReady = false; // the next update's traversal waits for this
    uint64_t need = 0;
    ark_ddgi_state_size(ctx, &need);
    if (bytes != need) return ctx->fail(ARK_DDGI_E_SIZE_MISMATCH, "state is %llu bytes, got %llu", (unsigned long long)need, (unsigned long long)bytes);
    StateHeader h;
    std::memcpy(&h, src, sizeof(h));
    StateHeader mine = stateHeaderOf(ctx);
    mine.nextProbeIndex = h.nextProbeIndex; // the window position is state, not geometry
    if (std::memcmp(&h, &mine, sizeof(h)) != 0 || h.nextProbeIndex >= static_cast<uint32_t>(ctx->N))
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "state blob is of another grid / zFar / clear mode / shard (or not a DDGI state)");
    const char* i = static_cast<const char*>(src) + sizeof(h);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(ctx->irr.ptr, i, ctx->irr.bytes, hipMemcpyHostToDevice));
    i += ctx->irr.bytes;
    ARK_HIP(hipMemcpy(ctx->vis.ptr, i, ctx->vis.bytes, hipMemcpyHostToDevice));
    i += ctx->vis.bytes;
    ARK_HIP(hipMemcpy(ctx->offsets.ptr, i, ctx->offsets.bytes, hipMemcpyHostToDevice));
    ctx->nextProbeIndex = h.nextProbeIndex;
    return ARK_DDGI_OK;
}

int ark_ddgi_get_next_probe_index(const ArkDdgiCtx* ctx, uint32_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    *out = ctx->nextProbeIndex;
    return ARK_DDGI_OK;
}

int ark_ddgi_get_device_views(ArkDdgiCtx* ctx, ArkDdgiDeviceViews* v)
{
    if (!ctx || !v) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::memset(v, 0, sizeof(*v));
    v->irradiance_atlas = ctx->irr.ptr;
    v->irradiance_bytes = ctx->irr.bytes;
    v->irradiance_width = ctx->Wi;
    v->irradiance_height = ctx->Hi;
    v->visibility_atlas = ctx->vis.ptr;
    v->visibility_bytes = ctx->vis.bytes;
    v->visibility_width = ctx->Wv;
    v->visibility_height = ctx->Hv;
    v->probe_offsets = ctx->offsets.ptr;
    v->probe_offsets_bytes = ctx->offsets.bytes;
    // Z-slab = contiguous texel-row band of both atlases (tile row = z, ddgi/common.glsl:58-61)
    const uint64_t rowI = static_cast<uint64_t>(ctx->Wi) * 8, rowV = static_cast<uint64_t>(ctx->Wv) * 4;
    const int si = ARK_DDGI_IRRADIANCE_RES + 2, sv = ARK_DDGI_VISIBILITY_RES + 2;
    v->irradiance_slab_offset = static_cast<uint64_t>(ctx->slabZ0) * si * rowI;
    v->irradiance_slab_bytes = static_cast<uint64_t>(ctx->slabZ1 - ctx->slabZ0) * si * rowI;
    v->visibility_slab_offset = static_cast<uint64_t>(ctx->slabZ0) * sv * rowV;
    v->visibility_slab_bytes = static_cast<uint64_t>(ctx->slabZ1 - ctx->slabZ0) * sv * rowV;
    return ARK_DDGI_OK;
}

int ark_ddgi_reset_history(ArkDdgiCtx* ctx)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->pipeReady = false; // the next update's traversal waits for this
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return clearHistory(ctx);
}

int ark_ddgi_set_counting(ArkDdgiCtx* ctx, int enabled)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->counting = enabled != 0;
    if (ctx->counting && !ctx->raySteps.ptr) {
        ARK_HIP(hipSetDevice(ctx->device));
        ARK_HIP(ctx->raySteps.alloc(static_cast<size_t>(ctx->Kmax) * ctx->Rmax * 2));
        ARK_HIP(hipMemset(ctx->raySteps.ptr, 0, ctx->raySteps.bytes));
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_get_counters(ArkDdgiCtx* ctx, ArkDdgiCounters* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    out->rays = ctx->lastRays;
    out->probes = ctx->lastProbes;
    if (ctx->countersPending) {
        unsigned long long c[8];
        ARK_HIP(hipSetDevice(ctx->device));
        ARK_HIP(hipDeviceSynchronize());
        ARK_HIP(hipMemcpy(c, ctx->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
        out->primary_node_visits = c[0];
        out->primary_tri_tests = c[1];
        out->hits = c[2];
        out->shadow_rays = c[3];
        out->shadow_node_visits = c[4];
        out->shadow_tri_tests = c[5];
        out->front_hits = c[6];
        out->primary_wave_steps = c[7];
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_set_timing(ArkDdgiCtx* ctx, int enabled)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->timing = enabled != 0;
    return ARK_DDGI_OK;
}

int ark_ddgi_get_last_timings(ArkDdgiCtx* ctx, float* out, int count)
{
    if (!ctx || !out || count <= 0) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->timingValid) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "timing not enabled for the last update");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipEventSynchronize(ctx->ev[3]));
    float ms[5] = {};
    ARK_HIP(hipEventElapsedTime(&ms[0], ctx->ev[0], ctx->ev[3]));
    ARK_HIP(hipEventElapsedTime(&ms[1], ctx->ev[0], ctx->ev[1]));
    // shade = ev5 -> ev2; shadow = (ev1 -> ev5) + (ev2 -> ev4): whichever side of
    // shading the schedule put the shadow rays on (the other interval is ~0)
    float pre = 0.0f, post = 0.0f;
    ARK_HIP(hipEventElapsedTime(&ms[2], ctx->ev[5], ctx->ev[2]));
    ARK_HIP(hipEventElapsedTime(&ms[3], ctx->ev[4], ctx->ev[3]));
    ARK_HIP(hipEventElapsedTime(&pre, ctx->ev[1], ctx->ev[5]));
    ARK_HIP(hipEventElapsedTime(&post, ctx->ev[2], ctx->ev[4]));
    ms[4] = pre + post;
    for (int i = 0; i < count && i < 5; ++i) out[i] = ms[i];
    return ARK_DDGI_OK;
}

int ark_ddgi_get_bvh_stats(ArkDdgiCtx* ctx, ArkDdgiBvhStats* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    *out = ctx->hasScene ? ctx->sceneStore->bvhStats : ctx->bvhStats; // the store's: installs and refits of any sharing context
    return ARK_DDGI_OK;
}

// AO / bent-normal bake (include/ark_ddgi.h; BakeAmbientOcclusionNode.cpp:15-131):
// raster -> barycentrics (+ covered-texel list) -> persistent AO rays, one stream.
int ark_ddgi_bake_ao(ArkDdgiCtx* ctx, const ArkBakeAoDesc* d, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!d || d->struct_size != sizeof(ArkBakeAoDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkBakeAoDesc");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake: no scene");
    if (d->instance_index >= ctx->sceneStore->instHost.size()) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake: instance %u out of range", d->instance_index);
    if (d->width == 0 || d->height == 0 || d->width > 16384 || d->height > 16384 || d->sample_count == 0)
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake: extent %ux%u / %u samples", d->width, d->height, d->sample_count);
    const ArkRTInstance& inst = ctx->sceneStore->instHost[d->instance_index];
    const ArkRTTriangleMesh& mesh = ctx->sceneStore->meshHost[inst.rt_mesh_index];
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (ctx->sceneVersion != ctx->sceneStore->version) // a sharing context refitted the scene or installed a deeper sun BVH
        if (const int rc = refreshScene(ctx)) return rc;
    ARK_HIP(orderBegin(ctx, s));
    const size_t texels = static_cast<size_t>(d->width) * d->height;
    const size_t outBytes = texels * (d->bent_normals ? 4 : 1);
    if (ctx->bakeTri.bytes < texels * 4) ARK_HIP(ctx->bakeTri.alloc(texels * 4));
    if (ctx->bakeBary.bytes < texels * 8) ARK_HIP(ctx->bakeBary.alloc(texels * 8));
    if (ctx->bakeOut.bytes < outBytes) ARK_HIP(ctx->bakeOut.alloc(outBytes));
    if (ctx->bakePixels.bytes < texels * 4) ARK_HIP(ctx->bakePixels.alloc(texels * 4));
    if (ctx->bakeCounters.bytes < 256) ARK_HIP(ctx->bakeCounters.alloc(256));
    ARK_HIP(hipMemsetAsync(ctx->bakeTri.ptr, 0, texels * 4, s)); // ClearValue::blackAtMaxDepth
    ARK_HIP(hipMemsetAsync(ctx->bakeCounters.ptr, 0, 256, s));
    BakeArgs b {};
    b.W = d->width;
    b.H = d->height;
    b.samples = d->sample_count;
    b.tri_count = inst.triangle_count;
    b.bent = d->bent_normals ? 1 : 0;
    b.first_index = static_cast<uint32_t>(mesh.first_index);
    b.first_vertex = static_cast<uint32_t>(mesh.first_vertex);
    b.indices = ctx->sceneStore->indices.as<uint32_t>();
    b.positions = ctx->sceneStore->positions.as<float>();
    b.vertices = ctx->sceneStore->vertices.as<float>();
    b.tri_idx = ctx->bakeTri.as<uint32_t>();
    b.bary = ctx->bakeBary.as<uint16_t>();
    b.out = ctx->bakeOut.as<uint8_t>();
    b.pixels = ctx->bakePixels.as<uint32_t>();
    b.counters = ctx->bakeCounters.as<uint32_t>();
    b.spill = ctx->spill.as<uint32_t>();
    if (b.tri_count > 0) ARK_HIP(launch_bake(ctx->scene, b, 0, 0, s));
    ARK_HIP(launch_bake(ctx->scene, b, 0, 1, s));
    // the persistent AO kernel uses the traversal spill area sized for shadowBlocks workgroups
    ARK_HIP(launch_bake(ctx->scene, b, ctx->shadowBlocks, 2, s));
    ARK_HIP(scenePositionsRead(*ctx->sceneStore, s)); // (the next vertex update's positions follow the bake)
    ARK_HIP(orderEnd(ctx, s));
    ctx->bakeW = d->width;
    ctx->bakeH = d->height;
    ctx->bakeBent = b.bent;
    return ARK_DDGI_OK;
}

int ark_ddgi_bake_read(ArkDdgiCtx* ctx, int which, void* dst, uint64_t bytes)
{
    if (!ctx || !dst) return ARK_DDGI_E_INVALID_ARGUMENT;
    const size_t texels = static_cast<size_t>(ctx->bakeW) * ctx->bakeH;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
    case ARK_BAKE_TRIANGLE_INDEX: src = ctx->bakeTri.ptr; n = texels * 4; break;
    case ARK_BAKE_BARYCENTRICS: src = ctx->bakeBary.ptr; n = texels * 8; break;
    case ARK_BAKE_OUTPUT: src = ctx->bakeOut.ptr; n = texels * (ctx->bakeBent ? 4 : 1); break;
    default: return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake_read: unknown resource %d", which);
    }
    if (texels == 0) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake_read: no bake yet");
    if (bytes != n) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake_read: %llu bytes, resource has %zu", static_cast<unsigned long long>(bytes), n);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return ARK_DDGI_OK;
}

int ark_ddgi_lighting_compose(ArkDdgiCtx* ctx, const ArkComposeDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkComposeDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkComposeDesc");
    if (!desc->out) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "lighting_compose: no output plane");
    if (static_cast<uint64_t>(desc->width) * desc->height >= (1ull << 32)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "lighting_compose: target too large");
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    // the DDGISamplingSet (DDGINode.cpp:45-66): grid constants + both atlases
    FrameArgs f {};
    f.X = ctx->X; f.Y = ctx->Y; f.Z = ctx->Z;
    f.Wi = ctx->Wi; f.Hi = ctx->Hi; f.Wv = ctx->Wv; f.Hv = ctx->Hv;
    for (int k = 0; k < 3; ++k) {
        f.spacing[k] = ctx->desc.probe_spacing[k];
        f.origin[k] = ctx->desc.offset_to_first[k];
    }
    f.irr = ctx->irr.as<uint16_t>();
    f.vis = ctx->vis.as<uint16_t>();
    ArkComposeDesc c = *desc;
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(launch_lighting_compose(f, c, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

int ark_ddgi_rt_reflections(ArkDdgiCtx* ctx, const ArkReflectionsDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkReflectionsDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkReflectionsDesc");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "rt_reflections before ark_ddgi_set_scene");
    if (!desc->out_radiance || !desc->out_direction) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections: no output image");
    if (desc->blue_noise && (desc->noise_width == 0 || desc->noise_height == 0)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections: empty blue noise");
    if (static_cast<uint64_t>(desc->width) * desc->height >= (1ull << 32)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections: target too large");
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    int rc;
    // the scene first: a sharing context's deeper sun BVH may grow,
    // i.e. reallocate, the spill area that f.spill points into below
    if (ctx->sceneVersion != ctx->sceneStore->version) {
        if ((rc = refreshScene(ctx)) != 0) return rc;
    } else if ((rc = ensureSpill(ctx)) != 0) {
        return rc;
    }
    FrameArgs f {};
    f.X = ctx->X; f.Y = ctx->Y; f.Z = ctx->Z;
    f.Wi = ctx->Wi; f.Hi = ctx->Hi; f.Wv = ctx->Wv; f.Hv = ctx->Hv;
    for (int k = 0; k < 3; ++k) {
        f.spacing[k] = ctx->desc.probe_spacing[k];
        f.origin[k] = ctx->desc.offset_to_first[k];
    }
    f.irr = ctx->irr.as<uint16_t>();
    f.vis = ctx->vis.as<uint16_t>();
    f.z_far = ctx->desc.z_far;
    f.ambient_amount = desc->ambient_amount;
    f.environment_multiplier = desc->environment_multiplier;
    f.spill = ctx->spill.as<uint32_t>();
    // ray-list work set (ensureReflWork): rays, hit records, light bits, shadow rays, counters
    const uint64_t pixels = static_cast<uint64_t>(desc->width) * desc->height;
    if (pixels == 0) return ARK_DDGI_OK;
    if ((rc = ensureReflWork(ctx, pixels)) != 0) return rc;
    {
        char* w = static_cast<char*>(ctx->reflWork.ptr);
        auto take = [&](uint64_t bytes) {
            char* q = w;
            w += (bytes + 255) & ~static_cast<uint64_t>(255);
            return q;
        };
        f.ray_list = reinterpret_cast<const float4*>(take(pixels * 32));
        f.hits = reinterpret_cast<GpuHit*>(take(pixels * sizeof(GpuHit)));
        f.shadow_bits = reinterpret_cast<uint32_t*>(take(pixels * 4));
        f.ray_counter = reinterpret_cast<uint32_t*>(take((kRayCounterWords + kRayCounterStride) * 4));
        f.shadow_rays = reinterpret_cast<ShadowRay*>(take(pixels * ctx->lightCount * sizeof(ShadowRay)));
    }
    f.shadow_count = f.ray_counter + kShadowCountWord;
    f.shadow_heads = f.ray_counter + kShadowHeadWord;
    f.list_count = f.ray_counter + kRayCounterWords;
    f.light_count = ctx->lightCount;
    f.refill_min = ctx->refillMin;
    f.sun_refill_min = ctx->sunRefillMin;
    f.grab_chunk = ctx->grabChunk;
    f.counters = ctx->counters.as<unsigned long long>();
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(flushLights(ctx, s));
    ARK_HIP(hipMemsetAsync(f.ray_counter, 0, (kRayCounterWords + kRayCounterStride) * 4, s));
    ARK_HIP(launch_rt_reflections(ctx->scene, f, *desc, ctx->traceBlocks, shadowBlocksFor(ctx, pixels), s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

int ark_ddgi_probe_debug(ArkDdgiCtx* ctx, const ArkProbeDebugDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkProbeDebugDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkProbeDebugDesc");
    if (desc->count && (!desc->probe_indices || !desc->directions || !desc->out)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "probe_debug: null plane");
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    FrameArgs f {};
    f.X = ctx->X; f.Y = ctx->Y; f.Z = ctx->Z;
    f.Wi = ctx->Wi; f.Hi = ctx->Hi; f.Wv = ctx->Wv; f.Hv = ctx->Hv;
    for (int k = 0; k < 3; ++k) {
        f.spacing[k] = ctx->desc.probe_spacing[k];
        f.origin[k] = ctx->desc.offset_to_first[k];
    }
    f.irr = ctx->irr.as<uint16_t>();
    f.vis = ctx->vis.as<uint16_t>();
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(launch_probe_debug(f, *desc, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

} // extern "C"
