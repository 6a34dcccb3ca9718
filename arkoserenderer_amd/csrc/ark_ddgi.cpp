// ark_ddgi.cpp — the C-ABI context of the MI355X DDGI path (include/ark_ddgi.h,
// ddgi_context.h): its lifetime, scene, lights and resources. The update itself is in
// ddgi_frame.cpp, the other passes in ddgi_passes.cpp.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ddgi_context.h"
#include "sun_cover_map.h"

namespace {

uint16_t f32_to_f16_host(float f)
{
    // host-side RNE conversion for the clear values (matches v_cvt_f16_f32)
    _Float16 h = static_cast<_Float16>(f);
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

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

} // namespace

int ark::ensureSpill(ArkDdgiCtx* ctx)
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
    return ARK_DDGI_OK;
}

static_assert(ARK_DDGI_MAX_SPOT_LIGHTS == kMaxLights - 1, "spot light capacity");

// deriveSceneArgs plus a traversal spill area deep enough for every BVH the derived
// args reach. Every caller goes through here: a sharing context may
// have installed a deeper sun BVH, and marking the store's version as seen without
// growing the spill area would let the next traversal overrun it.
int ark::refreshScene(ArkDdgiCtx* ctx)
{
    deriveSceneArgs(ctx);
    return ensureSpill(ctx);
}

// The context's spot lights reach the device in stream order on `s`, ahead of the
// operation that reads them (a by-value kernel argument: no host buffer to keep alive).
hipError_t ark::flushLights(ArkDdgiCtx* ctx, hipStream_t s)
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
hipError_t ark::drainContext(ArkDdgiCtx* ctx)
{
    hipError_t e = hipStreamSynchronize(ctx->traceStream);
    if (e == hipSuccess && ctx->orderValid) e = hipEventSynchronize(ctx->evOrder);
    return e;
}

// What the scene's calls (scene_store.h) take from the calling context
SceneCall ark::sceneCall(ArkDdgiCtx* ctx)
{
    SceneCall c {};
    c.err = ctx;
    c.flags = ctx->desc.flags;
    c.hasSun = ctx->hasSun != 0;
    std::copy(ctx->sunDir, ctx->sunDir + 3, c.sunDir);
    c.shared = ctx->sceneStore.use_count() > 1;
    return c;
}

namespace {

// The shading work set (shadeWorkLayout) holds the largest window with `lightCount` lights
int ensureShadeWork(ArkDdgiCtx* ctx, uint32_t lightCount)
{
    const uint64_t rays = static_cast<uint64_t>(ctx->Kmax) * ctx->Rmax;
    if (rays >= (1ull << 28) && lightCount > 0)
        return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "%llu rays per update: shadow-ray owners pack (ray << 4) | light in 32 bits", static_cast<unsigned long long>(rays));
    const ShadeWorkLayout w = shadeWorkLayout(ctx, lightCount);
    if (ctx->shadeWork.bytes < w.total) ARK_HIP(ctx->shadeWork.alloc(w.total));
    return ARK_DDGI_OK;
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
    if ((rc = ensureShadeWork(ctx, ctx->lightCount)) != 0) return rc;
    if ((rc = ensureSpill(ctx)) != 0) return rc;
    ctx->hasScene = true;
    return ARK_DDGI_OK;
}

// A refit entry (set_instances, update_geometry, skin_geometry): `refit` is the store's call
// on `s` - the refit of the next geometry copy on the store's stream, which `s` then
// follows; finished background rebuilds installed and new ones started on `s`
template<class Refit>
int refitEntry(ArkDdgiCtx* ctx, const char* before, void* hipStream, Refit refit)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "%s before ark_ddgi_set_scene", before);
    SceneStore& st = *ctx->sceneStore;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(orderBegin(ctx, s));
    if (const int rc = refit(st, sceneCall(ctx), s)) return rc;
    if (ctx->sceneVersion != st.version)
        if (const int rc = refreshScene(ctx)) return rc;
    ARK_HIP(orderEnd(ctx, s));
    st.bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ARK_DDGI_OK;
}

// The blocking form of a refit entry: on the context's internal stream, then waited for
template<class Async>
int refitBlocking(ArkDdgiCtx* ctx, Async async)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = async(ctx->stream)) return rc;
    ARK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->sceneStore->bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->bvhStats = ctx->sceneStore->bvhStats;
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
    ctx->frames.pipelining = (desc->flags & ARK_DDGI_FLAG_SERIAL_FRAMES) == 0;
    ctx->sunBvh = desc->sun_bvh == ARK_DDGI_SUN_BVH_WORLD ? 0 : desc->sun_bvh == ARK_DDGI_SUN_BVH_LIGHT_SPACE ? 1 : -1;
    // a counter-collecting profiler (rocprofv3 --pmc) runs one kernel at a time across
    // queues: a polling wait could then hold the GPU while the kernel it waits for queues
    // behind it: it would give up after its bound and fail closed (checkSequencing),
    // dropping frames; such a context starts with events instead (the profiler's own
    // environment, not a tuning knob; ark_ddgi_set_sequencing overrides it)
    if (const char* pc = std::getenv("ROCPROF_COUNTER_COLLECTION"))
        if (*pc && std::strcmp(pc, "0") != 0 && std::strcmp(pc, "false") != 0) ctx->frames.setSequencing(false);
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
    for (DeviceBuffer* b : { &ctx->irr, &ctx->vis, &ctx->offsets, &ctx->slots, &ctx->slotOrder, &ctx->fib, &ctx->fibOrder, &ctx->order, &ctx->hits, &ctx->surfels, &ctx->spill, &ctx->rayCounter, &ctx->seqWords, &ctx->shadeWork, &ctx->reflWork, &ctx->rtShadowWork, &ctx->ptWork,
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
    ctx->frames.externalWrite();
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
    ctx->frames.externalWrite();
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
        if (ctx->shadeWork.bytes < shadeWorkLayout(ctx, count).total) {
            ARK_HIP(drainContext(ctx));
            if (const int rc = ensureShadeWork(ctx, count)) return rc;
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

int ark_ddgi_set_instances_async(ArkDdgiCtx* ctx, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    return refitEntry(ctx, "ark_ddgi_set_instances", hipStream,
                      [&](SceneStore& st, const SceneCall& c, hipStream_t s) { return sceneSetInstances(st, c, instances, count, s); });
}

int ark_ddgi_set_instances(ArkDdgiCtx* ctx, const ArkRTInstance* instances, uint32_t count)
{
    return refitBlocking(ctx, [&](void* s) { return ark_ddgi_set_instances_async(ctx, instances, count, s); });
}

// set_instances' refit with the vertex ranges written first (scene_store.h)
int ark_ddgi_update_geometry_async(ArkDdgiCtx* ctx, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    return refitEntry(ctx, "ark_ddgi_update_geometry", hipStream, [&](SceneStore& st, const SceneCall& c, hipStream_t s) {
        return sceneUpdateGeometry(st, c, updates, updateCount, instances, count, s);
    });
}

int ark_ddgi_update_geometry(ArkDdgiCtx* ctx, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count)
{
    return refitBlocking(ctx, [&](void* s) { return ark_ddgi_update_geometry_async(ctx, updates, updateCount, instances, count, s); });
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

// the skins' runs on `s`, then update_geometry's refit with their outputs as device sources
int ark_ddgi_skin_geometry_async(ArkDdgiCtx* ctx, const ArkDdgiSkinPose* poses, uint32_t poseCount, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    return refitEntry(ctx, "ark_ddgi_skin_geometry", hipStream, [&](SceneStore& st, const SceneCall& c, hipStream_t s) {
        return sceneSkinGeometry(st, c, poses, poseCount, instances, count, s);
    });
}

int ark_ddgi_skin_geometry(ArkDdgiCtx* ctx, const ArkDdgiSkinPose* poses, uint32_t poseCount, const ArkRTInstance* instances, uint32_t count)
{
    return refitBlocking(ctx, [&](void* s) { return ark_ddgi_skin_geometry_async(ctx, poses, poseCount, instances, count, s); });
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

static int resourceInfo(const ArkDdgiCtx* ctx, int which, void** ptr, uint64_t* bytes)
{
    switch (which) {
    case ARK_DDGI_ATLAS_IRRADIANCE: *ptr = ctx->irr.ptr; *bytes = ctx->irr.bytes; return 0;
    case ARK_DDGI_ATLAS_VISIBILITY: *ptr = ctx->vis.ptr; *bytes = ctx->vis.bytes; return 0;
    case ARK_DDGI_SURFELS: *ptr = ctx->surfels.ptr; *bytes = ctx->surfels.bytes; return 0;
    case ARK_DDGI_PROBE_OFFSETS: *ptr = ctx->offsets.ptr; *bytes = ctx->offsets.bytes; return 0;
    case ARK_DDGI_DEBUG_HITS: *ptr = ctx->hits.as<GpuHit>() + static_cast<uint64_t>(ctx->frames.lastSet()) * ctx->Kmax * ctx->Rmax; *bytes = ctx->hits.bytes / 2; return 0;
    case ARK_DDGI_DEBUG_SHADOW_BITS: // the head of the shading work set (shadeWorkLayout)
        *ptr = ctx->shadeWork.ptr; *bytes = static_cast<uint64_t>(ctx->Kmax) * ctx->Rmax * 4u; return ctx->shadeWork.ptr ? 0 : ARK_DDGI_E_INVALID_ARGUMENT;
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
    ctx->frames.externalWrite();
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
    ctx->frames.externalWrite();
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
    ctx->frames.externalWrite();
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

} // extern "C"
