// ddgi_frame.cpp — a context's update (include/ark_ddgi.h: ark_ddgi_update and its forms):
// the frame's kernel arguments, its traversal-stream part and its caller-stream part,
// enqueued as the book of the frames in flight (frame_book.h) plans them; the sequencing of
// the two streams by device words or events, failing closed (checkSequencing); the Z-slab
// exchanges and the window packets between them.
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cmath>
#include <cstdio>
#include <string>

#include "ddgi_context.h"
#include "shade_schedule.h"

namespace {

// roctx range over a scope (host-side enqueue markers, named after the reference's
// ScopedDebugZone labels, DDGINode.cpp:152-247); begin() opens one left closed, end() closes it early.
class RoctxRange {
public:
    RoctxRange() = default;
    explicit RoctxRange(const char* name) { begin(name); }
    ~RoctxRange() { end(); }
    void begin(const char* name) { roctxRangePushA(name); m_open = true; }
    void end()
    {
        if (m_open) roctxRangePop();
        m_open = false;
    }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;

private:
    bool m_open { false };
};

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

uint32_t countSlabProbes(const ArkDdgiCtx* ctx, uint32_t first, uint32_t K)
{
    if (ctx->desc.shard_count <= 1) return K;
    return slabRankOf(static_cast<uint32_t>(ctx->X), static_cast<uint32_t>(ctx->Y), static_cast<uint32_t>(ctx->Z), static_cast<uint32_t>(ctx->slabZ0),
                      static_cast<uint32_t>(ctx->slabZ1), first, K);
}

// The context's sequence words (ctx->seqWords): a wait on `s` for word >= value, failing closed
enum SeqWord : uint32_t { kSeqTrace = 0, kSeqMain = 32, kSeqTimedOut = 64, kSeqExchange = 96 };

hipError_t seqWait(ArkDdgiCtx* ctx, SeqWord word, uint32_t value, hipStream_t s)
{
    uint32_t* w = ctx->seqWords.as<uint32_t>();
    return launch_seq_wait(w + word, value, w + kSeqTimedOut, ctx->hostAbortDev, ctx->seqTimeoutTicks, s);
}

// The caller's stream s waits for the traversal stream's part of a pipelined frame
// (slot table, traversal, offsets): device-side sequencing, or an event.
hipError_t tracedSync(ArkDdgiCtx* ctx, const FramePlan& plan, hipStream_t ts, hipStream_t s)
{
    if (plan.seq) {
        hipError_t e = launch_seq_signal(ctx->seqWords.as<uint32_t>() + kSeqTrace, plan.seqN, ts);
        return e != hipSuccess ? e : seqWait(ctx, kSeqTrace, plan.seqN, s);
    }
    hipError_t e = hipEventRecord(ctx->evTraced, ts);
    return e != hipSuccess ? e : hipStreamWaitEvent(s, ctx->evTraced, 0);
}

// a pipelined window below kPipeHalfRays rays: its traversal runs the half-occupancy grid
bool halfWindow(const FramePlan& plan, const FrameArgs& f) { return plan.pipe && f.window_rays < kPipeHalfRays; }

// The kernel arguments of the plan's frame: window [first, first + K) of R rays per probe,
// in buffer set plan.b (the scene is up to date: refreshScene)
FrameArgs frameArgs(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, uint32_t K, uint32_t R, const FramePlan& plan)
{
    const bool count = ctx->counting;
    const uint64_t b = plan.b, Kmax = static_cast<uint64_t>(ctx->Kmax), Rmax = static_cast<uint64_t>(ctx->Rmax);
    FrameArgs f = samplingSetArgs(ctx);
    f.abort_word = ctx->seqWords.as<uint32_t>() + kSeqTimedOut;
    f.z_far = ctx->desc.z_far;
    f.frame = p->frame_index;
    f.first = p->first_probe_index % static_cast<uint32_t>(ctx->N);
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
    f.offsets = ctx->offsets.as<float4>();
    f.slots = ctx->slots.as<GpuProbeSlot>() + b * Kmax;
    f.slot_order = ctx->slotOrder.as<uint32_t>() + b * Kmax; // written by k_probe_slots
    f.fib = ctx->fib.as<float4>() + b * Rmax;
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
    f.grab_chunk = halfWindow(plan, f) ? std::min<uint32_t>(ctx->grabChunk, 32u) : ctx->grabChunk;
    f.ray_counter = ctx->rayCounter.as<uint32_t>() + b * kRayCounterWords; // (k_probe_slots zeroes it)
    f.counters = ctx->counters.as<unsigned long long>();
    f.ray_steps = count ? ctx->raySteps.as<uint16_t>() : nullptr;
    // (counters.ptr is cleared when counting: the cover map's counts are its last three
    // words, the seed candidates' count the word before them)
    f.seed_cache = ctx->seeds.as<uint32_t>();
    f.seed_offsets_write = f.seed_cache && f.update_offsets && ctx->scene.root_masked < 0 ? 1u : 0u;
    f.seed_counts = count && f.seed_cache ? ctx->counters.as<uint32_t>() + ctx->counters.bytes / 4u - 4u : nullptr;
    f.cover_counts = count ? ctx->counters.as<uint32_t>() + ctx->counters.bytes / 4u - 3u : nullptr;
    // shading work set (ensureShadeWork): per-ray light bits | shadow-ray list
    const ShadeWorkLayout l = shadeWorkLayout(ctx, ctx->lightCount);
    char* w = static_cast<char*>(ctx->shadeWork.ptr);
    f.shadow_bits = reinterpret_cast<uint32_t*>(w + l.bits);
    f.shadow_rays = reinterpret_cast<ShadowRay*>(w + l.list);
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
    return f;
}

// The traversal part of the frame - slot table, primary traversal, and the probe offsets
// when pipelined - on the traversal stream once the plan's waits are met, else in line on
// the caller's stream s; s then waits for it (tracedSync).
// Frames in flight: the part reads the scene, the sample order and the probe offsets only,
// which nothing of the previous frame's shadow rays, shading or atlas update writes (its
// offsets ran before them), so it may start before the previous frame is done.
int traversalPart(ArkDdgiCtx* ctx, const FramePlan& plan, const FrameArgs& f, hipStream_t s, RoctxRange& traceZone)
{
    const hipStream_t ts = plan.pipe ? ctx->traceStream : s;
    // after frame n - 2, the last user of buffer set b
    if (plan.reuse == FramePlan::Word) ARK_HIP(seqWait(ctx, kSeqMain, plan.reuseSeq, ts));
    else if (plan.reuse == FramePlan::Event) ARK_HIP(hipStreamWaitEvent(ts, ctx->evFrameDone[plan.b], 0));
    // a serial previous frame wrote its offsets on the caller's stream
    if (plan.waitOtherDone) ARK_HIP(hipStreamWaitEvent(ts, ctx->evFrameDone[plan.b ^ 1u], 0));
    // a refit or an installed rebuild of the scene enqueued since this context's last
    // update (on any stream, by any context sharing the scene): the traversal reads the
    // BVH it writes
    if (ctx->geometrySeen != ctx->sceneStore->geometrySeq) {
        ARK_HIP(hipStreamWaitEvent(ts, ctx->sceneStore->evGeometry, 0));
        ctx->geometrySeen = ctx->sceneStore->geometrySeq;
    }
    // a new record order of the world BVHs (set_scene, an installed rebuild - this context's
    // in updateImpl, or a sharing context's): the cached record indices are the old order's. The
    // traversals of a context run one after the other (they share a spill region), so on ts
    // the fill follows the last traversal that wrote old indices and precedes the first
    // that reads the new tree.
    if (f.seed_cache && (ctx->seedStale || ctx->seedTopologySeen != ctx->sceneStore->worldTopologySeq)) {
        ARK_HIP(launch_fill_u32(ctx->seeds.ptr, ctx->seeds.bytes / 4, seed::kNone, ts));
        ctx->seedStale = false;
        ctx->seedTopologySeen = ctx->sceneStore->worldTopologySeq;
    }
    // (instrumented frames are serial: ts is s)
    if (ctx->counting) ARK_HIP(hipMemsetAsync(ctx->counters.ptr, 0, ctx->counters.bytes, s));
    if (ctx->timing) ARK_HIP(hipEventRecord(ctx->ev[0], s));
    ARK_HIP(launch_probe_slots(f, ts));
    if (f.window_probes > 0) {
        traceZone.begin("Trace rays");
        ARK_HIP(launch_trace(ctx->scene, f, halfWindow(plan, f) ? ctx->pipeTraceBlocks : ctx->traceBlocks, ctx->counting, ts));
        // probeUpdateOffset (k_probe_offsets: from the hit records), so that the
        // next frame's slot table may follow on this stream. The rest of the frame
        // needs only the hit records, but waiting for the offsets too costs less
        // (7 us) than a second cross-stream wait for them at the end of the frame
        // (each wait ~11 us of queue latency, satisfied or not: profiles/r03_v)
        if (plan.pipe) ARK_HIP(launch_probe_offsets(f, ts));
    }
    if (plan.pipe) ARK_HIP(tracedSync(ctx, plan, ts, s));
    return ARK_DDGI_OK;
}

// Shadow rays and shading of the frame's window on s, in the schedule shadeScheduleOf picks:
// the shadow-ray generator, their traversal and k_shade, or for the sun alone with its cover
// map k_shade first and its deferred pass behind the traversal. `shadeWaits` runs before the
// first kernel that reads the atlases. The update's caller part and ark_ddgi_debug_shade.
template<class Waits>
int shadeWindow(ArkDdgiCtx* ctx, const FramePlan& plan, const FrameArgs& f, hipStream_t s, bool timing, Waits&& shadeWaits, FrameArgs* shadeArgs)
{
    const bool count = ctx->counting;
    FrameArgs fs = f;
    fs.spill = ctx->spill.as<uint32_t>(); // region 0
    if (count) ctx->coverFrame = fs;
    // the sun alone, with its cover map: shading resolves the sun's rays itself, and
    // only what the map leaves undecided is listed, traced and shaded in a second pass
    // (not beside a half-occupancy traversal: shade_schedule.h)
    const bool sunOnly = shadeScheduleOf({ f.light_count, ctx->scene.has_sun != 0, ctx->scene.sun_map != nullptr, ctx->desc.flags, halfWindow(plan, f),
                                           ctx->sunOnlySmallWindows }) == ShadeSchedule::SunOnly;
    ctx->lastSunOnly = sunOnly;
    ctx->lastDeferredCount = fs.sun_rays ? fs.sun_count : fs.shadow_count;
    // (the grid stays sized by the window although the cover map leaves a few percent of
    // the sun's rays on the list: an eighth of it measured the same, EXPERIMENTS.md)
    const uint32_t shadowBlocks = count ? ctx->shadowBlocks : shadowBlocksFor(ctx, f.window_rays);
    if (f.light_count > 0 && !sunOnly) {
        ARK_HIP(launch_shadow_gen(ctx->scene, fs, s));
        ARK_HIP(launch_trace_shadow(ctx->scene, fs, shadowBlocks, count, s));
    }
    if (timing) ARK_HIP(hipEventRecord(ctx->ev[5], s));
    ARK_HIP(shadeWaits());
    ARK_HIP(launch_shade(ctx->scene, fs, ctx->shadeBlocks, count, s, sunOnly));
    if (timing) ARK_HIP(hipEventRecord(ctx->ev[2], s));
    if (sunOnly) {
        // (timings: "shade" is pass 1, "shadow" the traversal and the deferred pass)
        ARK_HIP(launch_trace_shadow(ctx->scene, fs, shadowBlocks, count, s));
        ARK_HIP(launch_shade_deferred(ctx->scene, fs, s));
    }
    if (timing) ARK_HIP(hipEventRecord(ctx->ev[4], s));
    *shadeArgs = fs;
    return ARK_DDGI_OK;
}

// The caller's part of the frame on s: shadow rays, shading, the probe update (behind the
// offsets when the frame is serial), then the frame's done signal: word main, or
// evFrameDone[b]. Shading reads the previous frame's atlases at arbitrary probes: on a
// Z-slab rank it waits for the previous exchange first (the traversal did not).
int callerPart(ArkDdgiCtx* ctx, const FramePlan& plan, const FrameArgs& f, hipStream_t s, void* shadeWaitEvent, uint32_t shadeWaitSeq, RoctxRange& traceZone)
{
    const bool timing = ctx->timing;
    auto shadeWaits = [&]() -> hipError_t {
        hipError_t e = shadeWaitEvent ? hipStreamWaitEvent(s, static_cast<hipEvent_t>(shadeWaitEvent), 0) : hipSuccess;
        return e != hipSuccess || !shadeWaitSeq ? e : seqWait(ctx, kSeqExchange, shadeWaitSeq, s);
    };
    if (f.window_probes > 0) {
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[1], s));
        FrameArgs fs;
        if (const int rc = shadeWindow(ctx, plan, f, s, timing, shadeWaits, &fs)) return rc;
        traceZone.end();
        // probeUpdateOffset (serial frames), probeUpdateIrradiance/Visibility + border
        // corners/edges, fused
        RoctxRange updateZone("Update probes");
        if (!plan.pipe) ARK_HIP(launch_probe_offsets(fs, s));
        ARK_HIP(launch_probe_update(fs, s));
    } else {
        ctx->lastSunOnly = false;
        ARK_HIP(shadeWaits());
        if (timing)
            for (int e : { 1, 5, 2, 4 }) ARK_HIP(hipEventRecord(ctx->ev[e], s));
    }
    if (timing) ARK_HIP(hipEventRecord(ctx->ev[3], s));
    if (plan.seq) ARK_HIP(launch_seq_signal(ctx->seqWords.as<uint32_t>() + kSeqMain, plan.seqN, s));
    else ARK_HIP(hipEventRecord(ctx->evFrameDone[plan.b], s));
    return ARK_DDGI_OK;
}

int updateImpl(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, void* hipStream, void* shadeWaitEvent, void* doneEvent, uint32_t shadeWaitSeq = 0)
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
    RoctxRange ddgiZone("DDGI"), traceZone;
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
    // which stream the traversal part runs on and what it waits for (frame_book.h);
    // instrumented updates (per-kernel events, counters) run serially
    const FramePlan plan = ctx->frames.begin(R, ctx->timing || ctx->counting);
    const FrameArgs f = frameArgs(ctx, p, K, R, plan);
    ctx->coverCountsValid = ctx->counting;
    if (const int rc = traversalPart(ctx, plan, f, s, traceZone)) return rc;
    if (const int rc = callerPart(ctx, plan, f, s, shadeWaitEvent, shadeWaitSeq, traceZone)) return rc;
    ctx->lastStream = s;
    if (doneEvent) ARK_HIP(hipEventRecord(static_cast<hipEvent_t>(doneEvent), s));
    ARK_HIP(orderEnd(ctx, s));
    ctx->frames.finished(plan, R);
    ctx->timingValid = ctx->timing;
    ctx->countersPending = ctx->counting;
    ctx->lastRays = f.window_rays;
    ctx->lastProbes = f.window_probes;
    ctx->nextProbeIndex = (f.first + K) % N;
    ctx->lastFirst = f.first;
    ctx->lastK = K;
    return ARK_DDGI_OK;
}

// ark_ddgi_debug_probe_update: the probe update's launches alone as one serial frame, through
// the update's own arguments and the book of the frames in flight, over the surfels the context
// holds and the caller's hit records (no traversal, no shading; the window does not advance).
int probeUpdateImpl(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, const ArkDdgiDebugHit* hits, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!p || p->struct_size != sizeof(ArkDdgiFrameParams)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkDdgiFrameParams");
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const uint32_t K = std::min(p->probe_updates, N);
    const uint32_t R = p->rays_per_probe;
    if (K == 0 || R == 0 || K > static_cast<uint32_t>(ctx->Kmax) || R > static_cast<uint32_t>(ctx->Rmax))
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "probe_updates %u / rays_per_probe %u outside [1,%d] / [1,%d]", K, R, ctx->Kmax, ctx->Rmax);
    if (p->update_offsets && !hits) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "debug_probe_update: update_offsets needs the hit records");
    const hipStream_t s = streamOf(hipStream);
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(orderBegin(ctx, s));
    if (ctx->orderR != R) { // (the slot table's pass stores the samples in traversal order too)
        sampleTraversalOrder(R, ctx->orderHost);
        ARK_HIP(hipMemcpyAsync(ctx->order.ptr, ctx->orderHost.data(), R * 4, hipMemcpyHostToDevice, s));
        ctx->orderR = R;
    }
    const FramePlan plan = ctx->frames.begin(R, true); // serial: every launch in line on s
    FrameArgs f = frameArgs(ctx, p, K, R, plan);
    f.seed_offsets_write = 0u; // planted records name no triangles of a scene
    if (hits && f.window_probes > 0) {
        std::vector<GpuHit> rec(static_cast<size_t>(f.window_probes) * R);
        for (size_t i = 0; i < rec.size(); ++i) rec[i] = GpuHit { hits[i].t, 0.0f, 0.0f, hits[i].tri };
        ARK_HIP(hipMemcpyAsync(f.hits, rec.data(), rec.size() * sizeof(GpuHit), hipMemcpyHostToDevice, s));
        ARK_HIP(hipStreamSynchronize(s)); // rec leaves scope
    }
    ARK_HIP(launch_probe_slots(f, s));
    if (f.window_probes > 0) {
        ARK_HIP(launch_probe_offsets(f, s));
        ARK_HIP(launch_probe_update(f, s));
    }
    ARK_HIP(hipEventRecord(ctx->evFrameDone[plan.b], s));
    ctx->lastStream = s;
    ARK_HIP(orderEnd(ctx, s));
    ctx->frames.finished(plan, R);
    return ARK_DDGI_OK;
}

// The hit records k_shade takes for planted hits, or false with the reason: `words` are the
// front copy's n triangle records (12 words each: the instance in word 9, the primitive in
// word 10, kHoleInstance for a hole), out[i] the record of hits[i]. A miss is {+inf, kNoHit}.
bool shadeHitRecords(const uint32_t* words, uint64_t n, uint32_t instances, float zFar, const ArkDdgiDebugShadeHit* hits, uint64_t count, GpuHit* out,
                     std::string* why)
{
    std::vector<std::vector<uint32_t>> recordOf(instances); // [instance][primitive] -> leaf-order record
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t inst = words[12u * i + 9u], prim = words[12u * i + 10u];
        if (inst == kHoleInstance || inst >= recordOf.size()) continue;
        if (recordOf[inst].size() <= prim) recordOf[inst].resize(static_cast<size_t>(prim) + 1u, kNoHit);
        if (recordOf[inst][prim] == kNoHit) recordOf[inst][prim] = static_cast<uint32_t>(i);
    }
    char msg[160];
    for (uint64_t i = 0; i < count; ++i) {
        const ArkDdgiDebugShadeHit& h = hits[i];
        if (h.instance == 0xffffffffu) {
            out[i] = GpuHit { __builtin_bit_cast(float, 0x7f800000u), 0.0f, 0.0f, kNoHit };
            continue;
        }
        msg[0] = 0;
        if (h.instance >= recordOf.size() || h.primitive >= recordOf[h.instance].size() || recordOf[h.instance][h.primitive] == kNoHit)
            std::snprintf(msg, sizeof(msg), "record %llu names no triangle of the scene (instance %u, primitive %u)", (unsigned long long)i, h.instance, h.primitive);
        else if (!std::isfinite(h.t) || !(std::fabs(h.t) >= 0.0001f && std::fabs(h.t) <= zFar))
            std::snprintf(msg, sizeof(msg), "record %llu has t = %g, |t| must be in [1e-4, %g]", (unsigned long long)i, static_cast<double>(h.t), static_cast<double>(zFar));
        else if (!std::isfinite(h.u) || !std::isfinite(h.v) || h.u < 0.0f || h.v < 0.0f || h.u + h.v > 1.0f)
            std::snprintf(msg, sizeof(msg), "record %llu has barycentrics (%g, %g) outside the triangle", (unsigned long long)i, static_cast<double>(h.u), static_cast<double>(h.v));
        if (msg[0]) {
            if (why) *why = msg;
            return false;
        }
        out[i] = GpuHit { h.t, h.u, h.v, recordOf[h.instance][h.primitive] };
    }
    return true;
}

// ark_ddgi_debug_shade: hit shading alone as one serial frame, through the update's own
// arguments and the book of the frames in flight: the slot table, the caller's hit records in
// place of the primary traversal, then shadeWindow - the shadow rays really traced from the
// planted hit points. No offsets, no blend; the window does not advance.
// A record reaches the kernels only as the leaf-order index of a triangle record the front copy
// holds, with barycentrics inside the triangle and a finite t in [1e-4, zFar]: everything the
// kernels index by it (the shading record, its instance, material and textures) is then the
// scene's own, sampleTexture wraps every texel coordinate into its texture and sampleDDGI
// clamps every probe coordinate into the grid, so no planted record can make them read out
// of bounds. Everything else is refused before the first launch.
int shadeImpl(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, const ArkDdgiDebugShadeHit* hits, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!p || p->struct_size != sizeof(ArkDdgiFrameParams)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkDdgiFrameParams");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_debug_shade before ark_ddgi_set_scene");
    if (!hits) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "debug_shade: no hit records");
    const uint32_t N = static_cast<uint32_t>(ctx->N);
    const uint32_t K = std::min(p->probe_updates, N);
    const uint32_t R = p->rays_per_probe;
    if (K == 0 || R == 0 || K > static_cast<uint32_t>(ctx->Kmax) || R > static_cast<uint32_t>(ctx->Rmax))
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "probe_updates %u / rays_per_probe %u outside [1,%d] / [1,%d]", K, R, ctx->Kmax, ctx->Rmax);
    const hipStream_t s = streamOf(hipStream);
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(hipSetDevice(ctx->device));
    // the front copy's records, downloaded from an idle device (as the host restatements' entries do)
    ARK_HIP(hipDeviceSynchronize());
    if (ctx->sceneVersion != ctx->sceneStore->version)
        if (const int rc = refreshScene(ctx)) return rc;
    std::vector<uint32_t> words;
    std::vector<int32_t> classOf;
    if (const int rc = sceneRecordsAndClasses(*ctx->sceneStore, ctx, words, classOf)) return rc;
    const uint32_t first = p->first_probe_index % N;
    const size_t rays = static_cast<size_t>(countSlabProbes(ctx, first, K)) * R;
    std::vector<GpuHit> rec(rays);
    std::string why;
    if (!shadeHitRecords(words.data(), words.size() / 12u, static_cast<uint32_t>(classOf.size()), ctx->desc.z_far, hits, rays, rec.data(), &why))
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "debug_shade: %s", why.c_str());
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(flushLights(ctx, s));
    if (ctx->orderR != R) {
        sampleTraversalOrder(R, ctx->orderHost);
        ARK_HIP(hipMemcpyAsync(ctx->order.ptr, ctx->orderHost.data(), R * 4, hipMemcpyHostToDevice, s));
        ctx->orderR = R;
    }
    const FramePlan plan = ctx->frames.begin(R, true); // serial: every launch in line on s
    FrameArgs f = frameArgs(ctx, p, K, R, plan);
    f.seed_offsets_write = 0u; // no traversal: the hit candidates are not written
    ctx->coverCountsValid = ctx->counting;
    if (ctx->counting) ARK_HIP(hipMemsetAsync(ctx->counters.ptr, 0, ctx->counters.bytes, s));
    ARK_HIP(launch_probe_slots(f, s));
    if (f.window_probes > 0) {
        ARK_HIP(hipMemcpyAsync(f.hits, rec.data(), rec.size() * sizeof(GpuHit), hipMemcpyHostToDevice, s));
        ARK_HIP(hipStreamSynchronize(s)); // rec leaves scope
        FrameArgs fs;
        if (const int rc = shadeWindow(ctx, plan, f, s, false, [] { return hipSuccess; }, &fs)) return rc;
    } else {
        ctx->lastSunOnly = false;
    }
    ARK_HIP(hipEventRecord(ctx->evFrameDone[plan.b], s));
    ctx->lastStream = s;
    ARK_HIP(orderEnd(ctx, s));
    ctx->frames.finished(plan, R);
    return ARK_DDGI_OK;
}

// The last window as Z-slab ranks exchange it (ark_ddgi_window_exchange_info)
ArkDdgiWindowExchange windowExchangeInfo(const ArkDdgiCtx* ctx)
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

int windowPack(ArkDdgiCtx* ctx, void* buf, uint64_t bytes, void* hipStream, bool unpack)
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

} // namespace

// Fail-closed frame sequencing (VERDICT r03 "do this" #3): a k_seq_wait that gave up
// has set the context's timed-out word, so every path kernel that starts after it
// skips (frameAborted) and leaves atlases, surfels and offsets as they were (a launch
// already running when the wait gave up completes). The first context
// call that sees the host-mapped flag drains the device (the late producer ends by
// itself), clears both words, switches the context to event sequencing (which no
// queue order can stall; FrameBook::timedOut) and reports ARK_DDGI_E_DEVICE; the calls after it run.
int ark::debugProbeUpdate(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, const ArkDdgiDebugHit* hits, void* hipStream)
{
    return probeUpdateImpl(ctx, p, hits, hipStream);
}

int ark::debugShadeMap(const uint32_t* words, uint64_t n, uint32_t instances, float zFar, const ArkDdgiDebugShadeHit* hits, uint64_t count, uint32_t* outTri)
{
    if ((n && !words) || (count && (!hits || !outTri))) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::vector<GpuHit> rec(count);
    if (!shadeHitRecords(words, n, instances, zFar, hits, count, rec.data(), nullptr)) return ARK_DDGI_E_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < count; ++i) outTri[i] = rec[i].tri;
    return ARK_DDGI_OK;
}

int ark::debugShade(ArkDdgiCtx* ctx, const ArkDdgiFrameParams* p, const ArkDdgiDebugShadeHit* hits, void* hipStream)
{
    return shadeImpl(ctx, p, hits, hipStream);
}

int ark::checkSequencing(ArkDdgiCtx* ctx)
{
    if (!ctx->hostAbort || __atomic_load_n(ctx->hostAbort, __ATOMIC_ACQUIRE) == 0u) return ARK_DDGI_OK;
    ARK_HIP(hipSetDevice(ctx->device));
    // the whole device (ADVICE r04 low asked for the context's own streams only): the
    // late producer may sit on a caller's stream (an exchange stream) whose end the
    // context recorded as a sequence word; once the context switches to events, nothing
    // else would order the next frame's shading after it
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemset(ctx->seqWords.as<uint32_t>() + kSeqTimedOut, 0, 4));
    __atomic_store_n(ctx->hostAbort, 0u, __ATOMIC_RELEASE);
    ctx->frames.timedOut();
    return ctx->fail(ARK_DDGI_E_DEVICE,
                     "a frame-sequencing wait between the context's streams gave up after %u ms: every update kernel that started after it skipped "
                     "(its atlases, surfels and offsets left as they were); the context now orders its streams with events",
                     ctx->seqTimeoutMs);
}

extern "C" {

int ark_ddgi_set_sequencing(ArkDdgiCtx* ctx, int device_sequence_words, uint32_t timeout_ms)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (timeout_ms > 3600u * 1000u) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "sequencing timeout %u ms above one hour", timeout_ms);
    ctx->frames.setSequencing(device_sequence_words != 0);
    if (timeout_ms) {
        ctx->seqTimeoutMs = timeout_ms;
        ctx->seqTimeoutTicks = ctx->wallClockKhz * timeout_ms;
    }
    return ARK_DDGI_OK;
}

int ark_ddgi_get_sequencing(const ArkDdgiCtx* ctx, int* out_device_sequence_words, uint32_t* out_timeout_ms, uint32_t* out_timeouts)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (out_device_sequence_words) *out_device_sequence_words = ctx->frames.words() ? 1 : 0;
    if (out_timeout_ms) *out_timeout_ms = ctx->seqTimeoutMs;
    if (out_timeouts) *out_timeouts = ctx->frames.timeouts();
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
    const uint32_t wait = ctx->frames.exchangePending();
    // without sequence words the exchange's end is an event (ark_ddgi_exchange_end)
    const int r = ctx->frames.words() ? updateImpl(ctx, p, hipStream, nullptr, nullptr, wait)
                                      : updateImpl(ctx, p, hipStream, wait ? ctx->evExchangeDone : nullptr, nullptr);
    if (r == ARK_DDGI_OK) ctx->frames.exchangeWaited();
    return r;
}

int ark_ddgi_exchange_begin(ArkDdgiCtx* ctx, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    const hipStream_t x = streamOf(hipStream);
    if (const int r = checkSequencing(ctx)) return r;
    ARK_HIP(hipSetDevice(ctx->device));
    if (ctx->frames.lastMainSeq()) {
        ARK_HIP(seqWait(ctx, kSeqMain, ctx->frames.lastMainSeq(), x));
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
    const uint32_t n = ctx->frames.exchangeNumber();
    if (ctx->frames.words()) ARK_HIP(launch_seq_signal(ctx->seqWords.as<uint32_t>() + kSeqExchange, n, streamOf(hipStream)));
    else ARK_HIP(hipEventRecord(ctx->evExchangeDone, streamOf(hipStream)));
    ctx->frames.exchangeEnded(n);
    return ARK_DDGI_OK;
}

int ark_ddgi_window_exchange_info(const ArkDdgiCtx* ctx, ArkDdgiWindowExchange* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    *out = windowExchangeInfo(ctx);
    return ARK_DDGI_OK;
}

int ark_ddgi_pack_window(ArkDdgiCtx* ctx, void* dst, uint64_t bytes, void* hipStream) { return windowPack(ctx, dst, bytes, hipStream, false); }

int ark_ddgi_unpack_window(ArkDdgiCtx* ctx, const void* src, uint64_t bytes, void* hipStream)
{
    return windowPack(ctx, const_cast<void*>(src), bytes, hipStream, true);
}

int ark_ddgi_mark_external_write(ArkDdgiCtx* ctx)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ctx->frames.externalWrite();
    return ARK_DDGI_OK;
}

int ark_ddgi_synchronize(ArkDdgiCtx* ctx)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    return checkSequencing(ctx);
}

} // extern "C"
