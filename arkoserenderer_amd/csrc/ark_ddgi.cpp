// ark_ddgi.cpp — the C-ABI context of the MI355X DDGI path (include/ark_ddgi.h).
//
// Owns all device memory of one DDGI node instance on one GPU: the persistent
// atlases/offsets (the DDGISamplingSet, DDGINode.cpp:62-66), the per-update
// working set (slot table, hit records, surfels) and the scene (BVH + RT mesh
// data + materials + lights). Every update is enqueued on one HIP stream.
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ark_ddgi.h"
#include "../../include/ark_ddgi_debug.h"
#include "ark_fmath.h"
#include "bvh_builder.h"
#include "ddgi_kernels.h"

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

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipError_t alloc(size_t n)
    {
        release();
        bytes = n;
        if (n == 0) return hipSuccess;
        return hipMalloc(&ptr, n);
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template<typename T> T* as() const { return static_cast<T*>(ptr); }
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

// One BVH8 set on the device - the world's three classes, or the sun's light-space BVH -
// with what its refits need. One allocation: the nodes, then the triangle records at the
// next 256-B boundary (the traversal addresses both through one buffer resource with a
// 32-bit byte offset), then one padding record (a five-load fetch of the last record
// stays in bounds, ARK_FETCH5).
struct DeviceBvh {
    DeviceBuffer buf; // the front copy: what the kernels read (SceneStore::Spare holds the others)
    size_t triOffset = 0;
    uint64_t nodeCount = 0, records = 0; // records: holes included, the padding record not
    uint32_t depth = 0;
    float inflateAbs = 0.0f; // the build's absolute box inflation (the refits' floor)
    // the refit: order[levelOffsets[i] .. [i + 1]) on the device = the nodes of one depth,
    // deepest first; its boxes scratch; the node masks (k_node_masks: per topology)
    DeviceBuffer order, boxes, masks;
    std::vector<uint32_t> levelOffsets;
    bool masksValid = false;
    static size_t triOffsetFor(uint64_t nodes) { return (nodes * sizeof(GpuBvh8Node) + 255) & ~static_cast<size_t>(255); }
    static size_t bytesFor(uint64_t nodes, uint64_t records) { return triOffsetFor(nodes) + (records + 1) * sizeof(GpuTriangle); }
    // nodes and records of a copy of it (the front one, or a spare)
    GpuBvh8Node* nodes(const DeviceBuffer& copy) const { return copy.as<GpuBvh8Node>(); }
    GpuTriangle* tris(const DeviceBuffer& copy) const { return reinterpret_cast<GpuTriangle*>(static_cast<char*>(copy.ptr) + triOffset); }
    void release()
    {
        for (DeviceBuffer* b : { &buf, &order, &boxes, &masks }) b->release();
    }
};

// `nodes` and `tris` into b.buf (allocated here; b's offset and counts set). s == nullptr:
// synchronous copies; else stream-ordered on `s` and complete on return.
static hipError_t uploadBvh(const std::vector<GpuBvh8Node>& nodes, std::vector<GpuTriangle>& tris, hipStream_t s, DeviceBvh& b)
{
    b.triOffset = DeviceBvh::triOffsetFor(nodes.size());
    b.nodeCount = nodes.size();
    b.records = tris.size();
    auto copy = [s](void* dst, const void* src, size_t n) { return s ? hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s) : hipMemcpy(dst, src, n, hipMemcpyHostToDevice); };
    tris.push_back(GpuTriangle {}); // the padding record
    hipError_t e = b.buf.alloc(DeviceBvh::bytesFor(b.nodeCount, b.records));
    if (e == hipSuccess) e = copy(b.buf.ptr, nodes.data(), nodes.size() * sizeof(GpuBvh8Node));
    if (e == hipSuccess) e = copy(b.tris(b.buf), tris.data(), tris.size() * sizeof(GpuTriangle));
    if (e == hipSuccess && s) e = hipStreamSynchronize(s);
    tris.pop_back();
    return e;
}

// A background rebuild of the sun's light-space BVH (sunRebuildStep): a host thread
// waits for a device snapshot of the world BVHs' triangle records (taken in stream
// order behind the refits, `snap` / `evSnap`), builds the BVH for `dir` and uploads it
// into `bvh`; `done` set last (release).
struct SunJob {
    std::thread t;
    std::atomic<bool> done { false };
    float dir[3] {};
    uint32_t version = 0; // SceneStore::version of the snapshot
    uint32_t refitsAt = 0; // SceneStore::refitCount of the snapshot (later refits: refitted forward at install)
    DeviceBuffer snap;    // the records it builds from
    hipEvent_t evSnap = nullptr;
    DeviceBvh bvh;        // the result (its level order still on the host: levelOrder)
    std::vector<uint32_t> levelOrder;
    double frame[9] {};
    float ms = 0.0f;
    bool ok = false;
    ~SunJob()
    {
        if (t.joinable()) t.join();
        bvh.release(); // not installed (an installed one was moved to the scene)
        snap.release();
        if (evSnap) (void)hipEventDestroy(evSnap);
    }
};

// A background rebuild of the world BVHs after refits (worldCollect / worldStart; the reference
// rebuilds its TLAS in full every 60 frames, GpuScene.cpp:998-1010): a host thread takes
// a device snapshot of the refitted triangle records, builds the three hit-mask classes'
// BVHs anew from them (set_scene's builder), keeps every record's words as they were
// (so hits stay bit-identical) and uploads nodes + records, the new record order's
// source indices (perm, for the shading records) and the refit's level order.
struct WorldJob {
    std::thread t;
    std::atomic<bool> done { false };
    uint32_t version = 0, refitsAt = 0;
    DeviceBuffer snap;
    hipEvent_t evSnap = nullptr;
    uint64_t snapRecords = 0;
    std::vector<int> classOf; // instance -> hit-mask class (0 opaque, 1 masked, 2 blend)
    DeviceBvh bvh;            // the result, its level order uploaded
    DeviceBuffer perm;
    int32_t roots[3] { -1, -1, -1 };
    uint32_t opaqueNodes = 0, maxLeaf = 0;
    float sah = 0.0f;
    float ms = 0.0f;
    bool ok = false;
    // runWorldJobGpu: the device built the result; or it handed the job to the host build
    // (t0: the job's start, so that ms stays the whole job's wall time)
    bool gpu = false, gpuFallback = false;
    std::chrono::steady_clock::time_point t0 {};
    std::string error;
    ~WorldJob()
    {
        if (t.joinable()) t.join();
        bvh.release();
        for (DeviceBuffer* b : { &perm, &snap }) b->release();
        if (evSnap) (void)hipEventDestroy(evSnap);
    }
};

// A buffer replaced while launches enqueued before may still read it: freed once `done`
// (recorded behind them) has completed.
struct Retired {
    DeviceBuffer buf;
    hipEvent_t done = nullptr;
};

// The scene of a context on the device (ark_ddgi_set_scene): BVH nodes + triangles,
// shading records, RT mesh data, materials, textures, lights. Reference-counted:
// ark_ddgi_share_scene lets the Z-slab contexts of one GPU use one copy.
struct SceneStore {
    int device = 0;
    DeviceBuffer triNormals, indices, vertices, positions, meshes, materials, instances, texInfos, texels;
    // the world BVHs (args) and the light-space BVH8 of the sun's shadow rays with its
    // world-space triangle records (sunArgs; nodeCount 0: none). The light-space BVH follows
    // the motion: refitted with the world BVHs (its records re-transformed, its boxes of
    // their light coordinates, sunFrameD)
    DeviceBvh world, sun;
    float sunCostWorld = 0.0f, sunCostLight = 0.0f; // sampled sun shadow-ray steps per ray (sun_shadow_cost)
    std::vector<ArkRTInstance> instHost;     // the AO bake (instance -> mesh segment), set_instances' topology check
    std::vector<ArkRTTriangleMesh> meshHost;
    SceneArgs args {};    // the world BVHs, pools, materials, textures (lights: per context, deriveSceneArgs)
    SceneArgs sunArgs {}; // sun_nodes / sun_tris / sun_root / sun_frame of the light-space BVH (sun_root -1: none)
    float sunDirBuilt[3] { 0, 0, 0 }; // the sun direction the light-space BVH was built for
    // the scene's lights as set_scene got them: a context's lights until ark_ddgi_set_lights
    int32_t hasSunScene = 0;
    ArkDirectionalLight sunScene {};
    std::vector<GpuSpotLight> spotsScene;
    ArkDdgiBvhStats bvhStats {};
    uint32_t bvhMaxDepth = 0; // deepest of the world BVHs and the sun's (traversal spill)
    // ark_ddgi_set_instances: bumped by every refit and install (a sharing context
    // re-derives its SceneArgs); the refit's transforms on the device
    uint32_t version = 0;
    DeviceBuffer refitInst;
    double sunFrameD[9] {};
    // the refit's transforms: the last ones uploaded (dirty = changed since the records
    // were written); pinned staging of the stream-ordered uploads, two sets in turn
    std::vector<RefitInstance> refitHost;
    // pinned staging of the per-frame uploads, a ring: a slot is reused once its copy (a
    // few calls back) has run, so the host runs up to kStageSlots / 2 frames of
    // set_instances_async ahead of the device (two slots: one frame, and every call
    // waited for the previous frame's refit)
    static constexpr int kStageSlots = 8;
    void* stage[kStageSlots] {};
    size_t stageBytes[kStageSlots] {};
    hipEvent_t stageDone[kStageSlots] {};
    int stageNext = 0;
    // object-space bounds of every instance's triangles (set_scene): the refit's world and
    // light-space bounds, for its box inflation, from the instances' transforms on the host
    std::vector<std::array<float, 6>> instObjBox;
    // The geometry a refit writes comes in three copies: the front one (world.buf, sun.buf,
    // instances above: what the kernels read) and two spares. A refit brings the next
    // spare from the transforms it holds (xf[slot]) to the new ones on the context's
    // refit stream and makes it the front one: it waits only for the operations that read
    // that copy while it was the front one, two refits before (the frame before last),
    // so that it runs beside the frame in flight's traversal and the next traversal does
    // not wait for it (with two copies it waited for the previous frame's shading, and
    // the frames ran one after the other: C4 4.3 ms per moving frame, static 3.3). An
    // install (a new topology) drops the spares; the next refit copies the front one.
    struct Spare {
        DeviceBuffer world, sun, instances;
        bool valid = false;
        int slot = 0;
    };
    Spare spare[2]; // spare[0]: the next refit's target
    // the inflations each copy's boxes hold ([slot][0 world, 1 sun]); refitFull: the next
    // refit reaches every node (a new topology, or boxes scratch not of this one)
    bool refitFull = true;
    float inflCopy[3][2] {};
    int front = 0; // slot of the front copy (xf index)
    std::vector<std::array<float, 12>> xf[3];
    // the light-space BVH follows the sun: set_scene chose it (sunWanted), and after a
    // sun-direction change it is rebuilt in the background (sunRebuildStep)
    bool sunWanted = false;
    int buildThreads = 16;
    std::unique_ptr<SunJob> sunJob;
    uint32_t sunRebuilds = 0;
    // rebuild requests (sunRebuildStep): the sun direction the contexts sharing this scene
    // asked for last and how many calls in a row asked for it; a rebuild starts only on a
    // stable request (>= 2), so contexts under different suns never start rebuilds that
    // undo each other. A failed build is remembered (direction and
    // scene version) and not retried until either changes.
    float sunReqDir[3] { 0, 0, 0 };
    uint32_t sunReqStreak = 0;
    bool sunFailed = false;
    float sunFailedDir[3] { 0, 0, 0 };
    uint32_t sunFailedVersion = 0;
    uint32_t sunFailures = 0;
    // the world BVHs' background rebuild (worldCollect / worldStart): refits since the installed
    // BVHs were built, the running job, rebuilds installed
    uint32_t refitsSinceBuild = 0, sunRefitsSinceBuild = 0;
    std::unique_ptr<WorldJob> worldJob;
    uint32_t worldRebuilds = 0, refitCount = 0;
    bool worldRebuildFailed = false;
    // ARK_DDGI_FLAG_GPU_REBUILD: the installed world BVHs are a device build (an LBVH: once
    // the motion stops one host rebuild replaces it, worldSettleWanted)
    bool worldGpuBuilt = false;
    // the background build started last (loosenedTurn: loosened BVHs take turns)
    enum : uint8_t { kBackgroundNone, kBackgroundWorld, kBackgroundSun };
    uint8_t lastBackground = kBackgroundNone;
    std::vector<Retired> retired;
    SceneStore() = default;
    SceneStore(const SceneStore&) = delete;
    SceneStore& operator=(const SceneStore&) = delete;
    ~SceneStore()
    {
        (void)hipSetDevice(device);
        sunJob.reset(); // joins them: the jobs read snapshots freed below
        worldJob.reset();
        (void)hipDeviceSynchronize();
        for (Retired& r : retired) {
            r.buf.release();
            if (r.done) (void)hipEventDestroy(r.done);
        }
        for (int i = 0; i < kStageSlots; ++i) {
            if (stage[i]) (void)hipHostFree(stage[i]);
            if (stageDone[i]) (void)hipEventDestroy(stageDone[i]);
        }
        world.release();
        sun.release();
        for (DeviceBuffer* b : { &triNormals, &indices, &vertices, &positions, &meshes, &materials, &instances, &texInfos, &texels, &refitInst, &spare[0].world,
                                 &spare[0].sun, &spare[0].instances, &spare[1].world, &spare[1].sun, &spare[1].instances })
            b->release();
    }
};

struct ArkDdgiCtx {
    ArkDdgiDesc desc {};
    std::string lastError;
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
    bool timing = false;
    hipEvent_t ev[6] = {};
    float lastMs[5] = {};
    bool timingValid = false;
    ArkDdgiCounters lastCounters {};
    bool countersPending = false;
    uint64_t lastRays = 0, lastProbes = 0;
    uint32_t nextProbeIndex = 0; // (first + K) % N of the last update, or of a loaded state
    uint32_t lastFirst = 0, lastK = 0; // the last update's window (ark_ddgi_window_exchange_info)
    // a refit or an installed rebuild enqueued on a caller's stream (ark_ddgi_set_instances_async,
    // worldCollect): the next update's traversal on the traversal stream waits for it
    hipEvent_t evRefit = nullptr;
    bool refitPending = false;
    // ark_ddgi_set_instances_async's refits run on refitStream (SceneStore::spare):
    // evFree[slot] ends with the operations that read that slot's copy while it was the
    // front one (recorded when a refit swapped it out, on the stream of the last
    // operation, which follows the others); evInstalled with the last install (a rebuild
    // installed on a caller's stream writes the front copy)
    hipStream_t refitStream = nullptr;
    hipEvent_t evFree[3] = {};
    bool freeValid[3] = { false, false, false };
    hipEvent_t evInstalled = nullptr;
    bool installValid = false;

    int fail(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        lastError = buf;
        return code;
    }
    int hipFail(hipError_t e, const char* what)
    {
        return fail(ARK_DDGI_E_DEVICE, "%s: %s", what, hipGetErrorString(e));
    }
};

#define ARK_HIP(expr)                                                   \
    do {                                                                \
        hipError_t _e = (expr);                                         \
        if (_e != hipSuccess) return ctx->hipFail(_e, #expr);           \
    } while (0)

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

template<typename T>
int upload(ArkDdgiCtx* ctx, DeviceBuffer& buf, const T* data, size_t count)
{
    size_t bytes = count * sizeof(T);
    ARK_HIP(buf.alloc(std::max<size_t>(bytes, 16)));
    if (bytes) ARK_HIP(hipMemcpy(buf.ptr, data, bytes, hipMemcpyHostToDevice));
    return ARK_DDGI_OK;
}

static_assert(ARK_DDGI_MAX_SPOT_LIGHTS == kMaxLights - 1, "spot light capacity");

// SpotLightData as the closest hit reads it (GpuScene.cpp:844-858: the fields of
// LightData.h:19-40 the DDGI path uses)
GpuSpotLight gpuSpotLight(const ArkSpotLight& sl)
{
    GpuSpotLight g;
    std::memset(&g, 0, sizeof(g));
    for (int k = 0; k < 3; ++k) {
        g.color[k] = sl.color[k];
        g.direction[k] = sl.world_space_direction[k];
        g.right[k] = sl.world_space_right[k];
        g.up[k] = sl.world_space_up[k];
        g.position[k] = sl.world_space_position[k];
    }
    g.position[3] = sl.outer_cone_half_angle;
    g.ies_texture = sl.ies_profile_index;
    return g;
}

// f(begin, end) over [0, n) in `threads` contiguous chunks (one when n is small)
template<class F>
void parallelFor(size_t n, int threads, F f)
{
    const int T = std::max(1, std::min<int>(threads, static_cast<int>(n >> 16) + 1));
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back([&, t] { f(n * t / T, n * (t + 1) / T); });
    f(0, n / T);
    for (std::thread& th : pool) th.join();
}

// sRGB EOTF applied per texel before filtering (Vulkan sRGB formats).
float srgbToLinear(float c)
{
    return c <= 0.04045f ? c / 12.92f : powf_((c + 0.055f) / 1.055f, 2.4f);
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

// --- scene maintenance: stream-ordered refits, background rebuilds ------------------

// A buffer the launches enqueued so far on `s` (and, through orderBegin, everything the
// context enqueued before) may read: freed by collectRetired once they are done.
hipError_t retireBuffer(SceneStore& st, DeviceBuffer& b, hipStream_t s)
{
    if (!b.ptr) return hipSuccess;
    Retired r;
    hipError_t e = hipEventCreateWithFlags(&r.done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(r.done, s);
    if (e != hipSuccess) {
        if (r.done) (void)hipEventDestroy(r.done);
        (void)hipStreamSynchronize(s); // cannot defer: wait, then free
        b.release();
        return e;
    }
    r.buf = b;
    b = DeviceBuffer {};
    st.retired.push_back(r);
    return hipSuccess;
}

void collectRetired(SceneStore& st)
{
    for (size_t i = 0; i < st.retired.size();) {
        Retired& r = st.retired[i];
        if (hipEventQuery(r.done) == hipSuccess) {
            r.buf.release();
            (void)hipEventDestroy(r.done);
            st.retired[i] = st.retired.back();
            st.retired.pop_back();
        } else {
            ++i;
        }
    }
}

// `bytes` of host data into `dst` in stream order on `s`, through the store's pinned
// staging ring (a slot is reused once its previous copy has run).
hipError_t stagedUpload(SceneStore& st, void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return hipSuccess;
    const int i = st.stageNext;
    st.stageNext = (i + 1) % SceneStore::kStageSlots;
    hipError_t e = hipSuccess;
    if (!st.stageDone[i] && (e = hipEventCreateWithFlags(&st.stageDone[i], hipEventDisableTiming)) != hipSuccess) return e;
    if (st.stageBytes[i]) (void)hipEventSynchronize(st.stageDone[i]); // its last copy (an earlier frame's) has run
    if (st.stageBytes[i] < bytes) {
        if (st.stage[i]) (void)hipHostFree(st.stage[i]);
        st.stage[i] = nullptr;
        st.stageBytes[i] = 0;
        if ((e = hipHostMalloc(&st.stage[i], bytes, hipHostMallocDefault)) != hipSuccess) return e;
        st.stageBytes[i] = bytes;
    }
    std::memcpy(st.stage[i], src, bytes);
    if ((e = hipMemcpyAsync(dst, st.stage[i], bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return hipEventRecord(st.stageDone[i], s);
}

// The boxes' absolute inflations of a refit, as set_scene and build_sun_bvh derive them
// from the records' bounds (world: bvh8_inflation_box, 1e-6 |diagonal|; light space:
// 2 x 1e-6 |light diagonal| + 2e-6 max |world coordinate|), here from bounds that
// contain the records: every instance's object-space box (st.instObjBox) through its
// current transform (st.refitHost), corner by corner in double, and those corners in the
// sun's frame. Never less than the build's (DeviceBvh::inflateAbs). Larger
// bounds only loosen the boxes; the hits do not depend on them.
void refitInflations(const SceneStore& st, float& world, float& light)
{
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    double llo[3] = { INFINITY, INFINITY, INFINITY }, lhi[3] = { -INFINITY, -INFINITY, -INFINITY };
    double maxAbs = 0.0;
    const size_t n = std::min(st.instObjBox.size(), st.refitHost.size());
    for (size_t i = 0; i < n; ++i) {
        const std::array<float, 6>& b = st.instObjBox[i];
        if (!(b[0] <= b[3])) continue; // no triangles
        const float* M = st.refitHost[i].m;
        for (int c = 0; c < 8; ++c) {
            const double P[3] = { b[(c & 1) ? 3 : 0], b[(c & 2) ? 4 : 1], b[(c & 4) ? 5 : 2] };
            double w[3];
            for (int r = 0; r < 3; ++r) {
                w[r] = double(M[4 * r]) * P[0] + double(M[4 * r + 1]) * P[1] + double(M[4 * r + 2]) * P[2] + double(M[4 * r + 3]);
                lo[r] = std::min(lo[r], w[r]);
                hi[r] = std::max(hi[r], w[r]);
                maxAbs = std::max(maxAbs, std::fabs(w[r]));
            }
            for (int r = 0; r < 3; ++r) {
                const double L = st.sunFrameD[3 * r] * w[0] + st.sunFrameD[3 * r + 1] * w[1] + st.sunFrameD[3 * r + 2] * w[2];
                llo[r] = std::min(llo[r], L);
                lhi[r] = std::max(lhi[r], L);
            }
        }
    }
    auto box = [](const double* l, const double* h) {
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a)
            if (h[a] >= l[a]) d2 += (h[a] - l[a]) * (h[a] - l[a]);
        return 1e-6 * std::sqrt(d2);
    };
    // rounded up to fp32 (the bounds' own rounding to fp32 in the builds is within it)
    world = std::max(st.world.inflateAbs, std::nextafter(static_cast<float>(box(lo, hi)), INFINITY));
    light = std::max(st.sun.inflateAbs, std::nextafter(static_cast<float>(2.0 * box(llo, lhi) + 2e-6 * maxAbs), INFINITY));
}

// The inflation of the refitted boxes rounded up to a power of two: it changes only when
// the scene's extent crosses one, so that a refit rarely has to touch the nodes of the
// instances that did not move (a change refits every node).
float inflationStep(float x) { return x > 0.0f ? std::ldexp(1.0f, static_cast<int>(std::ceil(std::log2(static_cast<double>(x))))) : x; }

// The refit of one BVH's copy `copy` on `s`, level by level: the nodes with an instance of
// `dirty` below them (the node masks, k_node_masks, computed first when the topology is
// new), or every node (refitFull, or an inflation other than the one the copy's boxes
// hold, `held`: updated).
int refitBvh(ArkDdgiCtx* ctx, SceneStore& st, DeviceBvh& b, const DeviceBuffer& copy, RefitBoxArgs args, uint64_t dirty, float& held, hipStream_t s)
{
    GpuBvh8Node* nodes = b.nodes(copy);
    GpuTriangle* tris = b.tris(copy);
    const uint32_t* order = b.order.as<uint32_t>();
    const std::vector<uint32_t>& lv = b.levelOffsets;
    if (!b.masksValid) {
        if (b.masks.bytes < std::max<uint64_t>(8, b.nodeCount * 8)) {
            ARK_HIP(retireBuffer(st, b.masks, s));
            ARK_HIP(b.masks.alloc(std::max<uint64_t>(8, b.nodeCount * 8)));
        }
        for (size_t l = 0; l + 1 < lv.size(); ++l) ARK_HIP(launch_node_masks(nodes, tris, b.masks.as<uint64_t>(), order + lv[l], lv[l + 1] - lv[l], s));
        b.masksValid = true;
    }
    args.dirty = (st.refitFull || args.inflate != held) ? ~0ull : dirty;
    for (size_t l = 0; l + 1 < lv.size(); ++l)
        ARK_HIP(launch_refit_nodes(nodes, tris, b.boxes.as<float>(), order + lv[l], lv[l + 1] - lv[l], args, b.masks.as<uint64_t>(), st.refitInst.as<RefitInstance>(),
                                   st.indices.as<uint32_t>(), st.positions.as<float>(), s));
    held = args.inflate;
    return ARK_DDGI_OK;
}

// The refit of the copy (`world`, `sun`; slot: the transforms and inflations it holds) of
// every BVH of the scene on `s`: the records of the moved instances (st.refitInst's dirty
// flags: those whose transform differs from the copy's) re-transformed, the boxes and
// planes above them recomputed - the world BVHs, then the light-space sun BVH (its boxes
// of the records' light coordinates). The boxes' inflations from the instances' bounds
// (refitInflations, host).
int enqueueRefit(ArkDdgiCtx* ctx, SceneStore& st, hipStream_t s, const DeviceBuffer& world, const DeviceBuffer& sun, int slot)
{
    float inflateWorld = 0.0f, inflateLight = 0.0f;
    refitInflations(st, inflateWorld, inflateLight);
    uint64_t dirty = 0;
    for (size_t i = 0; i < st.refitHost.size(); ++i)
        if (st.refitHost[i].dirty) dirty |= 1ull << (i & 63u);
    RefitBoxArgs a {};
    a.inflate = inflationStep(inflateWorld);
    a.light = 0;
    if (const int rc = refitBvh(ctx, st, st.world, world, a, dirty, st.inflCopy[slot][0], s)) return rc;
    if (st.sunArgs.sun_root >= 0 && st.sun.records && !st.sun.levelOffsets.empty()) {
        std::memcpy(a.frame, st.sunFrameD, sizeof(a.frame));
        a.inflate = inflationStep(inflateLight);
        a.light = 1;
        if (const int rc = refitBvh(ctx, st, st.sun, sun, a, dirty, st.inflCopy[slot][1], s)) return rc;
    }
    st.refitFull = false;
    return ARK_DDGI_OK;
}

// The refit's transforms of `instances` on the device (stream-ordered), every one dirty
// (have = nullptr: the records are of an older version, an installed rebuild) or those
// whose transform differs from the one the target copy's records hold (`have`).
int uploadRefitInstances(ArkDdgiCtx* ctx, SceneStore& st, const ArkRTInstance* instances, uint32_t count, const std::vector<std::array<float, 12>>* have,
                         hipStream_t s)
{
    bool allDirty = !have || have->size() != count;
    if (st.refitHost.size() != count) st.refitHost.assign(count, RefitInstance {});
    if (!st.refitInst.ptr || st.refitInst.bytes < std::max<size_t>(16, count * sizeof(RefitInstance))) ARK_HIP(st.refitInst.alloc(std::max<size_t>(16, count * sizeof(RefitInstance))));
    for (uint32_t ii = 0; ii < count; ++ii) {
        const float* M = instances[ii].object_to_world;
        const float det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
        const ArkRTTriangleMesh& mesh = st.meshHost[instances[ii].rt_mesh_index];
        RefitInstance& q = st.refitHost[ii];
        const bool moved = allDirty || std::memcmp((*have)[ii].data(), M, sizeof(q.m)) != 0;
        std::memcpy(q.m, M, sizeof(q.m));
        q.first_vertex = mesh.first_vertex;
        q.first_index = static_cast<uint32_t>(mesh.first_index);
        q.flip = det < 0.0f ? 1u : 0u;
        q.dirty = moved ? 1u : 0u;
    }
    ARK_HIP(stagedUpload(st, st.refitInst.ptr, st.refitHost.data(), count * sizeof(RefitInstance), s));
    return ARK_DDGI_OK;
}

// A BVH of the scene was replaced (an install): its node masks are recomputed and the
// next refit reaches every node.
void markTopologyChanged(SceneStore& st)
{
    st.world.masksValid = false;
    st.sun.masksValid = false;
    st.refitFull = true;
}

// The spare geometry copies retired behind everything enqueued on `s` so far.
hipError_t dropSpares(SceneStore& st, hipStream_t s)
{
    hipError_t e = hipSuccess;
    for (SceneStore::Spare& c : st.spare) {
        for (DeviceBuffer* b : { &c.world, &c.sun, &c.instances })
            if (e == hipSuccess) e = retireBuffer(st, *b, s);
        c.valid = false;
    }
    return e;
}

// An install replaced a BVH of the front copy (a new topology, refitted forward on `s`):
// the back copy is dropped - retired behind everything enqueued so far - and copied anew
// from the front one by the next refit, which waits for the install (evInstalled).
hipError_t installedGeometry(ArkDdgiCtx* ctx, SceneStore& st, hipStream_t s)
{
    hipError_t e = dropSpares(st, s);
    markTopologyChanged(st); // (again: the boxes scratch is of the old topology without a forward refit)
    std::vector<std::array<float, 12>>& xf = st.xf[st.front];
    xf.resize(st.instHost.size());
    for (size_t i = 0; i < st.instHost.size(); ++i) std::memcpy(xf[i].data(), st.instHost[i].object_to_world, sizeof(float) * 12);
    if (e == hipSuccess) e = hipEventRecord(ctx->evInstalled, s);
    ctx->installValid = e == hipSuccess;
    return e;
}

// Background builds' host-thread inputs: a snapshot of the world records on `s` behind
// every refit enqueued so far (the refits run on the callers' streams; a thread reading
// the live records could see a half-refitted set).
hipError_t snapshotRecords(SceneStore& st, DeviceBuffer& snap, hipEvent_t& ev, hipStream_t s)
{
    const size_t bytes = st.world.records * sizeof(GpuTriangle);
    hipError_t e = snap.alloc(std::max<size_t>(bytes, 16));
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(snap.ptr, st.world.tris(st.world.buf), bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && !ev) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, s);
    return e;
}

// The sun rebuild's thread: the snapshot of the world records, the light-space BVH of
// job->dir on the host (as set_scene builds it), uploaded into job->bvh.
void runSunJob(SunJob* job, int device, uint64_t count, int threads)
{
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = hipSetDevice(device) == hipSuccess;
    hipStream_t s = nullptr;
    ok = ok && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventSynchronize(job->evSnap) == hipSuccess;
    std::vector<GpuTriangle> rec(ok ? count : 0);
    ok = ok && hipMemcpyAsync(rec.data(), job->snap.ptr, count * sizeof(GpuTriangle), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    Bvh8BuildResult r;
    if (ok) {
        SunBvhInput in;
        sun_frame(job->dir, in.frame);
        sun_add_records(in, rec, threads);
        std::vector<GpuTriangle>().swap(rec);
        BvhBuildOptions opt;
        opt.threads = threads;
        Bvh8CollapseOptions copt;
        copt.threads = threads;
        ok = build_sun_bvh(in, opt, copt, r) && !r.nodes.empty();
        std::memcpy(job->frame, in.frame, sizeof(job->frame));
        job->bvh.inflateAbs = in.inflateAbs;
        job->bvh.depth = r.max_depth;
        const int32_t root = 0;
        ok = ok && bvhLevelOrder(r.nodes.data(), r.nodes.size(), &root, 1, job->levelOrder, job->bvh.levelOffsets);
    }
    ok = ok && uploadBvh(r.nodes, r.tris, s, job->bvh) == hipSuccess;
    if (s) (void)hipStreamDestroy(s);
    job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    job->ok = ok;
    job->done.store(true, std::memory_order_release);
}

// The world rebuild's thread: the three classes' BVHs from the snapshot's records (their
// vertices v0, v0 + e1, v0 + e2; each leaf record then replaced by its source record,
// bit for bit), the record order's source indices and the refit's level order.
void runWorldJob(WorldJob* job, int device, int threads)
{
    const auto t0 = job->gpuFallback ? job->t0 : std::chrono::steady_clock::now();
    bool ok = hipSetDevice(device) == hipSuccess;
    hipStream_t s = nullptr;
    ok = ok && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventSynchronize(job->evSnap) == hipSuccess;
    std::vector<GpuTriangle> rec(ok ? job->snapRecords : 0);
    ok = ok && hipMemcpyAsync(rec.data(), job->snap.ptr, rec.size() * sizeof(GpuTriangle), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) job->error = "snapshot download failed";
    std::vector<BuildTriangle> cls[3];
    if (ok) {
        for (size_t i = 0; i < rec.size(); ++i) {
            const GpuTriangle& g = rec[i];
            if (isHoleTriangle(g)) continue;
            uint32_t inst, flip;
            std::memcpy(&inst, &g.t2[1], 4);
            std::memcpy(&flip, &g.t2[3], 4);
            if (inst >= job->classOf.size()) {
                ok = false;
                job->error = "record of an unknown instance";
                break;
            }
            BuildTriangle t;
            const float e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
            for (int a = 0; a < 3; ++a) {
                t.v0[a] = g.t0[a];
                t.v1[a] = g.t0[a] + e1[a];
                t.v2[a] = g.t0[a] + e2[a];
            }
            t.instance = inst;
            t.primitive = static_cast<uint32_t>(i); // the source record (replaced below)
            t.flip_facing = flip;
            cls[job->classOf[inst]].push_back(t);
        }
    }
    WorldBvh8 w;
    std::vector<uint32_t> perm, order;
    if (ok) {
        BvhBuildOptions opt;
        opt.threads = threads;
        Bvh8CollapseOptions copt;
        copt.threads = threads;
        ok = build_world_bvh8(cls, opt, copt, w, job->error);
        if (w.maxLeaf > static_cast<uint32_t>(kBvh8MaxLeafSize)) job->error = "BVH2 leaf over the leaf size";
    }
    if (ok) {
        perm.assign(w.tris.size(), 0xffffffffu);
        for (size_t i = 0; i < w.tris.size(); ++i) {
            GpuTriangle& g = w.tris[i];
            if (isHoleTriangle(g)) continue;
            uint32_t src;
            std::memcpy(&src, &g.t2[2], 4);
            perm[i] = src;
            g = rec[src];
        }
        std::copy(w.roots, w.roots + 3, job->roots);
        job->opaqueNodes = w.opaqueNodes;
        job->maxLeaf = w.maxLeaf;
        job->sah = w.sah;
        job->bvh.depth = w.depth;
        ok = bvhLevelOrder(w.nodes.data(), w.nodes.size(), w.roots, 3, order, job->bvh.levelOffsets);
    }
    if (ok) {
        ok = DeviceBvh::bytesFor(w.nodes.size(), w.tris.size()) < (1ull << 32) && job->perm.alloc(std::max<size_t>(16, perm.size() * 4)) == hipSuccess &&
             job->bvh.order.alloc(std::max<size_t>(16, order.size() * 4)) == hipSuccess &&
             hipMemcpyAsync(job->perm.ptr, perm.data(), perm.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
             hipMemcpyAsync(job->bvh.order.ptr, order.data(), order.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess && uploadBvh(w.nodes, w.tris, s, job->bvh) == hipSuccess;
        if (!ok && job->error.empty()) job->error = "upload failed";
    }
    if (s) (void)hipStreamDestroy(s);
    job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    job->ok = ok;
    job->done.store(true, std::memory_order_release);
}

// The deepest BVH8 the device build installs. The traversal's spill area is sized from the
// installed depth (ensureSpill: depth + 2 - kStackLds entries per lane, DeviceBvh::depth),
// and the deepest tree the host builds hand it is bounded by the BVH2 builder's depth cap
// (BvhBuildOptions::max_depth, 60); a radix tree over coincident centroids can be
// deeper, and such a scene is left to the host build.
constexpr uint32_t kGpuBuildMaxDepth = 60;

// Errors after which the device is not used again by the job (no host fallback)
bool isDeviceFault(hipError_t e)
{
    return e == hipErrorIllegalAddress || e == hipErrorLaunchFailure || e == hipErrorLaunchTimeOut || e == hipErrorECCNotCorrectable || e == hipErrorAssert ||
           e == hipErrorNoDevice || e == hipErrorInvalidDevice;
}

// The device build of runWorldJobGpu on `s`: hipSuccess and `why` empty when job holds the
// result; `why` set when the host has to build this scene.
hipError_t buildWorldGpu(WorldJob* job, hipStream_t s, std::string& why)
{
    // Scratch in two allocations (one sized from the snapshot, one from the count of
    // triangles read back): a free waits for the device's streams, frames in flight included
    struct Arena {
        DeviceBuffer buf;
        size_t used = 0;
        static size_t pad(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }
        DeviceBuffer take(size_t n)
        {
            DeviceBuffer b;
            b.ptr = static_cast<char*>(buf.ptr) + used;
            b.bytes = n;
            used += pad(n);
            return b; // a view: never released
        }
        ~Arena() { buf.release(); }
    } arenaA, arenaB;
    struct {
        DeviceBuffer classOf, hdr, idx, idxSorted, keys, keysSorted, sortTemp, split, position, items[2], nodes, counters, masks, inst, boxes;
    } w;
    hipError_t e = hipSuccess;
#define ARK_GB(expr)                          \
    do {                                      \
        if ((e = (expr)) != hipSuccess) return e; \
    } while (0)
    if (job->snapRecords == 0 || job->snapRecords > 0x7fffffffull || job->classOf.empty()) {
        why = "no records";
        return hipSuccess;
    }
    const uint32_t records = static_cast<uint32_t>(job->snapRecords), instances = static_cast<uint32_t>(job->classOf.size());
    const GpuTriangle* snap = job->snap.as<GpuTriangle>();
    std::vector<uint32_t> classHost(job->classOf.begin(), job->classOf.end());
    ARK_GB(arenaA.buf.alloc(Arena::pad(instances * 4ull) + Arena::pad(sizeof(LbvhHeader)) + Arena::pad(records * 4ull) + Arena::pad(records * 8ull)));
    w.classOf = arenaA.take(instances * 4ull);
    w.hdr = arenaA.take(sizeof(LbvhHeader));
    w.idx = arenaA.take(records * 4ull);
    w.keys = arenaA.take(records * 8ull);
    ARK_GB(hipMemcpyAsync(w.classOf.ptr, classHost.data(), instances * 4ull, hipMemcpyHostToDevice, s));
    ARK_GB(hipStreamWaitEvent(s, job->evSnap, 0));
    ARK_GB(launch_lbvh_prims(snap, records, w.classOf.as<uint32_t>(), instances, w.idx.as<uint32_t>(), w.keys.as<uint64_t>(), w.hdr.as<LbvhHeader>(), s));
    LbvhHeader hdr {};
    ARK_GB(hipMemcpyAsync(&hdr, w.hdr.ptr, sizeof(hdr), hipMemcpyDeviceToHost, s));
    ARK_GB(hipStreamSynchronize(s));
    if (hdr.error || hdr.prims == 0 || hdr.prims > records || hdr.classCount[0] + hdr.classCount[1] + hdr.classCount[2] != hdr.prims) {
        why = hdr.error ? "record of an unknown instance" : "no triangles";
        return hipSuccess;
    }
    const uint32_t n = hdr.prims;
    // sort the (key, record index) pairs
    size_t tempBytes = 0;
    ARK_GB(launch_lbvh_sort(nullptr, tempBytes, w.keys.as<uint64_t>(), nullptr, w.idx.as<uint32_t>(), nullptr, n, s));
    // (the collapse's bound on the nodes: below)
    const uint32_t nodeCap = n / 2u + 8u;
    {
        const size_t sizes[] = { tempBytes, n * 8ull, n * 4ull, n * 4ull, nodeCap * sizeof(GpuBvh8Node), nodeCap * sizeof(lbvh::Member), nodeCap * sizeof(lbvh::Member),
                                 n * 4ull, kLbvhCounters * 4ull, nodeCap * 8ull, instances * sizeof(RefitInstance), nodeCap * 6ull * sizeof(float) };
        size_t total = 0;
        for (size_t b : sizes) total += Arena::pad(b);
        ARK_GB(arenaB.buf.alloc(total));
        w.sortTemp = arenaB.take(sizes[0]);
        w.keysSorted = arenaB.take(sizes[1]);
        w.idxSorted = arenaB.take(sizes[2]);
        w.split = arenaB.take(sizes[3]);
        w.nodes = arenaB.take(sizes[4]);
        w.items[0] = arenaB.take(sizes[5]);
        w.items[1] = arenaB.take(sizes[6]);
        w.position = arenaB.take(sizes[7]);
        w.counters = arenaB.take(sizes[8]);
        w.masks = arenaB.take(sizes[9]);
        w.inst = arenaB.take(sizes[10]);
        w.boxes = arenaB.take(sizes[11]);
    }
    ARK_GB(launch_lbvh_sort(w.sortTemp.ptr, tempBytes, w.keys.as<uint64_t>(), w.keysSorted.as<uint64_t>(), w.idx.as<uint32_t>(), w.idxSorted.as<uint32_t>(), n, s));
    // the radix trees, class by class
    uint32_t classLo[3], first = 0;
    for (int c = 0; c < 3; ++c) {
        classLo[c] = first;
        first += hdr.classCount[c];
        ARK_GB(launch_lbvh_hierarchy(w.keysSorted.as<uint64_t>(), classLo[c], classLo[c] + hdr.classCount[c], w.split.as<uint32_t>(), s));
    }
    // the collapse. Every BVH8 node but a class's root is a BVH2 node of at least 4
    // triangles, and one with an internal child has 8 members. With L nodes without an
    // internal child (4 triangles of their own each), C with one (7 members of their
    // own) and fewer than L with more, 4 L + 7 C <= n bounds 2 L + C by n / 2: fewer than
    // n / 2 + 3 nodes (the kernel checks, and the job falls back beyond).
    ARK_GB(hipMemsetAsync(w.counters.ptr, 0, kLbvhCounters * 4, s));
    float lo[3], hi[3];
    LbvhCollapseArgs a {};
    for (int k = 0; k < 3; ++k) {
        lo[k] = lbvhOrderedFloat(hdr.lo[k]);
        hi[k] = lbvhOrderedFloat(hdr.hi[k]);
        a.extent[k] = hi[k] - lo[k];
    }
    a.keys = w.keysSorted.as<uint64_t>();
    a.split = w.split.as<uint32_t>();
    a.nodes = w.nodes.as<GpuBvh8Node>();
    a.position = w.position.as<uint32_t>();
    a.counters = w.counters.as<uint32_t>();
    a.criterion = lbvh::kDefaultCriterion;
    std::vector<std::array<uint32_t, 3>> levels; // node counts [depth][class]
    uint32_t nodeTotal = 0, counters[kLbvhCounters] = {};
    for (int c = 0; c < 3; ++c) {
        if (!hdr.classCount[c]) continue;
        job->roots[c] = static_cast<int32_t>(nodeTotal);
        a.items = nullptr;
        a.root.r.first = classLo[c];
        a.root.r.last = classLo[c] + hdr.classCount[c] - 1u;
        a.root.node = classLo[c];
        a.count = 1;
        a.levelBase = nodeTotal;
        int pong = 0;
        for (uint32_t depth = 0; a.count; ++depth) {
            if (depth >= kGpuBuildMaxDepth || a.levelBase + a.count > nodeCap) {
                why = depth >= kGpuBuildMaxDepth ? "BVH8 deeper than the device build installs" : "more nodes than the device build's scratch";
                return hipSuccess;
            }
            a.nextBase = a.levelBase + a.count;
            a.nextCapacity = nodeCap - a.nextBase;
            a.next = w.items[pong].as<lbvh::Member>();
            ARK_GB(hipMemsetAsync(w.counters.as<uint32_t>() + kLbvhNextCount, 0, 4, s));
            ARK_GB(launch_lbvh_collapse(a, s));
            // the level's count, before the next level is launched
            ARK_GB(hipMemcpyAsync(counters, w.counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, s));
            ARK_GB(hipStreamSynchronize(s));
            if (counters[kLbvhOverflow]) {
                why = "more nodes than the device build's scratch";
                return hipSuccess;
            }
            if (levels.size() <= depth) levels.push_back({ 0u, 0u, 0u });
            levels[depth][c] = a.count;
            a.items = a.next;
            a.levelBase = a.nextBase;
            a.count = counters[kLbvhNextCount];
            pong ^= 1;
        }
        nodeTotal = a.levelBase;
        if (c == 0) job->opaqueNodes = nodeTotal;
    }
    const uint32_t outRecords = counters[kLbvhRecords];
    if (!(DeviceBvh::bytesFor(nodeTotal, outRecords) < (1ull << 32))) {
        why = "nodes and records of 4 GiB or more";
        return hipSuccess;
    }
    // the installed buffers, sized from the counts read back
    DeviceBvh& b = job->bvh;
    b.triOffset = DeviceBvh::triOffsetFor(nodeTotal);
    ARK_GB(b.buf.alloc(DeviceBvh::bytesFor(nodeTotal, outRecords)));
    ARK_GB(job->perm.alloc(std::max<size_t>(16, outRecords * 4ull)));
    GpuBvh8Node* nodes = b.nodes(b.buf);
    GpuTriangle* tris = b.tris(b.buf);
    ARK_GB(hipMemcpyAsync(nodes, w.nodes.ptr, nodeTotal * sizeof(GpuBvh8Node), hipMemcpyDeviceToDevice, s));
    ARK_GB(launch_lbvh_scatter(snap, w.idxSorted.as<uint32_t>(), w.position.as<uint32_t>(), tris, job->perm.as<uint32_t>(), n, outRecords, s));
    // the refit's level order from the level counts (bvhLevelOrder's format: deepest level
    // first, ascending node index within a level; each class one breadth-first range)
    std::vector<uint32_t> order;
    order.reserve(nodeTotal);
    b.levelOffsets.assign(1, 0u);
    {
        std::vector<std::array<uint32_t, 3>> base(levels.size());
        uint32_t at[3];
        for (int c = 0; c < 3; ++c) at[c] = job->roots[c] >= 0 ? static_cast<uint32_t>(job->roots[c]) : 0u;
        for (size_t d = 0; d < levels.size(); ++d)
            for (int c = 0; c < 3; ++c) {
                base[d][c] = at[c];
                at[c] += levels[d][c];
            }
        for (size_t d = levels.size(); d-- > 0;) {
            for (int c = 0; c < 3; ++c)
                for (uint32_t k = 0; k < levels[d][c]; ++k) order.push_back(base[d][c] + k);
            b.levelOffsets.push_back(static_cast<uint32_t>(order.size()));
        }
    }
    ARK_GB(b.order.alloc(std::max<size_t>(16, order.size() * 4)));
    ARK_GB(hipMemcpyAsync(b.order.ptr, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
    // boxes, grids and planes: the refit over every level, deepest first, every node live
    // (all mask bits set, no instance dirty: no record is touched), the inflation runWorldJob's
    ARK_GB(hipMemsetAsync(w.masks.ptr, 0xff, nodeTotal * 8ull, s));
    ARK_GB(hipMemsetAsync(w.inst.ptr, 0, instances * sizeof(RefitInstance), s));
    RefitBoxArgs ra {};
    ra.inflate = bvh8_inflation_box(lo, hi);
    ra.light = 0;
    ra.dirty = ~0ull;
    for (size_t l = 0; l + 1 < b.levelOffsets.size(); ++l)
        ARK_GB(launch_refit_nodes(nodes, tris, w.boxes.as<float>(), b.order.as<uint32_t>() + b.levelOffsets[l], b.levelOffsets[l + 1] - b.levelOffsets[l], ra,
                                  w.masks.as<uint64_t>(), w.inst.as<RefitInstance>(), nullptr, nullptr, s));
    ARK_GB(hipStreamSynchronize(s));
#undef ARK_GB
    b.nodeCount = nodeTotal;
    b.records = outRecords;
    b.depth = static_cast<uint32_t>(levels.size());
    job->maxLeaf = std::min<uint32_t>(n, static_cast<uint32_t>(kBvh8MaxLeafSize));
    job->sah = 0.0f; // not evaluated on the device
    return hipSuccess;
}

// The world rebuild's thread with ARK_DDGI_FLAG_GPU_REBUILD: the same inputs and outputs as
// runWorldJob, the three BVHs built on the device (ddgi_bvh_build.hip) on a stream of the
// lowest priority that waits for the snapshot on the device. A scene the device build
// does not take (4 GiB, depth, an error that is not a device fault) is built by
// runWorldJob within this job.
void runWorldJobGpu(WorldJob* job, int device, int threads)
{
    job->t0 = std::chrono::steady_clock::now();
    hipStream_t s = nullptr;
    std::string why;
    hipError_t e = hipSetDevice(device);
    int least = 0, greatest = 0;
    if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least);
    if (e == hipSuccess) e = buildWorldGpu(job, s, why);
    if (s) (void)hipStreamDestroy(s);
    if (e == hipSuccess && why.empty()) {
        job->gpu = true;
        job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - job->t0).count();
        job->ok = true;
        job->done.store(true, std::memory_order_release);
        return;
    }
    if (isDeviceFault(e)) {
        job->error = std::string("device build: ") + hipGetErrorString(e);
        job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - job->t0).count();
        job->ok = false;
        job->done.store(true, std::memory_order_release);
        return;
    }
    // the host build from the same snapshot
    job->bvh.release();
    job->bvh = DeviceBvh {};
    job->perm.release();
    job->roots[0] = job->roots[1] = job->roots[2] = -1;
    job->opaqueNodes = 0;
    job->gpuFallback = true;
    runWorldJob(job, device, threads);
}

// Frames in flight may read what an install replaces: a shared scene waits for the
// device (every context's work); otherwise the caller's stream `s` waits for the
// context's earlier operations (orderBegin) and the old buffers are retired behind it.
hipError_t installBarrier(ArkDdgiCtx* ctx, hipStream_t s)
{
    if (ctx->sceneStore.use_count() > 1) return hipDeviceSynchronize();
    return orderBegin(ctx, s);
}

// The end of a refit or an install on `s`: with a shared scene the other contexts'
// next traversals do not wait for this context's streams, so the work completes here.
hipError_t installDone(ArkDdgiCtx* ctx, hipStream_t s)
{
    if (ctx->sceneStore.use_count() > 1) return hipStreamSynchronize(s);
    return hipSuccess;
}

// instance -> hit-mask class (the world rebuild's input, the world BVH check)
std::vector<int> instanceClasses(const SceneStore& st)
{
    std::vector<int> c(st.instHost.size());
    for (size_t i = 0; i < c.size(); ++i) c[i] = hit_mask_class(st.instHost[i].hit_mask);
    return c;
}

// The kernels' view of the front copies (set_scene, the installs, rotateGeometry)
void setWorldArgs(SceneStore& st)
{
    st.args.nodes = st.world.nodes(st.world.buf);
    st.args.tris = st.world.tris(st.world.buf);
    st.args.tri_byte_offset = static_cast<uint32_t>(st.world.triOffset);
    st.args.instances = st.instances.as<GpuInstance>();
}

void setWorldRoots(SceneStore& st, const int32_t roots[3], uint32_t opaqueNodes)
{
    st.args.root_opaque = roots[0];
    st.args.root_masked = roots[1];
    st.args.root_blend = roots[2];
    st.args.opaque_nodes = opaqueNodes;
}

void setSunArgs(SceneStore& st)
{
    st.sunArgs.sun_nodes = st.sun.nodes(st.sun.buf);
    st.sunArgs.sun_tris = st.sun.tris(st.sun.buf);
    st.sunArgs.sun_root = 0;
}

// The refit's boxes scratch of `b` for its node count, with a quarter to spare (a smaller
// one retired behind `s`)
hipError_t growBoxes(SceneStore& st, DeviceBvh& b, hipStream_t s)
{
    const size_t need = b.nodeCount * 6 * sizeof(float);
    if (b.boxes.bytes >= need) return hipSuccess;
    const hipError_t e = retireBuffer(st, b.boxes, s);
    return e == hipSuccess ? b.boxes.alloc(std::max<size_t>(16, need * 5 / 4)) : e;
}

// A finished build `b` (buffer, level order, counts) replaces `cur`: the old buffer and
// level order retired behind everything enqueued on `s` so far, the refit's scratch kept
// (growBoxes follows).
hipError_t replaceBvh(SceneStore& st, DeviceBvh& cur, DeviceBvh& b, hipStream_t s)
{
    hipError_t e = retireBuffer(st, cur.buf, s);
    if (e == hipSuccess) e = retireBuffer(st, cur.order, s);
    if (e != hipSuccess) return e;
    b.boxes = cur.boxes;
    b.masks = cur.masks;
    b.masksValid = false;
    cur = std::move(b);
    b = DeviceBvh {};
    return hipSuccess;
}

// The light-space BVH `b` (its level order on the host) built for the sun direction `dir`
// in `frame` becomes the scene's: uploaded by the job (sunCollect: host null), or here from
// `host` (set_scene, synchronously).
int installSunBvh(ArkDdgiCtx* ctx, SceneStore& st, DeviceBvh& b, Bvh8BuildResult* host, const std::vector<uint32_t>& levelOrder, const double* frame, const float* dir,
                  hipStream_t s)
{
    ARK_HIP(replaceBvh(st, st.sun, b, s));
    ARK_HIP(st.sun.order.alloc(std::max<size_t>(16, levelOrder.size() * 4)));
    ARK_HIP(hipMemcpy(st.sun.order.ptr, levelOrder.data(), levelOrder.size() * 4, hipMemcpyHostToDevice));
    st.sun.nodeCount = levelOrder.size();
    ARK_HIP(growBoxes(st, st.sun, s));
    if (host) ARK_HIP(uploadBvh(host->nodes, host->tris, nullptr, st.sun));
    setSunArgs(st);
    for (int k = 0; k < 9; ++k) {
        st.sunArgs.sun_frame[k] = static_cast<float>(frame[k]);
        st.sunFrameD[k] = frame[k];
    }
    std::memcpy(st.sunDirBuilt, dir, sizeof(st.sunDirBuilt));
    return ARK_DDGI_OK;
}

// The end of an install on `s` (sunCollect, worldCollect): the new topology refitted
// forward when refits came in while it was built (every instance re-transformed), the
// spares dropped, the next traversal and refit ordered behind it, the scene's version bumped.
int finishInstall(ArkDdgiCtx* ctx, SceneStore& st, uint32_t refitsSince, hipStream_t s)
{
    markTopologyChanged(st);
    if (refitsSince) {
        if (const int rc = uploadRefitInstances(ctx, st, st.instHost.data(), static_cast<uint32_t>(st.instHost.size()), nullptr, s)) return rc;
        if (const int rc = enqueueRefit(ctx, st, s, st.world.buf, st.sun.buf, st.front)) return rc;
    }
    ARK_HIP(installedGeometry(ctx, st, s));
    ARK_HIP(hipEventRecord(ctx->evRefit, s));
    ARK_HIP(installDone(ctx, s));
    ctx->refitPending = true;
    ++st.version;
    return refreshScene(ctx);
}

// The light-space sun BVH follows the context's sun (called by every update and by
// set_lights / set_instances, on the stream `s` of the call): a finished rebuild for
// this context's sun is installed - stream-ordered behind the frames that may read the
// old one, and refitted forward when refits came in between - and a new one is started
// when the scene chose the light-space BVH at set_scene but holds none for this
// direction. Until it is installed the sun's shadow rays traverse the world BVHs
// (deriveSceneArgs), with the same results. sunCollect: the request streak and a
// finished rebuild; sunStartKind / sunStart: a new one.
int sunCollect(ArkDdgiCtx* ctx, hipStream_t s)
{
    SceneStore& st = *ctx->sceneStore;
    auto sameDir = [](const float* a, const float* b) { return std::memcmp(a, b, 3 * sizeof(float)) == 0; };
    if (ctx->hasSun) {
        if (st.sunReqStreak && sameDir(st.sunReqDir, ctx->sunDir)) {
            st.sunReqStreak = std::min<uint32_t>(st.sunReqStreak + 1u, 1u << 30);
        } else {
            std::memcpy(st.sunReqDir, ctx->sunDir, sizeof(st.sunReqDir));
            st.sunReqStreak = 1;
        }
    }
    if (st.sunJob && st.sunJob->done.load(std::memory_order_acquire)) {
        SunJob& j = *st.sunJob;
        if (!j.ok) {
            // remembered: not started again for this direction and scene version
            st.sunFailed = true;
            std::memcpy(st.sunFailedDir, j.dir, sizeof(j.dir));
            st.sunFailedVersion = j.version;
            st.bvhStats.sun_rebuild_failures = ++st.sunFailures;
            j.t.join();
            st.sunJob.reset();
        } else if (st.sunReqStreak >= 2 && !sameDir(j.dir, st.sunReqDir)) {
            // stale: the scene's contexts settled on another sun
            j.t.join();
            st.sunJob.reset();
        } else if (ctx->hasSun && sameDir(j.dir, ctx->sunDir)) {
            std::unique_ptr<SunJob> job = std::move(st.sunJob);
            job->t.join();
            ARK_HIP(installBarrier(ctx, s));
            if (const int rc = installSunBvh(ctx, st, job->bvh, nullptr, job->levelOrder, job->frame, job->dir, s)) return rc;
            ARK_HIP(retireBuffer(st, job->snap, s));
            st.bvhMaxDepth = std::max(st.bvhMaxDepth, st.sun.depth);
            st.bvhStats.max_depth = st.bvhMaxDepth;
            st.bvhStats.sun_node_count = st.sun.nodeCount;
            st.bvhStats.sun_max_depth = st.sun.depth;
            st.bvhStats.sun_rebuilds = ++st.sunRebuilds;
            st.bvhStats.sun_build_ms = job->ms;
            st.sunRefitsSinceBuild = st.refitCount - job->refitsAt;
            st.bvhStats.sun_built_refit_version = job->refitsAt;
            // (refits that came in while it was built: its records follow them)
            if (const int rc = finishInstall(ctx, st, st.sunRefitsSinceBuild, s)) return rc;
        }
        // else: built for another context's sun; that context installs it
    }
    return ARK_DDGI_OK;
}

// The sun rebuild this context's sun asks for: kSunNone; kSunMissing when the scene holds
// no light-space BVH for it (started at once, even beside a world rebuild); kSunLoosened
// when the installed one was built for it and refits have loosened it since (a
// background rebuild like the world BVHs', one at a time with them, not with
// ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD). Only on a stable request, and not again after a
// failure for the same direction and scene version.
enum SunStart { kSunNone, kSunLoosened, kSunMissing };
SunStart sunStartKind(const ArkDdgiCtx* ctx)
{
    const SceneStore& st = *ctx->sceneStore;
    auto sameDir = [](const float* a, const float* b) { return std::memcmp(a, b, 3 * sizeof(float)) == 0; };
    if (!st.sunWanted || !ctx->hasSun || st.sunJob || st.sunReqStreak < 2 || !sameDir(st.sunReqDir, ctx->sunDir)) return kSunNone;
    if (st.sunFailed && st.sunFailedVersion == st.version && sameDir(st.sunFailedDir, ctx->sunDir)) return kSunNone;
    if (st.sunArgs.sun_root >= 0 && sameDir(ctx->sunDir, st.sunDirBuilt))
        return (st.sunRefitsSinceBuild == 0 || (ctx->desc.flags & ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD)) ? kSunNone : kSunLoosened;
    return kSunMissing;
}

// A world rebuild is wanted while refits have loosened the installed BVHs (and none
// failed, and background rebuilds are on).
bool worldStartWanted(const ArkDdgiCtx* ctx)
{
    const SceneStore& st = *ctx->sceneStore;
    return !st.worldJob && st.refitsSinceBuild != 0 && !st.worldRebuildFailed && !(ctx->desc.flags & ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD);
}

// The settle rebuild of ARK_DDGI_FLAG_GPU_REBUILD: the installed world BVHs are a device
// build and no refit has arrived since their snapshot - the motion has stopped - so one
// host rebuild replaces the LBVH with the SAH tree a static scene traces faster.
bool worldSettleWanted(const ArkDdgiCtx* ctx)
{
    const SceneStore& st = *ctx->sceneStore;
    const uint32_t f = ctx->desc.flags;
    return (f & ARK_DDGI_FLAG_GPU_REBUILD) && !(f & ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD) && st.worldGpuBuilt && !st.worldJob && st.refitsSinceBuild == 0 &&
           !st.worldRebuildFailed;
}

int sunStart(ArkDdgiCtx* ctx, hipStream_t s)
{
    SceneStore& st = *ctx->sceneStore;
    auto job = std::make_unique<SunJob>();
    std::memcpy(job->dir, ctx->sunDir, sizeof(job->dir));
    job->version = st.version;
    job->refitsAt = st.refitCount;
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(snapshotRecords(st, job->snap, job->evSnap, s));
    job->t = std::thread(runSunJob, job.get(), st.device, st.world.records, std::max(1, st.buildThreads / 2));
    st.sunJob = std::move(job);
    st.lastBackground = SceneStore::kBackgroundSun;
    return ARK_DDGI_OK;
}

// A loosened BVH's rebuild starts when no other background build runs; when both the
// world BVHs and the light-space one are loosened they take turns (under continuous
// motion each would otherwise start again the moment its last one is installed).
bool loosenedTurn(const SceneStore& st, uint8_t mine, bool otherWanted)
{
    if (st.worldJob || st.sunJob) return false;
    return !otherWanted || st.lastBackground != mine;
}

// sunCollect, then a sun rebuild to start (set_lights: the world BVHs' rebuilds are
// left to the next update or set_instances)
int sunRebuildStep(ArkDdgiCtx* ctx, hipStream_t s)
{
    if (const int rc = sunCollect(ctx, s)) return rc;
    const SunStart k = sunStartKind(ctx);
    if (k == kSunMissing || (k == kSunLoosened && loosenedTurn(*ctx->sceneStore, SceneStore::kBackgroundSun, worldStartWanted(ctx))))
        return sunStart(ctx, s);
    return ARK_DDGI_OK;
}

// The world BVHs' background rebuild after refits (the reference's full TLAS build every
// 60 frames restores tightness, GpuScene.cpp:998-1010; a refit keeps the old topology,
// whose boxes loosen as instances move): a finished rebuild is installed on `s` -
// behind the frames that may read the old BVHs, its shading records gathered into its
// record order, and refitted forward when refits came in while it was built - and,
// while refits have loosened the installed one, a new one is started (worldStart).
int worldCollect(ArkDdgiCtx* ctx, hipStream_t s)
{
    SceneStore& st = *ctx->sceneStore;
    if (st.worldJob && st.worldJob->done.load(std::memory_order_acquire)) {
        std::unique_ptr<WorldJob> job = std::move(st.worldJob);
        job->t.join();
        if (job->gpuFallback) st.bvhStats.bvh_gpu_fallbacks++;
        if (!job->ok) {
            // the refitted BVHs stay (results do not depend on the tree); no more
            // background rebuilds of this scene (a set_scene builds anew), reported in
            // the stats and last_error, the update goes on
            st.worldRebuildFailed = true;
            st.bvhStats.bvh_rebuild_failures++;
            ctx->lastError = "background BVH rebuild failed: " + job->error;
            return ARK_DDGI_OK;
        }
        ARK_HIP(installBarrier(ctx, s));
        // the shading records in the new record order (before the old ones are retired)
        DeviceBuffer tn;
        ARK_HIP(tn.alloc(std::max<size_t>(64, job->bvh.records * 64)));
        ARK_HIP(launch_gather_records(tn.as<float4>(), st.triNormals.as<float4>(), job->perm.as<uint32_t>(), job->bvh.records, s));
        ARK_HIP(retireBuffer(st, st.triNormals, s));
        st.triNormals = tn;
        job->bvh.inflateAbs = st.world.inflateAbs; // the refits' floor stays set_scene's
        ARK_HIP(replaceBvh(st, st.world, job->bvh, s));
        ARK_HIP(retireBuffer(st, job->perm, s));
        ARK_HIP(retireBuffer(st, job->snap, s));
        ARK_HIP(growBoxes(st, st.world, s));
        setWorldArgs(st);
        setWorldRoots(st, job->roots, job->opaqueNodes);
        st.args.tri_normals = st.triNormals.as<float4>();
        st.bvhMaxDepth = std::max(st.world.depth, st.sunArgs.sun_root >= 0 ? st.sun.depth : 0u);
        st.bvhStats.node_count = st.world.nodeCount;
        st.bvhStats.max_depth = st.bvhMaxDepth;
        st.bvhStats.max_leaf_size = job->maxLeaf;
        st.bvhStats.sah_cost = job->sah;
        st.bvhStats.node_bytes = st.world.nodeCount * sizeof(GpuBvh8Node);
        st.bvhStats.triangle_bytes = st.world.records * sizeof(GpuTriangle);
        st.bvhStats.bvh_rebuilds = ++st.worldRebuilds;
        st.bvhStats.bvh_rebuild_ms = job->ms;
        st.worldGpuBuilt = job->gpu;
        st.bvhStats.bvh_installed_builder = job->gpu ? 1u : 0u;
        if (job->gpu) st.bvhStats.bvh_gpu_rebuilds++;
        st.refitsSinceBuild = st.refitCount - job->refitsAt; // refits since its snapshot
        st.bvhStats.bvh_built_refit_version = job->refitsAt;
        return finishInstall(ctx, st, st.refitsSinceBuild, s);
    }
    return ARK_DDGI_OK;
}

int worldStart(ArkDdgiCtx* ctx, hipStream_t s, bool gpu)
{
    SceneStore& st = *ctx->sceneStore;
    auto job = std::make_unique<WorldJob>();
    job->version = st.version;
    job->refitsAt = st.refitCount;
    job->snapRecords = st.world.records;
    job->classOf = instanceClasses(st);
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(snapshotRecords(st, job->snap, job->evSnap, s));
    // half the host threads: the other half stays with the frames being enqueued meanwhile
    job->t = std::thread(gpu ? runWorldJobGpu : runWorldJob, job.get(), st.device, std::max(1, st.buildThreads / 2));
    st.worldJob = std::move(job);
    st.lastBackground = SceneStore::kBackgroundWorld;
    st.refitsSinceBuild = 0;
    return ARK_DDGI_OK;
}

// Everything an operation on `s` does to the scene first: buffers retired by earlier
// installs freed, finished rebuilds installed, new ones started.
int sceneMaintenance(ArkDdgiCtx* ctx, hipStream_t s)
{
    collectRetired(*ctx->sceneStore);
    if (const int rc = worldCollect(ctx, s)) return rc;
    if (const int rc = sunCollect(ctx, s)) return rc;
    const SunStart k = sunStartKind(ctx);
    if (k == kSunMissing) {
        if (const int rc = sunStart(ctx, s)) return rc;
    }
    // loosened world BVHs: the device build with ARK_DDGI_FLAG_GPU_REBUILD; settled ones it built: the host's
    const bool loosened = worldStartWanted(ctx), world = loosened || worldSettleWanted(ctx), sun = k == kSunLoosened;
    if (world && loosenedTurn(*ctx->sceneStore, SceneStore::kBackgroundWorld, sun))
        return worldStart(ctx, s, loosened && (ctx->desc.flags & ARK_DDGI_FLAG_GPU_REBUILD));
    if (sun && loosenedTurn(*ctx->sceneStore, SceneStore::kBackgroundSun, world)) return sunStart(ctx, s);
    return ARK_DDGI_OK;
}

// Makes `st` the context's scene with the scene's lights: the per-context work sets
// follow its light count and BVH depth.
int adoptScene(ArkDdgiCtx* ctx, std::shared_ptr<SceneStore> st)
{
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
        desc->sun_bvh < ARK_DDGI_SUN_BVH_AUTO || desc->sun_bvh > ARK_DDGI_SUN_BVH_LIGHT_SPACE || (desc->flags & ~(ARK_DDGI_FLAG_SERIAL_FRAMES | ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD | ARK_DDGI_FLAG_GPU_REBUILD)) ||
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
    if ((e = hipEventCreateWithFlags(&ctx->evRefit, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&ctx->evInstalled, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    for (auto& ev : ctx->evFree)
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    {
        // the refit stream at the device's highest priority: its per-level launches are
        // dispatched ahead of the frame in flight's work when both wait for a CU
        int lo = 0, hi = 0;
        if ((e = hipDeviceGetStreamPriorityRange(&lo, &hi)) != hipSuccess) return bad(e, "hipDeviceGetStreamPriorityRange");
        if ((e = hipStreamCreateWithPriority(&ctx->refitStream, hipStreamNonBlocking, hi)) != hipSuccess) return bad(e, "hipStreamCreateWithPriority");
    }
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
    if ((e = ctx->counters.alloc(8 * sizeof(unsigned long long))) != hipSuccess) return bad(e, "alloc counters");
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
                             &ctx->raySteps, &ctx->counters, &ctx->lights, &ctx->bakeTri, &ctx->bakeBary, &ctx->bakeOut, &ctx->bakePixels, &ctx->bakeCounters })
        b->release();
    ctx->sceneStore.reset();
    for (auto& ev : ctx->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->evOrder) (void)hipEventDestroy(ctx->evOrder);
    if (ctx->evTraced) (void)hipEventDestroy(ctx->evTraced);
    if (ctx->evExchangeSrc) (void)hipEventDestroy(ctx->evExchangeSrc);
    if (ctx->evExchangeDone) (void)hipEventDestroy(ctx->evExchangeDone);
    if (ctx->evRefit) (void)hipEventDestroy(ctx->evRefit);
    if (ctx->evInstalled) (void)hipEventDestroy(ctx->evInstalled);
    for (auto& ev : ctx->evFree)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->refitStream) (void)hipStreamDestroy(ctx->refitStream);
    for (auto& ev : ctx->evFrameDone)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->traceStream) (void)hipStreamDestroy(ctx->traceStream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->hostAbort) (void)hipHostFree(ctx->hostAbort);
    delete ctx;
}

const char* ark_ddgi_last_error(const ArkDdgiCtx* ctx) { return ctx ? ctx->lastError.c_str() : "null context"; }

namespace {
// ark_ddgi_set_scene's steps, in the order they run

int validateScene(ArkDdgiCtx* ctx, const ArkDdgiScene* s)
{
    for (uint32_t i = 0; i < s->instance_count; ++i) {
        const ArkRTInstance& inst = s->instances[i];
        if (inst.rt_mesh_index >= s->mesh_count) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u: rt_mesh_index out of range", i);
        const ArkRTTriangleMesh& m = s->meshes[inst.rt_mesh_index];
        if (m.material_index < 0 || static_cast<uint32_t>(m.material_index) >= s->material_count)
            return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "mesh %u: material_index out of range", inst.rt_mesh_index);
        if (static_cast<uint64_t>(m.first_index) + 3ull * inst.triangle_count > s->index_count)
            return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u: indices out of range", i);
    }
    if (s->spot_light_count > ARK_DDGI_MAX_SPOT_LIGHTS || (s->spot_light_count && !s->spot_lights))
        return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "at most %d spot lights (GpuScene.cpp:430)", ARK_DDGI_MAX_SPOT_LIGHTS);
    return ARK_DDGI_OK;
}

// An instance in the shading kernels' table: the rows of its transform, its facing flip
// (det(ObjectToWorld) < 0), hit mask and material
GpuInstance gpuInstance(const ArkRTInstance& inst, const ArkRTTriangleMesh& mesh)
{
    const float* M = inst.object_to_world;
    const float det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
    GpuInstance g;
    std::memset(&g, 0, sizeof(g));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) g.normal_matrix[r * 4 + c] = M[r * 4 + c];
    g.rt_mesh_index = static_cast<int32_t>(inst.rt_mesh_index);
    g.flip_facing = det < 0.0f ? 1 : 0;
    g.hit_mask = static_cast<int32_t>(inst.hit_mask);
    g.material_index = mesh.material_index;
    return g;
}

// World-space triangles per hit-mask class (GpuScene.cpp:883-929: one TLAS instance per
// mesh segment; flattened here into one BVH per class) and the instance table.
int flattenInstances(ArkDdgiCtx* ctx, const ArkDdgiScene* s, std::vector<BuildTriangle> cls[3], std::vector<GpuInstance>& ginst)
{
    ginst.resize(s->instance_count);
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) {
        const ArkRTInstance& inst = s->instances[ii];
        const ArkRTTriangleMesh& m = s->meshes[inst.rt_mesh_index];
        const float* M = inst.object_to_world;
        const GpuInstance& g = ginst[ii] = gpuInstance(inst, m);
        const int c = hit_mask_class(inst.hit_mask);
        for (uint32_t p = 0; p < inst.triangle_count; ++p) {
            BuildTriangle t;
            float* w[3] = { t.v0, t.v1, t.v2 };
            for (int k = 0; k < 3; ++k) {
                const uint32_t idx = s->indices[static_cast<size_t>(m.first_index) + 3u * p + k];
                const uint64_t vi = static_cast<uint64_t>(m.first_vertex) + idx;
                if (vi >= s->vertex_count) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u prim %u: vertex out of range", ii, p);
                const float* P = &s->positions[vi * 3];
                w[k][0] = M[0] * P[0] + M[1] * P[1] + M[2] * P[2] + M[3];
                w[k][1] = M[4] * P[0] + M[5] * P[1] + M[6] * P[2] + M[7];
                w[k][2] = M[8] * P[0] + M[9] * P[1] + M[10] * P[2] + M[11];
            }
            t.instance = ii;
            t.primitive = p;
            t.flip_facing = static_cast<uint32_t>(g.flip_facing);
            cls[c].push_back(t);
        }
    }
    return ARK_DDGI_OK;
}

// textures: decoded to float4 texels (sRGB EOTF per texel), + trailing 1x1 white
int decodeTextures(ArkDdgiCtx* ctx, const ArkDdgiScene* s, std::vector<GpuTextureInfo>& infos, std::vector<float>& texels)
{
    for (uint32_t i = 0; i <= s->texture_count; ++i) {
        GpuTextureInfo ti {};
        ti.texel_offset = texels.size() / 4;
        if (i == s->texture_count) {
            ti.width = ti.height = 1;
            ti.wrap = ARK_WRAP_REPEAT;
            texels.insert(texels.end(), { 1.0f, 1.0f, 1.0f, 1.0f });
        } else {
            const ArkTexture& t = s->textures[i];
            if (t.width <= 0 || t.height <= 0 || !t.data) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u invalid", i);
            ti.width = t.width;
            ti.height = t.height;
            // per-axis wrap, s in bits 0-3 and t in 4-7 (ARK_WRAP_AXES)
            const int ws = (t.wrap & ARK_WRAP_PER_AXIS) ? (t.wrap & 0xf) : t.wrap, wt = (t.wrap & ARK_WRAP_PER_AXIS) ? ((t.wrap >> 4) & 0xf) : t.wrap;
            if (ws < ARK_WRAP_REPEAT || ws > ARK_WRAP_MIRRORED_REPEAT || wt < ARK_WRAP_REPEAT || wt > ARK_WRAP_MIRRORED_REPEAT ||
                ((t.wrap & ARK_WRAP_PER_AXIS) && (t.wrap & ~0x1ff)))
                return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u: unknown wrap mode 0x%x", i, t.wrap);
            ti.wrap = ws | (wt << 4);
            const size_t n = static_cast<size_t>(t.width) * t.height;
            for (size_t p = 0; p < n; ++p)
                for (int c = 0; c < 4; ++c) {
                    float v = 0.0f;
                    switch (t.format) {
                    case ARK_TEX_RGBA8_UNORM: v = static_cast<float>(static_cast<const uint8_t*>(t.data)[p * 4 + c]) / 255.0f; break;
                    case ARK_TEX_RGBA8_SRGB:
                        v = static_cast<float>(static_cast<const uint8_t*>(t.data)[p * 4 + c]) / 255.0f;
                        if (c < 3) v = srgbToLinear(v);
                        break;
                    case ARK_TEX_R32F: v = c == 0 ? static_cast<const float*>(t.data)[p] : (c == 3 ? 1.0f : 0.0f); break;
                    case ARK_TEX_RGBA32F: v = static_cast<const float*>(t.data)[p * 4 + c]; break;
                    default: return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u: unknown format", i);
                    }
                    texels.push_back(v);
                }
        }
        infos.push_back(ti);
    }
    return ARK_DDGI_OK;
}

// every instance's object-space box (refitInflations)
void instanceObjectBoxes(const ArkDdgiScene* s, int threads, std::vector<std::array<float, 6>>& boxes)
{
    boxes.assign(s->instance_count, { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY });
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) {
        const ArkRTInstance& in = s->instances[ii];
        const ArkRTTriangleMesh& mesh = s->meshes[in.rt_mesh_index];
        std::array<float, 6>& box = boxes[ii];
        std::mutex mu;
        parallelFor(static_cast<size_t>(in.triangle_count) * 3u, threads, [&](size_t b, size_t e) {
            float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (size_t k = b; k < e; ++k) {
                const float* P = s->positions + (static_cast<int64_t>(mesh.first_vertex) + s->indices[static_cast<size_t>(mesh.first_index) + k]) * 3;
                for (int a = 0; a < 3; ++a) {
                    lo[a] = std::min(lo[a], P[a]);
                    hi[a] = std::max(hi[a], P[a]);
                }
            }
            std::lock_guard<std::mutex> g(mu);
            for (int a = 0; a < 3; ++a) {
                box[a] = std::min(box[a], lo[a]);
                box[3 + a] = std::max(box[3 + a], hi[a]);
            }
        });
    }
}

// per-triangle shading records (GpuTriangle order, 64 B): the three vertex normals, the
// instance and the three UVs, copied from the vertex pool, so the shading and shadow-ray
// kernels reach a hit's surface in one fetch instead of instance -> mesh -> indices ->
// vertices
void shadingRecords(const ArkDdgiScene* s, const std::vector<GpuTriangle>& tris, int threads, std::vector<float>& tn)
{
    tn.assign(tris.size() * 16, 0.0f);
    parallelFor(tris.size(), threads, [&](size_t b, size_t e) {
        for (size_t t = b; t < e; ++t) {
            if (isHoleTriangle(tris[t])) continue; // never hit: no record
            uint32_t inst, prim;
            std::memcpy(&inst, &tris[t].t2[1], 4);
            std::memcpy(&prim, &tris[t].t2[2], 4);
            const ArkRTTriangleMesh& mesh = s->meshes[s->instances[inst].rt_mesh_index];
            float* o = tn.data() + t * 16;
            for (int q = 0; q < 3; ++q) {
                const uint32_t idx = s->indices[static_cast<size_t>(mesh.first_index) + 3u * prim + q];
                const float* v = reinterpret_cast<const float*>(s->vertices) + (static_cast<size_t>(mesh.first_vertex) + idx) * 9;
                for (int k = 0; k < 3; ++k) o[q * 3 + k] = v[2 + k];
                o[10 + 2 * q] = v[0];
                o[11 + 2 * q] = v[1];
            }
            std::memcpy(o + 9, &inst, 4);
        }
    });
    if (tn.empty()) tn.assign(16, 0.0f);
}
} // namespace

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
    auto st = std::make_shared<SceneStore>();
    st->device = ctx->device;
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    if ((rc = validateScene(ctx, s)) != 0) return rc;
    std::vector<BuildTriangle> cls[3];
    std::vector<GpuInstance> ginst;
    if ((rc = flattenInstances(ctx, s, cls, ginst)) != 0) return rc;
    // host threads for the build (ArkDdgiDesc.build_threads; 0: the box's CPU share per
    // GPU, 16 cores)
    BvhBuildOptions opt;
    opt.threads = ctx->desc.build_threads > 0 ? ctx->desc.build_threads : 16;
    // BVH2 -> BVH8 child selection: SAH-optimal (Ylitie et al. 2017 DP) with the default
    // node / triangle costs (a lower triangle cost and the greedy collapse measured no
    // better)
    Bvh8CollapseOptions copt;
    copt.threads = opt.threads;
    // the sun's light-space BVH input, before the class builds free their triangles; the
    // build itself on its own thread beside the class builds (each build's top levels
    // leave cores idle: C4 setup 13.5 -> s)
    const bool sunBvh = s->has_directional_light && ctx->sunBvh != 0;
    SunBvhInput sunIn;
    Bvh8BuildResult r; // the sun's
    bool sunBuilt = false, sunOk = true;
    float sunBuildMs = 0.0f;
    struct Joiner {
        std::thread t;
        ~Joiner()
        {
            if (t.joinable()) t.join();
        }
    } sunThread;
    if (sunBvh) {
        const auto ts0 = std::chrono::steady_clock::now();
        sun_frame(s->directional_light.world_space_direction, sunIn.frame);
        for (int c = 0; c < 3; ++c) sun_add_triangles(sunIn, cls[c], opt.threads);
        sunBuilt = !sunIn.tris.empty();
        if (sunBuilt)
            sunThread.t = std::thread([&sunIn, &opt, &copt, &r, &sunOk, &sunBuildMs, ts0] {
                sunOk = build_sun_bvh(sunIn, opt, copt, r);
                sunBuildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - ts0).count();
            });
    }
    WorldBvh8 w;
    std::string why;
    if (!build_world_bvh8(cls, opt, copt, w, why)) return ctx->fail(w.tooLarge ? ARK_DDGI_E_UNSUPPORTED : ARK_DDGI_E_DEVICE, "%s", why.c_str());
    std::vector<GpuTextureInfo> infos;
    std::vector<float> texels;
    if ((rc = decodeTextures(ctx, s, infos, texels)) != 0) return rc;
    std::vector<GpuSpotLight> gspots(s->spot_light_count);
    for (uint32_t i = 0; i < s->spot_light_count; ++i) gspots[i] = gpuSpotLight(s->spot_lights[i]);
    // (the traversal's 32-bit byte offset: nodes and records must stay below 4 GiB)
    if (DeviceBvh::bytesFor(w.nodes.size(), w.tris.size()) >= (1ull << 32)) return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "BVH nodes + triangles exceed 4 GiB");
    ARK_HIP(uploadBvh(w.nodes, w.tris, nullptr, st->world));
    st->world.depth = w.depth;
    st->world.inflateAbs = w.inflateAbs;
    if (sunThread.t.joinable()) sunThread.t.join();
    const auto ts0 = std::chrono::steady_clock::now();
    const int32_t sroot = 0;
    if (sunBuilt) {
        if (!sunOk) return ctx->fail(ARK_DDGI_E_DEVICE, "sun BVH2 leaf over %d triangles", kBvh8MaxLeafSize);
        if (!checkBvh8Structure(r.nodes, r.tris, &sroot, 1, why)) return ctx->fail(ARK_DDGI_E_DEVICE, "%s", why.c_str());
        // by cost unless forced: sample sun shadow rays through both structures on the host
        const float* sd = s->directional_light.world_space_direction;
        const float dd = sd[0] * sd[0] + sd[1] * sd[1] + sd[2] * sd[2];
        const float isc = 1.0f / std::sqrt(dd);
        const float L[3] = { -(sd[0] * isc), -(sd[1] * isc), -(sd[2] * isc) };
        std::vector<float> origins;
        sun_sample_origins(w.tris, L, 4096u, origins);
        st->sunCostWorld = static_cast<float>(sun_shadow_cost(w.nodes, w.tris, w.roots, 3, nullptr, L, origins));
        st->sunCostLight = static_cast<float>(sun_shadow_cost(r.nodes, r.tris, &sroot, 1, sunIn.frame, L, origins));
    }
    st->sunArgs.sun_root = -1;
    if (sunBuilt && (ctx->sunBvh == 1 || sun_bvh_pays(st->sunCostWorld, st->sunCostLight))) {
        DeviceBvh sb;
        std::vector<uint32_t> order;
        if (!bvhLevelOrder(r.nodes.data(), r.nodes.size(), &sroot, 1, order, sb.levelOffsets)) return ctx->fail(ARK_DDGI_E_DEVICE, "sun BVH: a node outside it");
        sb.depth = r.max_depth;
        sb.inflateAbs = sunIn.inflateAbs;
        if ((rc = installSunBvh(ctx, *st, sb, &r, order, &sunIn.frame[0][0], s->directional_light.world_space_direction, nullptr)) != 0) return rc;
    }
    sunBuildMs += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - ts0).count();
    std::vector<GpuTriangle>().swap(sunIn.world);
    if ((rc = upload(ctx, st->indices, s->indices, s->index_count)) != 0) return rc;
    if ((rc = upload(ctx, st->vertices, reinterpret_cast<const float*>(s->vertices), s->vertex_count * 9)) != 0) return rc;
    if ((rc = upload(ctx, st->positions, s->positions, s->vertex_count * 3)) != 0) return rc;
    st->instHost.assign(s->instances, s->instances + s->instance_count);
    // the transforms both geometry copies hold (the back one is made at the first refit)
    st->xf[0].resize(s->instance_count);
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) std::memcpy(st->xf[0][ii].data(), s->instances[ii].object_to_world, sizeof(float) * 12);
    st->xf[1] = st->xf[2] = st->xf[0];
    st->spare[0].slot = 1;
    st->spare[1].slot = 2;
    st->meshHost.assign(s->meshes, s->meshes + s->mesh_count);
    instanceObjectBoxes(s, opt.threads, st->instObjBox);
    if ((rc = upload(ctx, st->meshes, s->meshes, s->mesh_count)) != 0) return rc;
    if ((rc = upload(ctx, st->materials, s->materials, s->material_count)) != 0) return rc;
    if ((rc = upload(ctx, st->instances, ginst.data(), ginst.size())) != 0) return rc;
    if ((rc = upload(ctx, st->texInfos, infos.data(), infos.size())) != 0) return rc;
    if ((rc = upload(ctx, st->texels, texels.data(), texels.size())) != 0) return rc;
    {
        std::vector<float> tn;
        shadingRecords(s, w.tris, opt.threads, tn);
        if ((rc = upload(ctx, st->triNormals, tn.data(), tn.size())) != 0) return rc;
    }
    SceneArgs& sc = st->args;
    setWorldArgs(*st);
    setWorldRoots(*st, w.roots, w.opaqueNodes);
    sc.tri_normals = st->triNormals.as<float4>();
    sc.texture_count = static_cast<int32_t>(s->texture_count);
    sc.indices = st->indices.as<uint32_t>();
    sc.vertices = st->vertices.as<float>();
    sc.meshes = st->meshes.as<ArkRTTriangleMesh>();
    sc.materials = st->materials.as<ArkShaderMaterial>();
    sc.tex_infos = st->texInfos.as<GpuTextureInfo>();
    sc.texels = st->texels.as<float4>();
    sc.white_texture = static_cast<int32_t>(s->texture_count);
    sc.env_texture = (s->environment_texture >= 0 && static_cast<uint32_t>(s->environment_texture) < s->texture_count) ? s->environment_texture : sc.white_texture;
    sc.sun_root = -1;
    // lights: the scene's are each context's until ark_ddgi_set_lights (deriveSceneArgs)
    st->hasSunScene = s->has_directional_light ? 1 : 0;
    st->sunScene = s->directional_light;
    st->spotsScene = std::move(gspots);
    st->sunWanted = st->sun.nodeCount > 0;
    st->buildThreads = opt.threads;
    // the sun's traversal pushes onto the same spill area (its depth counts)
    st->bvhMaxDepth = std::max(st->world.depth, st->sun.depth);
    const auto t1 = std::chrono::steady_clock::now();
    st->bvhStats.node_count = w.nodes.size();
    st->bvhStats.triangle_count = w.triangles;
    st->bvhStats.max_depth = st->bvhMaxDepth;
    st->bvhStats.max_leaf_size = w.maxLeaf;
    st->bvhStats.sah_cost = w.sah;
    st->bvhStats.build_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    st->bvhStats.node_bytes = w.nodes.size() * sizeof(GpuBvh8Node);
    st->bvhStats.triangle_bytes = w.tris.size() * sizeof(GpuTriangle);
    st->bvhStats.sun_node_count = st->sun.nodeCount;
    st->bvhStats.sun_max_depth = st->sun.depth;
    st->bvhStats.sun_cost_world = st->sunCostWorld;
    st->bvhStats.sun_cost_light = st->sunCostLight;
    st->bvhStats.sun_build_ms = sunBuildMs;
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
    const bool sunWork = st.sunWanted && ctx->hasSun && (st.sunJob ? st.sunJob->done.load(std::memory_order_acquire) : true);
    if (!sunWork) return sunRebuildStep(ctx, nullptr);
    const uint32_t v = st.version;
    const bool hadJob = static_cast<bool>(st.sunJob);
    ARK_HIP(orderBegin(ctx, ctx->stream));
    if (const int rc = sunRebuildStep(ctx, ctx->stream)) return rc;
    if (st.version != v || static_cast<bool>(st.sunJob) != hadJob) ARK_HIP(orderEnd(ctx, ctx->stream));
    return ARK_DDGI_OK;
}

namespace {
// ark_ddgi_set_instances' first use of a scene: the world BVHs' nodes by depth, deepest
// first, and the refit's work buffers (a topology download: refits never change it)
int prepareRefit(ArkDdgiCtx* ctx, SceneStore& st)
{
    DeviceBvh& w = st.world;
    const uint64_t n = w.nodeCount;
    std::vector<GpuBvh8Node> h(n);
    if (n) ARK_HIP(hipMemcpy(h.data(), w.buf.ptr, n * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost));
    const int32_t roots[3] = { st.args.root_opaque, st.args.root_masked, st.args.root_blend };
    std::vector<uint32_t> order;
    if (!bvhLevelOrder(h.data(), n, roots, 3, order, w.levelOffsets)) return ctx->fail(ARK_DDGI_E_DEVICE, "refit: a node outside the BVH");
    int rc;
    if ((rc = upload(ctx, w.order, order.data(), order.size())) != 0) return rc;
    ARK_HIP(w.boxes.alloc(std::max<size_t>(16, n * 6 * sizeof(float))));
    return ARK_DDGI_OK;
}
} // namespace

namespace {
// The refitted spare becomes the front copy (SceneStore::spare), the front one the last
// spare: the kernel views follow.
void rotateGeometry(SceneStore& st)
{
    const bool sun = st.sunArgs.sun_root >= 0 && st.sun.buf.ptr;
    SceneStore::Spare old;
    old.world = st.world.buf;
    old.sun = st.sun.buf;
    old.instances = st.instances;
    old.valid = true;
    old.slot = st.front;
    st.world.buf = st.spare[0].world;
    st.sun.buf = st.spare[0].sun;
    st.instances = st.spare[0].instances;
    st.front = st.spare[0].slot;
    st.spare[0] = st.spare[1];
    st.spare[1] = old;
    setWorldArgs(st);
    if (sun) setSunArgs(st);
}
} // namespace

static int checkSequencing(ArkDdgiCtx* ctx);

int ark_ddgi_set_instances_async(ArkDdgiCtx* ctx, const ArkRTInstance* instances, uint32_t count, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "ark_ddgi_set_instances before ark_ddgi_set_scene");
    SceneStore& st = *ctx->sceneStore;
    if (count != st.instHost.size() || (count && !instances))
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: %u instances, the scene has %zu", count, st.instHost.size());
    for (uint32_t i = 0; i < count; ++i) {
        const ArkRTInstance &a = instances[i], &b = st.instHost[i];
        if (a.rt_mesh_index != b.rt_mesh_index || a.triangle_count != b.triangle_count || a.hit_mask != b.hit_mask)
            return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: instance %u changed its mesh, triangle count or hit mask (a set_scene builds a new scene)", i);
        for (float v : a.object_to_world)
            if (!std::isfinite(v)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: instance %u: non-finite transform", i);
    }
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (const int r = checkSequencing(ctx)) return r;
    // with a shared scene every context's launches may read either copy: all of them end
    // first (and the refit below before returning)
    const bool shared = ctx->sceneStore.use_count() > 1;
    if (shared) ARK_HIP(hipDeviceSynchronize());
    int rc;
    if (st.world.levelOffsets.empty() && (rc = prepareRefit(ctx, st)) != 0) return rc;
    // everything this context enqueued so far ends with its last operation (orderBegin
    // chains the others into it): the front copy's readers among them. Events that mark
    // that point are recorded on `s` behind it (orderBegin) - not on the last operation's
    // stream, which the caller may have destroyed since, nor on a stream of the
    // context's own (one more stream on the process's few hardware queues; measured no
    // better under motion, profiles/r06_ab2_refit_ordering/)
    ARK_HIP(orderBegin(ctx, s));
    const hipStream_t last = s;
    // a light-space sun BVH without a refit order (none recorded) cannot follow: dropped
    if (st.sunArgs.sun_root >= 0 && st.sun.levelOffsets.empty()) {
        st.sunArgs.sun_root = -1;
        st.sunArgs.sun_nodes = nullptr;
        st.sunArgs.sun_tris = nullptr;
        ARK_HIP(retireBuffer(st, st.sun.buf, last));
        ARK_HIP(dropSpares(st, last));
        st.sun.nodeCount = 0;
        st.bvhStats.sun_node_count = 0;
        st.bvhStats.sun_max_depth = 0;
    }
    // The refit writes the next spare copy on the refit stream, after the operations that
    // read it (while it was the front one: evFree) and the last install; the frames in
    // flight keep reading the front copy. The copy swapped out here is free once the
    // operations enqueued so far are done.
    SceneStore::Spare& tgt = st.spare[0];
    const int fs = st.front, ts = tgt.slot;
    const hipStream_t rs = ctx->refitStream;
    ARK_HIP(hipEventRecord(ctx->evFree[fs], last));
    ctx->freeValid[fs] = true;
    if (ctx->freeValid[ts]) ARK_HIP(hipStreamWaitEvent(rs, ctx->evFree[ts], 0));
    if (ctx->installValid) {
        ARK_HIP(hipStreamWaitEvent(rs, ctx->evInstalled, 0));
        ctx->installValid = false;
    }
    if (!tgt.valid) {
        // a copy of the front one (a new scene or an installed rebuild)
        auto copy = [&](DeviceBuffer& dst, const DeviceBuffer& src) -> hipError_t {
            if (!src.ptr) return retireBuffer(st, dst, last);
            hipError_t e = hipSuccess;
            if (dst.bytes != src.bytes) {
                if ((e = retireBuffer(st, dst, last)) != hipSuccess) return e;
                if ((e = dst.alloc(src.bytes)) != hipSuccess) return e;
            }
            return hipMemcpyAsync(dst.ptr, src.ptr, src.bytes, hipMemcpyDeviceToDevice, rs);
        };
        ARK_HIP(copy(tgt.world, st.world.buf));
        ARK_HIP(copy(tgt.sun, st.sun.buf));
        ARK_HIP(copy(tgt.instances, st.instances));
        st.xf[ts] = st.xf[fs];
        st.inflCopy[ts][0] = st.inflCopy[fs][0];
        st.inflCopy[ts][1] = st.inflCopy[fs][1];
        tgt.valid = true;
    }
    // the instance table of the shading kernels (set_scene's determinant and rows)
    std::vector<GpuInstance> ginst(count);
    for (uint32_t ii = 0; ii < count; ++ii) ginst[ii] = gpuInstance(instances[ii], st.meshHost[instances[ii].rt_mesh_index]);
    ARK_HIP(stagedUpload(st, tgt.instances.ptr, ginst.data(), count * sizeof(GpuInstance), rs));
    if ((rc = uploadRefitInstances(ctx, st, instances, count, &st.xf[ts], rs)) != 0) return rc;
    if ((rc = enqueueRefit(ctx, st, rs, tgt.world, tgt.sun, ts)) != 0) return rc;
    ARK_HIP(hipEventRecord(ctx->evRefit, rs));
    if (shared) ARK_HIP(hipStreamSynchronize(rs));
    // the refitted copy becomes the front one
    st.xf[ts].resize(count);
    for (uint32_t ii = 0; ii < count; ++ii) std::memcpy(st.xf[ts][ii].data(), instances[ii].object_to_world, sizeof(float) * 12);
    rotateGeometry(st);
    // the caller's stream follows the refit (what it runs next sees the new geometry); the
    // next update's traversal on the traversal stream waits for it too (refitPending)
    ARK_HIP(hipStreamWaitEvent(s, ctx->evRefit, 0));
    ctx->refitPending = true;
    for (uint32_t ii = 0; ii < count; ++ii) std::memcpy(st.instHost[ii].object_to_world, instances[ii].object_to_world, sizeof(float) * 12);
    ++st.version;
    ++st.refitsSinceBuild;
    ++st.sunRefitsSinceBuild;
    st.bvhStats.refit_version = ++st.refitCount;
    if ((rc = refreshScene(ctx)) != 0) return rc;
    // background rebuilds of the loosened BVHs (world and light-space), from a snapshot
    // taken on s behind this refit
    if ((rc = sceneMaintenance(ctx, s)) != 0) return rc;
    ARK_HIP(orderEnd(ctx, s));
    st.bvhStats.refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_scene_digest(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "scene digest before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    const SceneStore& st = *ctx->sceneStore;
    auto digest = [&](const void* dev, size_t bytes, uint64_t& h) -> hipError_t {
        h = 1469598103934665603ull;
        if (!dev || !bytes) return hipSuccess;
        std::vector<unsigned char> b(bytes);
        const hipError_t e = hipMemcpy(b.data(), dev, bytes, hipMemcpyDeviceToHost);
        for (unsigned char c : b) h = (h ^ c) * 1099511628211ull;
        return e;
    };
    ARK_HIP(digest(st.args.nodes, st.world.nodeCount * sizeof(GpuBvh8Node), out[0]));
    ARK_HIP(digest(st.args.tris, st.world.records * sizeof(GpuTriangle), out[1]));
    const bool sun = st.sunArgs.sun_root >= 0;
    ARK_HIP(digest(sun ? st.sunArgs.sun_nodes : nullptr, st.sun.nodeCount * sizeof(GpuBvh8Node), out[2]));
    ARK_HIP(digest(sun ? st.sunArgs.sun_tris : nullptr, st.sun.records * sizeof(GpuTriangle), out[3]));
    if (!sun) out[2] = out[3] = 0;
    return ARK_DDGI_OK;
}

int ark_ddgi_debug_world_bvh_check(ArkDdgiCtx* ctx, uint64_t* out)
{
    if (!ctx || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "world BVH check before ark_ddgi_set_scene");
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    const SceneStore& st = *ctx->sceneStore;
    std::vector<GpuBvh8Node> nodes(st.world.nodeCount);
    std::vector<GpuTriangle> tris(st.world.records);
    std::vector<uint32_t> order(nodes.size());
    if (!nodes.empty()) ARK_HIP(hipMemcpy(nodes.data(), st.args.nodes, nodes.size() * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost));
    if (!tris.empty()) ARK_HIP(hipMemcpy(tris.data(), st.args.tris, tris.size() * sizeof(GpuTriangle), hipMemcpyDeviceToHost));
    if (!order.empty() && st.world.order.bytes >= order.size() * 4) ARK_HIP(hipMemcpy(order.data(), st.world.order.ptr, order.size() * 4, hipMemcpyDeviceToHost));
    const std::vector<int> classOf = instanceClasses(st);
    const int32_t roots[3] = { st.args.root_opaque, st.args.root_masked, st.args.root_blend };
    Bvh8CheckResult c = check_bvh8_full(nodes, tris, roots, 3, &classOf, nullptr);
    std::string why;
    if (!checkBvh8Structure(nodes, tris, roots, 3, why)) c.violations++;
    if (c.nodes != nodes.size()) c.violations++; // a node outside the classes' ranges
    if (st.worldGpuBuilt) c.violations += c.notBreadthFirst; // the device build's order (the host collapse's: breadth first per subtree block)
    if (roots[0] >= 0 && st.args.opaque_nodes != static_cast<uint32_t>((roots[1] >= 0 ? roots[1] : roots[2] >= 0 ? roots[2] : static_cast<int32_t>(nodes.size())) - roots[0]))
        c.violations++;
    // the refit's level order (none before the first refit after set_scene) against the
    // one recomputed from the downloaded nodes
    std::vector<uint32_t> wantOrder, wantOffsets;
    if (!bvhLevelOrder(nodes.data(), nodes.size(), roots, 3, wantOrder, wantOffsets)) {
        c.violations++;
    } else if (!st.world.levelOffsets.empty() && (wantOrder != order || wantOffsets != st.world.levelOffsets)) {
        c.violations++;
        why += " level order";
    }
    uint64_t live = 0, digest = 0;
    for (const GpuTriangle& g : tris) {
        if (isHoleTriangle(g)) continue;
        ++live;
        uint64_t h = 1469598103934665603ull;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(&g);
        for (size_t k = 0; k < sizeof(GpuTriangle); ++k) h = (h ^ b[k]) * 1099511628211ull;
        digest += h;
    }
    if (live != c.triangles) c.violations++;
    out[0] = nodes.size();
    out[1] = c.leafChildren;
    out[2] = c.maxDepth;
    out[3] = c.violations;
    out[4] = live;
    out[5] = tris.size();
    out[6] = digest;
    out[7] = st.worldGpuBuilt ? 1u : 0u;
    if (c.violations) ctx->lastError = "world BVH check: " + std::to_string(c.violations) + " violations" + (why.empty() ? "" : " (" + why + ")");
    return c.violations ? 1 : ARK_DDGI_OK;
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
    if (const int rc = sceneMaintenance(ctx, s)) return rc;
    if (ctx->sceneVersion != ctx->sceneStore->version) // another context refitted the shared scene or installed a BVH
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
    // a refit or an installed rebuild enqueued since the last update (on any stream): the
    // traversal reads the BVH it writes
    if (ctx->refitPending) {
        if (ts != s) ARK_HIP(hipStreamWaitEvent(ts, ctx->evRefit, 0));
        ctx->refitPending = false;
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
        if (f.light_count > 0) {
            ARK_HIP(launch_shadow_gen(ctx->scene, fs, s));
            ARK_HIP(launch_trace_shadow(ctx->scene, fs, count ? ctx->shadowBlocks : shadowBlocksFor(ctx, f.window_rays), count, s));
        }
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[5], s));
        // shading reads the previous frame's atlases at arbitrary probes: on a Z-slab
        // rank it waits here for the previous exchange (the traversal above did not)
        if (shadeWaitEvent) ARK_HIP(hipStreamWaitEvent(s, static_cast<hipEvent_t>(shadeWaitEvent), 0));
        if (shadeWaitSeq) ARK_HIP(launch_seq_wait(seqTrace + 96, shadeWaitSeq, seqTimedOut, ctx->hostAbortDev, ctx->seqTimeoutTicks, s));
        ARK_HIP(launch_shade(ctx->scene, fs, ctx->shadeBlocks, count, s));
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[2], s));
        if (timing) ARK_HIP(hipEventRecord(ctx->ev[4], s));
        traceZone.end();
        // probeUpdateOffset (serial frames), probeUpdateIrradiance/Visibility + border
        // corners/edges, fused
        RoctxRange updateZone("Update probes");
        if (!pipe) ARK_HIP(launch_probe_offsets(fs, s));
        ARK_HIP(launch_probe_update(fs, s));
    } else {
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
