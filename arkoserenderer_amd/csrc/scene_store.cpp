// scene_store.cpp — the device scene and its maintenance (scene_store.h): set_scene's
// build, the stream-ordered refits of ark_ddgi_set_instances, the background rebuilds of
// the world BVHs and the light-space sun BVH, the debug downloads.
#include "scene_store.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <thread>

#include "../../include/ark_ddgi_debug.h"
#include "ark_fmath.h"
#include "bvh_builder.h"

// (every function here that can fail has an ErrorSink* err in scope)
#define ARK_HIP(expr) ARK_HIP_TO(err, expr)

namespace ark {

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

// A background rebuild of the sun's light-space BVH (sunCollect / sunStart): a host thread
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
    // runSunJobGpu: the device built the result; or it handed the job to the host build
    // (t0: the job's start, so that ms stays the whole job's wall time)
    bool gpu = false, gpuFallback = false, gpuFallbackCounted = false;
    uint32_t instances = 0; // of the scene (the device build checks the records' against it)
    std::chrono::steady_clock::time_point t0 {};
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

namespace {

template<typename T>
int upload(ErrorSink* err, DeviceBuffer& buf, const T* data, size_t count)
{
    size_t bytes = count * sizeof(T);
    ARK_HIP(buf.alloc(std::max<size_t>(bytes, 16)));
    if (bytes) ARK_HIP(hipMemcpy(buf.ptr, data, bytes, hipMemcpyHostToDevice));
    return ARK_DDGI_OK;
}

} // namespace

// (GpuScene.cpp:844-858: the fields of LightData.h:19-40 the DDGI path uses)
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

namespace {

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

// --- scene maintenance: stream-ordered refits, background rebuilds ------------------

// A buffer the launches enqueued so far on `s` (and, by the entry points' precondition,
// everything the context enqueued before) may read: freed by collectRetired once they are done.
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
int refitBvh(ErrorSink* err, SceneStore& st, DeviceBvh& b, const DeviceBuffer& copy, RefitBoxArgs args, uint64_t dirty, float& held, hipStream_t s)
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
int enqueueRefit(ErrorSink* err, SceneStore& st, hipStream_t s, const DeviceBuffer& world, const DeviceBuffer& sun, int slot)
{
    float inflateWorld = 0.0f, inflateLight = 0.0f;
    refitInflations(st, inflateWorld, inflateLight);
    uint64_t dirty = 0;
    for (size_t i = 0; i < st.refitHost.size(); ++i)
        if (st.refitHost[i].dirty) dirty |= 1ull << (i & 63u);
    RefitBoxArgs a {};
    a.inflate = inflationStep(inflateWorld);
    a.light = 0;
    if (const int rc = refitBvh(err, st, st.world, world, a, dirty, st.inflCopy[slot][0], s)) return rc;
    if (st.sunArgs.sun_root >= 0 && st.sun.records && !st.sun.levelOffsets.empty()) {
        std::memcpy(a.frame, st.sunFrameD, sizeof(a.frame));
        a.inflate = inflationStep(inflateLight);
        a.light = 1;
        if (const int rc = refitBvh(err, st, st.sun, sun, a, dirty, st.inflCopy[slot][1], s)) return rc;
    }
    st.refitFull = false;
    return ARK_DDGI_OK;
}

// The refit's transforms of `instances` on the device (stream-ordered), every one dirty
// (have = nullptr: the records are of an older version, an installed rebuild) or those
// whose transform differs from the one the target copy's records hold (`have`).
int uploadRefitInstances(ErrorSink* err, SceneStore& st, const ArkRTInstance* instances, uint32_t count, const std::vector<std::array<float, 12>>* have,
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
hipError_t installedGeometry(SceneStore& st, hipStream_t s)
{
    hipError_t e = dropSpares(st, s);
    markTopologyChanged(st); // (again: the boxes scratch is of the old topology without a forward refit)
    std::vector<std::array<float, 12>>& xf = st.xf[st.front];
    xf.resize(st.instHost.size());
    for (size_t i = 0; i < st.instHost.size(); ++i) std::memcpy(xf[i].data(), st.instHost[i].object_to_world, sizeof(float) * 12);
    if (e == hipSuccess) e = hipEventRecord(st.evInstalled, s);
    st.installValid = e == hipSuccess;
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
    const auto t0 = job->gpuFallback ? job->t0 : std::chrono::steady_clock::now();
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

// What a traced device build keeps on the host (ark_ddgi_debug_lbvh_device_parity): every
// stage's result, downloaded before buildLbvhGpu returns (the stages after a fallback: empty)
struct LbvhGpuTrace {
    LbvhHeader hdr {};                            // as the build uses it (the light build's classCount[0] = prims)
    std::vector<uint32_t> idx, idxSorted, split;  // hdr.prims each (split: set at the internal indices of each class range)
    std::vector<uint64_t> keysSorted;
    std::vector<GpuBvh8Node> nodes;
    std::vector<GpuTriangle> tris;                // the rows, then the padding record
    std::vector<uint32_t> perm, order, levelOffsets;
    int32_t roots[3] { -1, -1, -1 };
    uint32_t opaqueNodes = 0, depth = 0;
    float inflateAbs = 0.0f;
    bool built = false;
    std::string why;                              // the fallback reason
};

// What the device builds of the world BVH8s and of the sun's light-space BVH8 differ in
// (buildLbvhGpu): the class ranges, the key kernels, the slot rule and the refit's boxes.
struct LbvhGpuBuild {
    // in
    const GpuTriangle* snap = nullptr; // the snapshot's records, ready once evSnap has completed
    hipEvent_t evSnap = nullptr;
    uint32_t records = 0;
    std::vector<uint32_t> classHost;   // instance -> class (its size: the instances)
    bool light = false;                // the sun's: one range over every class, keys and boxes in `frame`
    double frame[9] {};
    int slotRule = lbvh::kSlotsOctant, wBits = lbvh::kMortonBits;
    DeviceBvh* bvh = nullptr;          // out: buffer, level order (device and offsets), counts, depth, inflateAbs
    DeviceBuffer* perm = nullptr;      // out: the record order's source indices (null: not wanted)
    LbvhGpuTrace* trace = nullptr;     // out: the stages' results (null in the product paths: nothing more is enqueued)
    // out
    int32_t roots[3] { -1, -1, -1 };
    uint32_t opaqueNodes = 0, prims = 0;
    std::vector<uint32_t> order;       // the level order on the host
};

// The device build on `s`: hipSuccess and `why` empty when g.bvh holds the result; `why`
// set when the host has to build this scene.
hipError_t buildLbvhGpu(LbvhGpuBuild& g, hipStream_t s, std::string& why)
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
    struct KeepWhy {
        LbvhGpuTrace* trace;
        const std::string& why;
        ~KeepWhy()
        {
            if (trace) trace->why = why;
        }
    } keepWhy { g.trace, why };
#define ARK_GB(expr)                          \
    do {                                      \
        if ((e = (expr)) != hipSuccess) return e; \
    } while (0)
    if (g.records == 0 || g.classHost.empty()) {
        why = "no records";
        return hipSuccess;
    }
    const uint32_t records = g.records, instances = static_cast<uint32_t>(g.classHost.size());
    const GpuTriangle* snap = g.snap;
    const std::vector<uint32_t>& classHost = g.classHost;
    ARK_GB(arenaA.buf.alloc(Arena::pad(instances * 4ull) + Arena::pad(sizeof(LbvhHeader)) + Arena::pad(records * 4ull) + Arena::pad(records * 8ull)));
    w.classOf = arenaA.take(instances * 4ull);
    w.hdr = arenaA.take(sizeof(LbvhHeader));
    w.idx = arenaA.take(records * 4ull);
    w.keys = arenaA.take(records * 8ull);
    ARK_GB(hipMemcpyAsync(w.classOf.ptr, classHost.data(), instances * 4ull, hipMemcpyHostToDevice, s));
    ARK_GB(hipStreamWaitEvent(s, g.evSnap, 0));
    if (g.light) {
        LbvhFrame fr;
        std::memcpy(fr.m, g.frame, sizeof(fr.m));
        ARK_GB(launch_lbvh_prims_light(snap, records, instances, fr, g.wBits, w.idx.as<uint32_t>(), w.keys.as<uint64_t>(), w.hdr.as<LbvhHeader>(), s));
    } else {
        ARK_GB(launch_lbvh_prims(snap, records, w.classOf.as<uint32_t>(), instances, w.idx.as<uint32_t>(), w.keys.as<uint64_t>(), w.hdr.as<LbvhHeader>(), s));
    }
    LbvhHeader hdr {};
    ARK_GB(hipMemcpyAsync(&hdr, w.hdr.ptr, sizeof(hdr), hipMemcpyDeviceToHost, s));
    ARK_GB(hipStreamSynchronize(s));
    if (g.light && !hdr.error) hdr.classCount[0] = hdr.prims; // one range [0, n): the keys' class bits are 0
    if (g.trace) g.trace->hdr = hdr;
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
    a.slotRule = g.slotRule;
    a.wBits = g.wBits;
    std::vector<std::array<uint32_t, 3>> levels; // node counts [depth][class]
    uint32_t nodeTotal = 0, counters[kLbvhCounters] = {};
    for (int c = 0; c < 3; ++c) {
        if (!hdr.classCount[c]) continue;
        g.roots[c] = static_cast<int32_t>(nodeTotal);
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
        if (c == 0) g.opaqueNodes = nodeTotal;
    }
    const uint32_t outRecords = counters[kLbvhRecords];
    if (!(DeviceBvh::bytesFor(nodeTotal, outRecords) < (1ull << 32))) {
        why = "nodes and records of 4 GiB or more";
        return hipSuccess;
    }
    // the installed buffers, sized from the counts read back
    DeviceBvh& b = *g.bvh;
    b.triOffset = DeviceBvh::triOffsetFor(nodeTotal);
    ARK_GB(b.buf.alloc(DeviceBvh::bytesFor(nodeTotal, outRecords)));
    if (g.perm) ARK_GB(g.perm->alloc(std::max<size_t>(16, outRecords * 4ull)));
    GpuBvh8Node* nodes = b.nodes(b.buf);
    GpuTriangle* tris = b.tris(b.buf);
    ARK_GB(hipMemcpyAsync(nodes, w.nodes.ptr, nodeTotal * sizeof(GpuBvh8Node), hipMemcpyDeviceToDevice, s));
    ARK_GB(launch_lbvh_scatter(snap, w.idxSorted.as<uint32_t>(), w.position.as<uint32_t>(), tris, g.perm ? g.perm->as<uint32_t>() : nullptr, n, outRecords, s));
    // the refit's level order from the level counts (bvhLevelOrder's format: deepest level
    // first, ascending node index within a level; each class one breadth-first range)
    std::vector<uint32_t>& order = g.order;
    order.clear();
    order.reserve(nodeTotal);
    b.levelOffsets.assign(1, 0u);
    {
        std::vector<std::array<uint32_t, 3>> base(levels.size());
        uint32_t at[3];
        for (int c = 0; c < 3; ++c) at[c] = g.roots[c] >= 0 ? static_cast<uint32_t>(g.roots[c]) : 0u;
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
    // or, in light coordinates, build_sun_bvh's (the box and the largest |coordinate| are
    // min / max reductions: the same bits whatever the order)
    ARK_GB(hipMemsetAsync(w.masks.ptr, 0xff, nodeTotal * 8ull, s));
    ARK_GB(hipMemsetAsync(w.inst.ptr, 0, instances * sizeof(RefitInstance), s));
    RefitBoxArgs ra {};
    ra.inflate = bvh8_inflation_box(lo, hi);
    ra.light = 0;
    if (g.light) {
        float maxAbs;
        std::memcpy(&maxAbs, &hdr.maxAbs, 4);
        ra.inflate = 2.0f * bvh8_inflation_box(lo, hi) + 2e-6f * maxAbs;
        ra.light = 1;
        std::memcpy(ra.frame, g.frame, sizeof(ra.frame));
    }
    b.inflateAbs = ra.inflate;
    ra.dirty = ~0ull;
    for (size_t l = 0; l + 1 < b.levelOffsets.size(); ++l)
        ARK_GB(launch_refit_nodes(nodes, tris, w.boxes.as<float>(), b.order.as<uint32_t>() + b.levelOffsets[l], b.levelOffsets[l + 1] - b.levelOffsets[l], ra,
                                  w.masks.as<uint64_t>(), w.inst.as<RefitInstance>(), nullptr, nullptr, s));
    ARK_GB(hipStreamSynchronize(s));
    if (LbvhGpuTrace* t = g.trace) {
        t->idx.resize(n);
        t->idxSorted.resize(n);
        t->split.resize(n);
        t->keysSorted.resize(n);
        t->nodes.resize(nodeTotal);
        t->tris.resize(outRecords + 1ull);
        t->perm.resize(g.perm ? outRecords : 0u);
        ARK_GB(hipMemcpyAsync(t->idx.data(), w.idx.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->idxSorted.data(), w.idxSorted.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->split.data(), w.split.ptr, n * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->keysSorted.data(), w.keysSorted.ptr, n * 8ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->nodes.data(), nodes, nodeTotal * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost, s));
        ARK_GB(hipMemcpyAsync(t->tris.data(), tris, (outRecords + 1ull) * sizeof(GpuTriangle), hipMemcpyDeviceToHost, s));
        if (!t->perm.empty()) ARK_GB(hipMemcpyAsync(t->perm.data(), g.perm->ptr, outRecords * 4ull, hipMemcpyDeviceToHost, s));
        ARK_GB(hipStreamSynchronize(s));
        t->order = order;
        t->levelOffsets = b.levelOffsets;
        std::copy(g.roots, g.roots + 3, t->roots);
        t->opaqueNodes = g.opaqueNodes;
        t->depth = static_cast<uint32_t>(levels.size());
        t->inflateAbs = ra.inflate;
        t->built = true;
    }
#undef ARK_GB
    b.nodeCount = nodeTotal;
    b.records = outRecords;
    b.depth = static_cast<uint32_t>(levels.size());
    g.prims = n;
    return hipSuccess;
}

// The device build of runWorldJobGpu: the three classes' BVH8s into job
hipError_t buildWorldGpu(WorldJob* job, hipStream_t s, std::string& why)
{
    if (job->snapRecords > 0x7fffffffull) {
        why = "no records";
        return hipSuccess;
    }
    LbvhGpuBuild g;
    g.snap = job->snap.as<GpuTriangle>();
    g.evSnap = job->evSnap;
    g.records = static_cast<uint32_t>(job->snapRecords);
    g.classHost.assign(job->classOf.begin(), job->classOf.end());
    g.bvh = &job->bvh;
    g.perm = &job->perm;
    const float inflateAbs = job->bvh.inflateAbs; // (worldCollect sets the installed one's)
    const hipError_t e = buildLbvhGpu(g, s, why);
    job->bvh.inflateAbs = inflateAbs;
    std::copy(g.roots, g.roots + 3, job->roots);
    job->opaqueNodes = g.opaqueNodes;
    job->maxLeaf = std::min<uint32_t>(g.prims, static_cast<uint32_t>(kBvh8MaxLeafSize));
    job->sah = 0.0f; // not evaluated on the device
    return e;
}


// The sun rebuild's thread with ARK_DDGI_FLAG_GPU_REBUILD_SUN: the same inputs and outputs as
// runSunJob (job->bvh, levelOrder, frame, inflateAbs, depth, ms), the light-space BVH8 built
// on the device - one LBVH over every class's records, keyed and boxed in the sun's frame,
// its slots in ascending w - on a stream of the lowest priority that waits for the snapshot
// on the device. A scene the device build does not take (no records, 4 GiB, depth, node
// scratch, an error that is not a device fault) is built by runSunJob within this job; a
// device fault fails the job (a sun rebuild failure: not retried).
void runSunJobGpu(SunJob* job, int device, uint64_t count, int threads)
{
    job->t0 = std::chrono::steady_clock::now();
    hipStream_t s = nullptr;
    std::string why;
    hipError_t e = hipSetDevice(device);
    int least = 0, greatest = 0;
    if (e == hipSuccess) e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least);
    if (e == hipSuccess) {
        double frame[3][3];
        sun_frame(job->dir, frame);
        std::memcpy(job->frame, frame, sizeof(job->frame));
        if (count > 0x7fffffffull) {
            why = "no records";
        } else {
            LbvhGpuBuild g;
            g.snap = job->snap.as<GpuTriangle>();
            g.evSnap = job->evSnap;
            g.records = static_cast<uint32_t>(count);
            g.classHost.assign(job->instances, 0u); // one tree: only the instance count matters
            g.light = true;
            std::memcpy(g.frame, job->frame, sizeof(g.frame));
            g.slotRule = lbvh::kSlotsAscendingW;
            g.wBits = lbvh::kSunKeyBitsW;
            g.bvh = &job->bvh;
            e = buildLbvhGpu(g, s, why);
            job->levelOrder = std::move(g.order);
            // (installSunBvh uploads the level order from the host, as after a host build)
            job->bvh.order.release();
        }
    }
    if (s) (void)hipStreamDestroy(s);
    if (e == hipSuccess && why.empty()) {
        job->gpu = true;
        job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - job->t0).count();
        job->ok = true;
        job->done.store(true, std::memory_order_release);
        return;
    }
    if (isDeviceFault(e)) {
        job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - job->t0).count();
        job->ok = false;
        job->done.store(true, std::memory_order_release);
        return;
    }
    // the host build from the same snapshot
    job->bvh.release();
    job->bvh = DeviceBvh {};
    job->levelOrder.clear();
    job->gpuFallback = true;
    runSunJob(job, device, count, threads);
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

// A shared scene's refits and installs, kept synchronous for now: the frames in flight of
// every sharing context may read what the call replaces or overwrites, and the store's
// events record only the calling context's readers, so the call begins once the device
// is idle (every context's work) and its work on `s` completes before it returns (the
// other contexts' next traversals need not wait for this context's streams). Unshared,
// the caller's stream is ordered behind its context's earlier operations (the
// precondition) and what is replaced is retired behind it.
hipError_t sharedBegin(const SceneCall& c) { return c.shared ? hipDeviceSynchronize() : hipSuccess; }
hipError_t sharedEnd(const SceneCall& c, hipStream_t s) { return c.shared ? hipStreamSynchronize(s) : hipSuccess; }

// The last refit or install ends on `s`: the contexts' next traversals wait for it
hipError_t geometryChanged(SceneStore& st, hipStream_t s)
{
    ++st.geometrySeq;
    return hipEventRecord(st.evGeometry, s);
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
int installSunBvh(ErrorSink* err, SceneStore& st, DeviceBvh& b, Bvh8BuildResult* host, const std::vector<uint32_t>& levelOrder, const double* frame, const float* dir,
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
int finishInstall(SceneStore& st, const SceneCall& c, uint32_t refitsSince, hipStream_t s)
{
    ErrorSink* err = c.err;
    markTopologyChanged(st);
    if (refitsSince) {
        if (const int rc = uploadRefitInstances(err, st, st.instHost.data(), static_cast<uint32_t>(st.instHost.size()), nullptr, s)) return rc;
        if (const int rc = enqueueRefit(err, st, s, st.world.buf, st.sun.buf, st.front)) return rc;
    }
    ARK_HIP(installedGeometry(st, s));
    ARK_HIP(geometryChanged(st, s));
    ARK_HIP(sharedEnd(c, s));
    ++st.version;
    return ARK_DDGI_OK;
}

// The light-space sun BVH follows the context's sun (called by every update and by
// set_lights / set_instances, on the stream `s` of the call): a finished rebuild for
// this context's sun is installed - stream-ordered behind the frames that may read the
// old one, and refitted forward when refits came in between - and a new one is started
// when the scene chose the light-space BVH at set_scene but holds none for this
// direction. Until it is installed the sun's shadow rays traverse the world BVHs
// (deriveSceneArgs), with the same results. sunCollect: the request streak and a
// finished rebuild (installed only when the caller mayEnqueue on `s`, else left to the
// next call); rebuildToStart / sunStart: a new one.
bool sameDir(const float* a, const float* b) { return std::memcmp(a, b, 3 * sizeof(float)) == 0; }

int sunCollect(SceneStore& st, const SceneCall& c, hipStream_t s, bool mayEnqueue)
{
    ErrorSink* err = c.err;
    if (c.hasSun) {
        if (st.sunReqStreak && sameDir(st.sunReqDir, c.sunDir)) {
            st.sunReqStreak = std::min<uint32_t>(st.sunReqStreak + 1u, 1u << 30);
        } else {
            std::memcpy(st.sunReqDir, c.sunDir, sizeof(st.sunReqDir));
            st.sunReqStreak = 1;
        }
    }
    if (st.sunJob && st.sunJob->done.load(std::memory_order_acquire)) {
        SunJob& j = *st.sunJob;
        if (j.gpuFallback && !j.gpuFallbackCounted) {
            st.bvhStats.sun_gpu_fallbacks++;
            j.gpuFallbackCounted = true;
        }
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
        } else if (mayEnqueue && c.hasSun && sameDir(j.dir, c.sunDir)) {
            std::unique_ptr<SunJob> job = std::move(st.sunJob);
            job->t.join();
            ARK_HIP(sharedBegin(c));
            if (const int rc = installSunBvh(err, st, job->bvh, nullptr, job->levelOrder, job->frame, job->dir, s)) return rc;
            ARK_HIP(retireBuffer(st, job->snap, s));
            st.bvhMaxDepth = std::max(st.bvhMaxDepth, st.sun.depth);
            st.bvhStats.max_depth = st.bvhMaxDepth;
            st.bvhStats.sun_node_count = st.sun.nodeCount;
            st.bvhStats.sun_max_depth = st.sun.depth;
            st.bvhStats.sun_rebuilds = ++st.sunRebuilds;
            st.bvhStats.sun_build_ms = job->ms;
            st.sunGpuBuilt = job->gpu;
            st.bvhStats.sun_installed_builder = job->gpu ? 1u : 0u;
            if (job->gpu) st.bvhStats.sun_gpu_rebuilds++;
            st.sunRefitsSinceBuild = st.refitCount - job->refitsAt;
            st.bvhStats.sun_built_refit_version = job->refitsAt;
            // (refits that came in while it was built: its records follow them)
            if (const int rc = finishInstall(st, c, st.sunRefitsSinceBuild, s)) return rc;
        }
        // else: built for another context's sun, which installs it (or the caller has no
        // ordered stream now: its next call does)
    }
    return ARK_DDGI_OK;
}

int sunStart(SceneStore& st, const SceneCall& c, hipStream_t s, bool gpu)
{
    ErrorSink* err = c.err;
    auto job = std::make_unique<SunJob>();
    std::memcpy(job->dir, c.sunDir, sizeof(job->dir));
    job->version = st.version;
    job->refitsAt = st.refitCount;
    ARK_HIP(snapshotRecords(st, job->snap, job->evSnap, s));
    job->instances = static_cast<uint32_t>(st.instHost.size());
    job->t = std::thread(gpu ? runSunJobGpu : runSunJob, job.get(), st.device, st.world.records, std::max(1, st.buildThreads / 2));
    st.sunJob = std::move(job);
    st.lastBackground = kBackgroundSun;
    return ARK_DDGI_OK;
}

// The world BVHs' background rebuild after refits (the reference's full TLAS build every
// 60 frames restores tightness, GpuScene.cpp:998-1010; a refit keeps the old topology,
// whose boxes loosen as instances move): a finished rebuild is installed on `s` -
// behind the frames that may read the old BVHs, its shading records gathered into its
// record order, and refitted forward when refits came in while it was built - and,
// while refits have loosened the installed one, a new one is started (worldStart).
int worldCollect(SceneStore& st, const SceneCall& c, hipStream_t s)
{
    ErrorSink* err = c.err;
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
            err->lastError = "background BVH rebuild failed: " + job->error;
            return ARK_DDGI_OK;
        }
        ARK_HIP(sharedBegin(c));
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
        return finishInstall(st, c, st.refitsSinceBuild, s);
    }
    return ARK_DDGI_OK;
}

int worldStart(SceneStore& st, const SceneCall& c, hipStream_t s, bool gpu)
{
    ErrorSink* err = c.err;
    auto job = std::make_unique<WorldJob>();
    job->version = st.version;
    job->refitsAt = st.refitCount;
    job->snapRecords = st.world.records;
    job->classOf = instanceClasses(st);
    ARK_HIP(snapshotRecords(st, job->snap, job->evSnap, s));
    // half the host threads: the other half stays with the frames being enqueued meanwhile
    job->t = std::thread(gpu ? runWorldJobGpu : runWorldJob, job.get(), st.device, std::max(1, st.buildThreads / 2));
    st.worldJob = std::move(job);
    st.lastBackground = kBackgroundWorld;
    st.refitsSinceBuild = 0;
    return ARK_DDGI_OK;
}

// The background build to start now (rebuildToStart over the store's state, the finished
// jobs collected), started on `s`
int startRebuild(SceneStore& st, const SceneCall& c, hipStream_t s, bool sunOnly)
{
    RebuildState q;
    q.sunWanted = st.sunWanted;
    q.hasSun = c.hasSun;
    q.sunJobRunning = static_cast<bool>(st.sunJob);
    q.worldJobRunning = static_cast<bool>(st.worldJob);
    q.sunInstalled = st.sunArgs.sun_root >= 0 && sameDir(c.sunDir, st.sunDirBuilt);
    q.requestStable = st.sunReqStreak >= 2 && sameDir(st.sunReqDir, c.sunDir);
    q.sunFailedHere = st.sunFailed && st.sunFailedVersion == st.version && sameDir(st.sunFailedDir, c.sunDir);
    q.worldRebuildFailed = st.worldRebuildFailed;
    q.worldGpuBuilt = st.worldGpuBuilt;
    q.sunGpuBuilt = st.sunGpuBuilt && q.sunInstalled;
    q.refitsSinceBuild = st.refitsSinceBuild;
    q.sunRefitsSinceBuild = st.sunRefitsSinceBuild;
    q.flags = c.flags;
    q.lastBackground = st.lastBackground;
    q.sunOnly = sunOnly;
    switch (rebuildToStart(q)) {
    case RebuildStart::Sun: return sunStart(st, c, s, false);
    case RebuildStart::SunDevice: return sunStart(st, c, s, true);
    case RebuildStart::WorldHost: return worldStart(st, c, s, false);
    case RebuildStart::WorldDevice: return worldStart(st, c, s, true);
    case RebuildStart::None: break;
    }
    return ARK_DDGI_OK;
}

} // namespace

int sceneMaintenance(SceneStore& st, const SceneCall& c, hipStream_t s)
{
    collectRetired(st);
    if (const int rc = worldCollect(st, c, s)) return rc;
    if (const int rc = sunCollect(st, c, s, true)) return rc;
    return startRebuild(st, c, s, false);
}

bool sunStepMayEnqueue(const SceneStore& st, const SceneCall& c)
{
    return st.sunWanted && c.hasSun && (st.sunJob ? st.sunJob->done.load(std::memory_order_acquire) : true);
}

bool sunJobPending(const SceneStore& st) { return static_cast<bool>(st.sunJob); }

int sceneSunStep(SceneStore& st, const SceneCall& c, hipStream_t s, bool mayEnqueue)
{
    if (const int rc = sunCollect(st, c, s, mayEnqueue)) return rc;
    return mayEnqueue ? startRebuild(st, c, s, true) : ARK_DDGI_OK;
}

namespace {

// ark_ddgi_set_scene's steps, in the order they run

int validateScene(ErrorSink* err,const ArkDdgiScene* s)
{
    for (uint32_t i = 0; i < s->instance_count; ++i) {
        const ArkRTInstance& inst = s->instances[i];
        if (inst.rt_mesh_index >= s->mesh_count) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u: rt_mesh_index out of range", i);
        const ArkRTTriangleMesh& m = s->meshes[inst.rt_mesh_index];
        if (m.material_index < 0 || static_cast<uint32_t>(m.material_index) >= s->material_count)
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "mesh %u: material_index out of range", inst.rt_mesh_index);
        if (static_cast<uint64_t>(m.first_index) + 3ull * inst.triangle_count > s->index_count)
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u: indices out of range", i);
    }
    if (s->spot_light_count > ARK_DDGI_MAX_SPOT_LIGHTS || (s->spot_light_count && !s->spot_lights))
        return err->fail(ARK_DDGI_E_UNSUPPORTED, "at most %d spot lights (GpuScene.cpp:430)", ARK_DDGI_MAX_SPOT_LIGHTS);
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
int flattenInstances(ErrorSink* err,const ArkDdgiScene* s, std::vector<BuildTriangle> cls[3], std::vector<GpuInstance>& ginst)
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
                if (vi >= s->vertex_count) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u prim %u: vertex out of range", ii, p);
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
int decodeTextures(ErrorSink* err,const ArkDdgiScene* s, std::vector<GpuTextureInfo>& infos, std::vector<float>& texels)
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
            if (t.width <= 0 || t.height <= 0 || !t.data) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u invalid", i);
            ti.width = t.width;
            ti.height = t.height;
            // per-axis wrap, s in bits 0-3 and t in 4-7 (ARK_WRAP_AXES)
            const int ws = (t.wrap & ARK_WRAP_PER_AXIS) ? (t.wrap & 0xf) : t.wrap, wt = (t.wrap & ARK_WRAP_PER_AXIS) ? ((t.wrap >> 4) & 0xf) : t.wrap;
            if (ws < ARK_WRAP_REPEAT || ws > ARK_WRAP_MIRRORED_REPEAT || wt < ARK_WRAP_REPEAT || wt > ARK_WRAP_MIRRORED_REPEAT ||
                ((t.wrap & ARK_WRAP_PER_AXIS) && (t.wrap & ~0x1ff)))
                return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u: unknown wrap mode 0x%x", i, t.wrap);
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
                    default: return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u: unknown format", i);
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

// the store's refit stream and the events that order its copies (scene_store.h)
hipError_t createOrdering(SceneStore& st)
{
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&st.refitStream, hipStreamNonBlocking, hi);
    for (hipEvent_t* ev : { &st.evFree[0], &st.evFree[1], &st.evFree[2], &st.evInstalled, &st.evGeometry })
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    return e;
}

} // namespace

SceneStore::SceneStore() = default;

SceneStore::~SceneStore()
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
    for (hipEvent_t ev : { evFree[0], evFree[1], evFree[2], evInstalled, evGeometry })
        if (ev) (void)hipEventDestroy(ev);
    if (refitStream) (void)hipStreamDestroy(refitStream);
    world.release();
    sun.release();
    for (DeviceBuffer* b : { &triNormals, &indices, &vertices, &positions, &meshes, &materials, &instances, &texInfos, &texels, &refitInst, &spare[0].world,
                             &spare[0].sun, &spare[0].instances, &spare[1].world, &spare[1].sun, &spare[1].instances })
        b->release();
}

int buildScene(ErrorSink* err, const ArkDdgiScene* s, int device, int buildThreads, int sunBvh, std::shared_ptr<SceneStore>& out)
{
    auto st = std::make_shared<SceneStore>();
    st->device = device;
    ARK_HIP(createOrdering(*st));
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    if ((rc = validateScene(err, s)) != 0) return rc;
    std::vector<BuildTriangle> cls[3];
    std::vector<GpuInstance> ginst;
    if ((rc = flattenInstances(err, s, cls, ginst)) != 0) return rc;
    // host threads for the build (ArkDdgiDesc.build_threads; 0: the box's CPU share per
    // GPU, 16 cores)
    BvhBuildOptions opt;
    opt.threads = buildThreads > 0 ? buildThreads : 16;
    // BVH2 -> BVH8 child selection: SAH-optimal (Ylitie et al. 2017 DP) with the default
    // node / triangle costs (a lower triangle cost and the greedy collapse measured no
    // better)
    Bvh8CollapseOptions copt;
    copt.threads = opt.threads;
    // the sun's light-space BVH input, before the class builds free their triangles; the
    // build itself on its own thread beside the class builds (each build's top levels
    // leave cores idle: C4 setup 13.5 -> s)
    const bool sunInput = s->has_directional_light && sunBvh != 0;
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
    if (sunInput) {
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
    if (!build_world_bvh8(cls, opt, copt, w, why)) return err->fail(w.tooLarge ? ARK_DDGI_E_UNSUPPORTED : ARK_DDGI_E_DEVICE, "%s", why.c_str());
    std::vector<GpuTextureInfo> infos;
    std::vector<float> texels;
    if ((rc = decodeTextures(err, s, infos, texels)) != 0) return rc;
    std::vector<GpuSpotLight> gspots(s->spot_light_count);
    for (uint32_t i = 0; i < s->spot_light_count; ++i) gspots[i] = gpuSpotLight(s->spot_lights[i]);
    // (the traversal's 32-bit byte offset: nodes and records must stay below 4 GiB)
    if (DeviceBvh::bytesFor(w.nodes.size(), w.tris.size()) >= (1ull << 32)) return err->fail(ARK_DDGI_E_UNSUPPORTED, "BVH nodes + triangles exceed 4 GiB");
    ARK_HIP(uploadBvh(w.nodes, w.tris, nullptr, st->world));
    st->world.depth = w.depth;
    st->world.inflateAbs = w.inflateAbs;
    if (sunThread.t.joinable()) sunThread.t.join();
    const auto ts0 = std::chrono::steady_clock::now();
    const int32_t sroot = 0;
    if (sunBuilt) {
        if (!sunOk) return err->fail(ARK_DDGI_E_DEVICE, "sun BVH2 leaf over %d triangles", kBvh8MaxLeafSize);
        if (!checkBvh8Structure(r.nodes, r.tris, &sroot, 1, why)) return err->fail(ARK_DDGI_E_DEVICE, "%s", why.c_str());
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
    if (sunBuilt && (sunBvh == 1 ||sun_bvh_pays(st->sunCostWorld, st->sunCostLight))) {
        DeviceBvh sb;
        std::vector<uint32_t> order;
        if (!bvhLevelOrder(r.nodes.data(), r.nodes.size(), &sroot, 1, order, sb.levelOffsets)) return err->fail(ARK_DDGI_E_DEVICE, "sun BVH: a node outside it");
        sb.depth = r.max_depth;
        sb.inflateAbs = sunIn.inflateAbs;
        if ((rc = installSunBvh(err, *st, sb, &r, order, &sunIn.frame[0][0], s->directional_light.world_space_direction, nullptr)) != 0) return rc;
    }
    sunBuildMs += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - ts0).count();
    std::vector<GpuTriangle>().swap(sunIn.world);
    if ((rc = upload(err, st->indices, s->indices, s->index_count)) != 0) return rc;
    if ((rc = upload(err, st->vertices, reinterpret_cast<const float*>(s->vertices), s->vertex_count * 9)) != 0) return rc;
    if ((rc = upload(err, st->positions, s->positions, s->vertex_count * 3)) != 0) return rc;
    st->instHost.assign(s->instances, s->instances + s->instance_count);
    // the transforms both geometry copies hold (the back one is made at the first refit)
    st->xf[0].resize(s->instance_count);
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) std::memcpy(st->xf[0][ii].data(), s->instances[ii].object_to_world, sizeof(float) * 12);
    st->xf[1] = st->xf[2] = st->xf[0];
    st->spare[0].slot = 1;
    st->spare[1].slot = 2;
    st->meshHost.assign(s->meshes, s->meshes + s->mesh_count);
    instanceObjectBoxes(s, opt.threads, st->instObjBox);
    if ((rc = upload(err, st->meshes, s->meshes, s->mesh_count)) != 0) return rc;
    if ((rc = upload(err, st->materials, s->materials, s->material_count)) != 0) return rc;
    if ((rc = upload(err, st->instances, ginst.data(), ginst.size())) != 0) return rc;
    if ((rc = upload(err, st->texInfos, infos.data(), infos.size())) != 0) return rc;
    if ((rc = upload(err, st->texels, texels.data(), texels.size())) != 0) return rc;
    {
        std::vector<float> tn;
        shadingRecords(s, w.tris, opt.threads, tn);
        if ((rc = upload(err, st->triNormals, tn.data(), tn.size())) != 0) return rc;
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
    out = std::move(st);
    return ARK_DDGI_OK;
}

namespace {

// ark_ddgi_set_instances' first use of a scene: the world BVHs' nodes by depth, deepest
// first, and the refit's work buffers (a topology download: refits never change it)
int prepareRefit(ErrorSink* err, SceneStore& st)
{
    DeviceBvh& w = st.world;
    const uint64_t n = w.nodeCount;
    std::vector<GpuBvh8Node> h(n);
    if (n) ARK_HIP(hipMemcpy(h.data(), w.buf.ptr, n * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost));
    const int32_t roots[3] = { st.args.root_opaque, st.args.root_masked, st.args.root_blend };
    std::vector<uint32_t> order;
    if (!bvhLevelOrder(h.data(), n, roots, 3, order, w.levelOffsets)) return err->fail(ARK_DDGI_E_DEVICE, "refit: a node outside the BVH");
    int rc;
    if ((rc = upload(err, w.order, order.data(), order.size())) != 0) return rc;
    ARK_HIP(w.boxes.alloc(std::max<size_t>(16, n * 6 * sizeof(float))));
    return ARK_DDGI_OK;
}

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

// The refit proper: the target spare st.spare[0] brought to `instances` on the refit
// stream (copied from the front copy first when it holds nothing valid: a new scene or an
// installed rebuild; what it replaces retired behind `last`). Any failure in here leaves
// the spare's contents unknown (sceneSetInstances).
int refitSpare(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t last)
{
    ErrorSink* err = c.err;
    SceneStore::Spare& tgt = st.spare[0];
    const int fs = st.front, ts = tgt.slot;
    const hipStream_t rs = st.refitStream;
    if (!tgt.valid) {
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
    int rc;
    if ((rc = uploadRefitInstances(err, st, instances, count, &st.xf[ts], rs)) != 0) return rc;
    if ((rc = enqueueRefit(err, st, rs, tgt.world, tgt.sun, ts)) != 0) return rc;
    ARK_HIP(geometryChanged(st, rs));
    ARK_HIP(sharedEnd(c, rs));
    return ARK_DDGI_OK;
}

} // namespace

int sceneSetInstances(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t s)
{
    ErrorSink* err = c.err;
    if (count != st.instHost.size() || (count && !instances))
        return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: %u instances, the scene has %zu", count, st.instHost.size());
    for (uint32_t i = 0; i < count; ++i) {
        const ArkRTInstance &a = instances[i], &b = st.instHost[i];
        if (a.rt_mesh_index != b.rt_mesh_index || a.triangle_count != b.triangle_count || a.hit_mask != b.hit_mask)
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: instance %u changed its mesh, triangle count or hit mask (a set_scene builds a new scene)", i);
        for (float v : a.object_to_world)
            if (!std::isfinite(v)) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: instance %u: non-finite transform", i);
    }
    ARK_HIP(sharedBegin(c));
    int rc;
    if (st.world.levelOffsets.empty() && (rc = prepareRefit(err, st)) != 0) return rc;
    // Everything the calling context enqueued so far ends on `s` (the precondition): the
    // front copy's readers among them. The events that mark that point are recorded on `s`
    // - not on the last operation's stream, which the caller may have destroyed since,
    // nor on a stream of the context's own (one more stream on the process's few hardware
    // queues; measured no better under motion, profiles/r06_ab2_refit_ordering/).
    // A light-space sun BVH without a refit order (none recorded) cannot follow: dropped
    if (st.sunArgs.sun_root >= 0 && st.sun.levelOffsets.empty()) {
        st.sunArgs.sun_root = -1;
        st.sunArgs.sun_nodes = nullptr;
        st.sunArgs.sun_tris = nullptr;
        ARK_HIP(retireBuffer(st, st.sun.buf, s));
        ARK_HIP(dropSpares(st, s));
        st.sun.nodeCount = 0;
        st.bvhStats.sun_node_count = 0;
        st.bvhStats.sun_max_depth = 0;
        st.sunGpuBuilt = false;
        st.bvhStats.sun_installed_builder = 0;
    }
    // The refit writes the next spare copy on the refit stream, after the operations that
    // read it (while it was the front one: evFree) and the last install; the frames in
    // flight keep reading the front copy. The copy swapped out here is free once the
    // operations enqueued so far are done.
    SceneStore::Spare& tgt = st.spare[0];
    const int fs = st.front, ts = tgt.slot;
    ARK_HIP(hipEventRecord(st.evFree[fs], s));
    st.freeValid[fs] = true;
    if (st.freeValid[ts]) ARK_HIP(hipStreamWaitEvent(st.refitStream, st.evFree[ts], 0));
    if (st.installValid) {
        ARK_HIP(hipStreamWaitEvent(st.refitStream, st.evInstalled, 0));
        st.installValid = false;
    }
    if ((rc = refitSpare(st, c, instances, count, s)) != 0) {
        // the spare may be half written and xf / inflCopy no longer describe it: the next
        // refit copies the front one anew and reaches every node
        tgt.valid = false;
        st.refitFull = true;
        return rc;
    }
    // the refitted copy becomes the front one
    st.xf[ts].resize(count);
    for (uint32_t ii = 0; ii < count; ++ii) std::memcpy(st.xf[ts][ii].data(), instances[ii].object_to_world, sizeof(float) * 12);
    rotateGeometry(st);
    // the caller's stream follows the refit (what it runs next sees the new geometry); the
    // contexts' next traversals on their traversal streams wait for it too (geometrySeq)
    ARK_HIP(hipStreamWaitEvent(s, st.evGeometry, 0));
    for (uint32_t ii = 0; ii < count; ++ii) std::memcpy(st.instHost[ii].object_to_world, instances[ii].object_to_world, sizeof(float) * 12);
    ++st.version;
    ++st.refitsSinceBuild;
    ++st.sunRefitsSinceBuild;
    st.bvhStats.refit_version = ++st.refitCount;
    // background rebuilds of the loosened BVHs (world and light-space), from a snapshot
    // taken on s behind this refit
    return sceneMaintenance(st, c, s);
}

int sceneDigest(const SceneStore& st, ErrorSink* err, uint64_t* out)
{
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

int sceneWorldBvhCheck(const SceneStore& st, ErrorSink* err, uint64_t* out)
{
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
    if (c.violations) err->lastError = "world BVH check: " + std::to_string(c.violations) + " violations" + (why.empty() ? "" : " (" + why + ")");
    return c.violations ? 1 : ARK_DDGI_OK;
}

int sceneSunBvhCheck(const SceneStore& st, ErrorSink* err, uint64_t* out)
{
    std::fill(out, out + 8, uint64_t(0));
    if (st.sunArgs.sun_root < 0 || !st.sun.nodeCount) return 1; // no light-space BVH
    std::vector<GpuBvh8Node> nodes(st.sun.nodeCount);
    std::vector<GpuTriangle> tris(st.sun.records);
    std::vector<uint32_t> order(nodes.size());
    ARK_HIP(hipMemcpy(nodes.data(), st.sunArgs.sun_nodes, nodes.size() * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost));
    if (!tris.empty()) ARK_HIP(hipMemcpy(tris.data(), st.sunArgs.sun_tris, tris.size() * sizeof(GpuTriangle), hipMemcpyDeviceToHost));
    if (st.sun.order.bytes >= order.size() * 4) ARK_HIP(hipMemcpy(order.data(), st.sun.order.ptr, order.size() * 4, hipMemcpyDeviceToHost));
    const int32_t root = 0;
    // (one tree for every class: classOf unchecked; the boxes hold light coordinates)
    Bvh8CheckResult c = check_bvh8_full(nodes, tris, &root, 1, nullptr, nullptr, st.sunFrameD);
    std::string why;
    if (!checkBvh8Structure(nodes, tris, &root, 1, why)) c.violations++;
    if (c.nodes != nodes.size()) c.violations++; // a node outside the tree
    if (st.sunGpuBuilt) c.violations += c.notBreadthFirst; // the device build's order
    std::vector<uint32_t> wantOrder, wantOffsets;
    if (!bvhLevelOrder(nodes.data(), nodes.size(), &root, 1, wantOrder, wantOffsets)) {
        c.violations++;
    } else if (wantOrder != order || wantOffsets != st.sun.levelOffsets) {
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
    out[7] = st.sunGpuBuilt ? 1u : 0u;
    if (c.violations) err->lastError = "sun BVH check: " + std::to_string(c.violations) + " violations" + (why.empty() ? "" : " (" + why + ")");
    return c.violations ? 1 : ARK_DDGI_OK;
}

} // namespace ark

// ark_ddgi_debug.h: one traced device build (buildLbvhGpu, the product's kernels and
// nothing else) of the given records on a stream of its own, without a context, against
// build_lbvh_host of the same records in the device's compaction order, stage by stage.
extern "C" int ark_ddgi_debug_lbvh_device_parity(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                                  const float* sun_dir, int w_bits, uint64_t* out)
{
    using namespace ark;
    if (!records || !class_of || !out || n_records == 0 || n_records > 0x7fffffffull || n_instances == 0) return -1;
    std::fill(out, out + 32, uint64_t(0));
    for (uint32_t i = 0; i < n_instances; ++i)
        if (class_of[i] < 0 || class_of[i] > 2) return -1; // (the kernels index the class counts by it)
    int wBits = lbvh::kMortonBits;
    if (sun_dir) {
        wBits = w_bits < 0 ? lbvh::kSunKeyBitsW : w_bits;
        if (wBits > lbvh::kMortonBits || (wBits & 1)) return -1;
    }
    const uint32_t n = static_cast<uint32_t>(n_records);
    std::vector<GpuTriangle> rec(n);
    std::memcpy(rec.data(), records, n * sizeof(GpuTriangle));

    // the device build
    struct Device {
        hipStream_t s = nullptr;
        hipEvent_t ev = nullptr;
        DeviceBuffer snap, perm;
        DeviceBvh bvh;
        ~Device()
        {
            if (s) (void)hipStreamSynchronize(s);
            bvh.release();
            perm.release();
            snap.release();
            if (ev) (void)hipEventDestroy(ev);
            if (s) (void)hipStreamDestroy(s);
        }
    } d;
    LbvhGpuTrace trace;
    LbvhGpuBuild g;
    std::string why;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d.s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d.ev, hipEventDisableTiming);
    if (e == hipSuccess) e = d.snap.alloc(std::max<size_t>(16, n * sizeof(GpuTriangle)));
    if (e == hipSuccess) e = hipMemcpyAsync(d.snap.ptr, rec.data(), n * sizeof(GpuTriangle), hipMemcpyHostToDevice, d.s);
    if (e == hipSuccess) e = hipEventRecord(d.ev, d.s);
    if (e == hipSuccess) {
        g.snap = d.snap.as<GpuTriangle>();
        g.evSnap = d.ev;
        g.records = n;
        g.classHost.assign(class_of, class_of + n_instances);
        if (sun_dir) {
            double frame[3][3];
            sun_frame(sun_dir, frame);
            g.light = true;
            std::memcpy(g.frame, frame, sizeof(g.frame));
            g.slotRule = lbvh::kSlotsAscendingW;
            g.wBits = wBits;
        }
        g.bvh = &d.bvh;
        g.perm = &d.perm;
        g.trace = &trace;
        e = buildLbvhGpu(g, d.s, why);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d.s);
    out[26] = static_cast<uint64_t>(e);
    if (e != hipSuccess) return -5;
    static const char* const kWhy[] = { "", "no records", "no triangles", "record of an unknown instance", "BVH8 deeper than the device build installs",
                                        "more nodes than the device build's scratch", "nodes and records of 4 GiB or more" };
    out[4] = 7;
    for (uint64_t k = 0; k < sizeof(kWhy) / sizeof(kWhy[0]); ++k)
        if (trace.why == kWhy[k]) out[4] = k;
    out[0] = trace.hdr.prims;
    if (!trace.why.empty() || !trace.built) return 2; // the host's scene: nothing was built

    // the compaction: a permutation of exactly the records that are not holes
    std::vector<uint32_t> live;
    for (uint32_t i = 0; i < n; ++i)
        if (!isHoleTriangle(rec[i])) live.push_back(i);
    {
        std::vector<uint32_t> sorted = trace.idx;
        std::sort(sorted.begin(), sorted.end());
        out[5] = sorted.size() != live.size() ? 1u : 0u;
        for (size_t j = 0; j < std::min(sorted.size(), live.size()); ++j) out[5] += sorted[j] != live[j] ? 1u : 0u;
    }
    if (sun_dir && !out[5] && !live.empty()) {
        // k_lbvh_prims_light: a wave's survivors one run, ascending
        uint64_t runs = 1, waves = 1;
        for (size_t j = 0; j + 1 < trace.idx.size(); ++j) {
            if ((trace.idx[j] >> 6) != (trace.idx[j + 1] >> 6)) runs++;
            else if (trace.idx[j] >= trace.idx[j + 1]) out[6]++;
            if ((live[j] >> 6) != (live[j + 1] >> 6)) waves++;
        }
        if (runs != waves) out[6]++;
    }
    std::vector<int> classOf(class_of, class_of + n_instances);
    LbvhSunOptions so;
    std::memcpy(so.frame, g.frame, sizeof(so.frame));
    so.wBits = wBits;
    const LbvhHostResult r = build_lbvh_host(rec, classOf, lbvh::kDefaultCriterion, sun_dir ? &so : nullptr, out[5] ? nullptr : &trace.idx);
    auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    // the header
    const uint32_t prims = static_cast<uint32_t>(live.size());
    out[7] = (trace.hdr.prims != prims ? 1u : 0u) + (trace.hdr.error ? 1u : 0u);
    for (int c = 0; c < 3; ++c) out[7] += trace.hdr.classCount[c] != r.classCount[c] ? 1u : 0u;
    for (int k = 0; k < 3; ++k) {
        // (== of floats: the ordered-bits atomics tell -0 from +0, std::min does not, and nothing later depends on a zero's sign)
        out[8] += lbvhOrderedFloat(trace.hdr.lo[k]) == r.sceneLo[k] ? 0u : 1u;
        out[8] += lbvhOrderedFloat(trace.hdr.hi[k]) == r.sceneHi[k] ? 0u : 1u;
    }
    out[9] = trace.hdr.maxAbs != bits(r.maxAbs) ? 1u : 0u;
    out[10] = bits(trace.inflateAbs) != bits(r.inflateAbs) ? 1u : 0u;
    // keys, sorted records, splits
    if (trace.keysSorted.size() != prims || trace.idxSorted.size() != prims || trace.split.size() != prims || r.keysSorted.size() != prims) {
        out[11] = out[12] = out[13] = 1;
    } else {
        for (uint32_t j = 0; j < prims; ++j) {
            out[11] += trace.keysSorted[j] != r.keysSorted[j] ? 1u : 0u;
            out[12] += trace.idxSorted[j] != r.idxSorted[j] ? 1u : 0u;
        }
        uint32_t first = 0;
        for (int c = 0; c < 3; ++c) {
            for (uint32_t i = first; i + 1u < first + r.classCount[c]; ++i) out[13] += trace.split[i] != r.split[i] ? 1u : 0u;
            first += r.classCount[c];
        }
    }
    // the tree
    const GpuTriangle padding = trace.tris.back(); // (records + 1 entries)
    trace.tris.pop_back();
    Bvh8TreeView dv, hv;
    dv.nodes = &trace.nodes;
    dv.tris = &trace.tris;
    dv.perm = &trace.perm;
    dv.order = &trace.order;
    dv.levelOffsets = &trace.levelOffsets;
    dv.padding = &padding;
    std::copy(trace.roots, trace.roots + 3, dv.roots);
    dv.opaqueNodes = trace.opaqueNodes;
    dv.depth = trace.depth;
    hv.nodes = &r.nodes;
    hv.tris = &r.tris;
    hv.perm = &r.perm;
    hv.order = &r.order;
    hv.levelOffsets = &r.levelOffsets;
    std::copy(r.roots, r.roots + 3, hv.roots);
    hv.opaqueNodes = r.opaqueNodes;
    hv.depth = r.depth;
    const Bvh8CanonicalDiff diff = compare_bvh8_canonical(dv, hv);
    out[1] = trace.nodes.size();
    out[2] = trace.tris.size();
    out[3] = trace.depth;
    out[14] = diff.shape;
    out[15] = diff.header;
    out[16] = diff.grid;
    out[17] = diff.planes;
    out[18] = diff.children;
    out[19] = diff.records;
    out[20] = diff.perm;
    out[21] = diff.holes;
    out[22] = diff.levelOrder;
    out[23] = diff.padding;
    out[24] = static_cast<uint64_t>(diff.firstA);
    out[25] = static_cast<uint64_t>(diff.firstB);
    out[27] = diff.pairs;
    out[28] = r.nodes.size();
    uint64_t mismatches = 0;
    for (int k = 5; k <= 23; ++k) mismatches += out[k];
    return mismatches ? 1 : 0;
}
