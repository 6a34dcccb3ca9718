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
#include "bvh8_check.h"
#include "bvh_builder.h"
#include "lbvh_device_build.h"
#include "sun_bvh.h"
#include "sun_cover_build.h"

// (every function here that can fail has an ErrorSink* err in scope)
#define ARK_HIP(expr) ARK_HIP_TO(err, expr)

namespace ark {

// A background rebuild (runRebuildJob), of the world BVHs after refits (worldCollect /
// worldStart; the reference rebuilds its TLAS in full every 60 frames, GpuScene.cpp:998-1010)
// or of the sun's light-space BVH for `dir` (sunCollect / sunStart). A host thread takes a
// device snapshot of the refitted triangle records, taken in stream order behind the refits
// (`snap` / `evSnap`), builds from them and uploads the result into `bvh`, level order
// included; `done` is set last (release).
//  - world: the three hit-mask classes' BVHs anew (set_scene's builder, or the device's),
//    every record's words kept as they were (so hits stay bit-identical), and the new record
//    order's source indices (perm, for the shading records).
//  - sun: the light-space BVH8 over every class's records in `frame`.
struct RebuildJob {
    enum Kind { World, Sun } kind = World;
    std::thread t;
    std::atomic<bool> done { false };
    uint32_t version = 0;  // SceneStore::version of the snapshot
    uint32_t refitsAt = 0; // SceneStore::refitCount of the snapshot (later refits: refitted forward at install)
    DeviceBuffer snap;     // the records it builds from
    hipEvent_t evSnap = nullptr;
    uint64_t snapRecords = 0;
    DeviceBvh bvh;         // the result
    float ms = 0.0f;       // the whole job's wall time (a device attempt that fell back included)
    bool ok = false;
    // the device built the result; or it handed the job to the host build (until counted)
    bool gpu = false, gpuFallback = false;
    // world
    std::vector<int> classOf; // instance -> hit-mask class (0 opaque, 1 masked, 2 blend)
    DeviceBuffer perm;
    int32_t roots[3] { -1, -1, -1 };
    uint32_t opaqueNodes = 0, opaqueRecords = 0, maxLeaf = 0;
    float sah = 0.0f;
    std::string error;
    // sun
    float dir[3] {};
    double frame[9] {};     // sun_frame(dir)
    uint32_t instances = 0; // of the scene (the device build checks the records' against it)
    bool sahPass = false;   // ARK_DDGI_FLAG_GPU_REBUILD_SAH: a device build runs the SAH pass
    bool planPass = false;  // ARK_DDGI_FLAG_GPU_REBUILD_PLAN: and collapses by the plan
    // the sun's cover map of the snapshot (either kind, when the scene keeps one and the
    // caller has a sun): built on the device after the BVH, installed with it when no refit
    // came in since the snapshot
    bool coverWanted = false, coverOk = false;
    float coverDir[3] {};
    double coverFrame[9] {};
    cover::Grid coverGrid {};
    DeviceBuffer coverBuf;
    float coverMs = 0.0f;
    ~RebuildJob()
    {
        if (t.joinable()) t.join();
        bvh.release(); // not installed (an installed one was moved to the scene)
        for (DeviceBuffer* b : { &perm, &snap, &coverBuf }) b->release();
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
// The ring's next slot, free for the host to fill (its last reader, a few calls back, has
// run) and grown to `bytes`; stageRelease records its reader's end on the reader's stream.
hipError_t ringAcquire(void** stage, size_t* stageBytes, hipEvent_t* stageDone, int& next, int slots, size_t bytes, int& slot)
{
    const int i = slot = next;
    next = (i + 1) % slots;
    hipError_t e = hipSuccess;
    if (!stageDone[i] && (e = hipEventCreateWithFlags(&stageDone[i], hipEventDisableTiming)) != hipSuccess) return e;
    if (stageBytes[i]) (void)hipEventSynchronize(stageDone[i]); // its last copy (an earlier frame's) has run
    if (stageBytes[i] < bytes) {
        if (stage[i]) (void)hipHostFree(stage[i]);
        stage[i] = nullptr;
        stageBytes[i] = 0;
        if ((e = hipHostMalloc(&stage[i], bytes, hipHostMallocDefault)) != hipSuccess) return e;
        stageBytes[i] = bytes;
    }
    return hipSuccess;
}

hipError_t stageAcquire(SceneStore& st, size_t bytes, int& slot)
{
    return ringAcquire(st.stage, st.stageBytes, st.stageDone, st.stageNext, SceneStore::kStageSlots, bytes, slot);
}

hipError_t stageRelease(SceneStore& st, int slot, hipStream_t s) { return hipEventRecord(st.stageDone[slot], s); }

// the vertex ranges' ring (SceneStore::vstage)
hipError_t vertexStageAcquire(SceneStore& st, size_t bytes, int& slot)
{
    return ringAcquire(st.vstage, st.vstageBytes, st.vstageDone, st.vstageNext, SceneStore::kVertexStageSlots, bytes, slot);
}

hipError_t vertexStageRelease(SceneStore& st, int slot, hipStream_t s) { return hipEventRecord(st.vstageDone[slot], s); }

hipError_t stagedUpload(SceneStore& st, void* dst, const void* src, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return hipSuccess;
    int i = 0;
    hipError_t e = stageAcquire(st, bytes, i);
    if (e != hipSuccess) return e;
    std::memcpy(st.stage[i], src, bytes);
    if ((e = hipMemcpyAsync(dst, st.stage[i], bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return stageRelease(st, i, s);
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
// hold, `held`: updated - or other than the one the boxes scratch holds, which the refit
// before left there for another copy: a live node reads its skipped children's boxes from it).
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
    args.dirty = (st.refitFull || args.inflate != held || args.inflate != b.boxesInflate) ? ~0ull : dirty;
    b.refitDirty = args.dirty;
    for (size_t l = 0; l + 1 < lv.size(); ++l)
        ARK_HIP(launch_refit_nodes(nodes, tris, b.boxes.as<float>(), order + lv[l], lv[l + 1] - lv[l], args, b.masks.as<uint64_t>(), st.refitInst.as<RefitInstance>(),
                                   st.indices.as<uint32_t>(), st.positions.as<float>(), s));
    held = args.inflate;
    b.boxesInflate = args.inflate;
    return ARK_DDGI_OK;
}

// The refit of the copy (`world`, `sun`; slot: the transforms and inflations it holds) of
// every BVH of the scene on `s`: the records of the moved instances (st.refitInst's dirty
// flags: those whose transform differs from the copy's or the refit before's) re-transformed, the boxes and
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
// whose transform differs from the one the target copy's records hold (`have`) or from
// the refit before's (st.instHost). The second keeps the boxes scratch, which the three
// copies share, current: a node is skipped only when nothing below it changed since the
// scratch last saw it, whichever copy that refit wrote. An instance back at the pose the
// target copy holds (a nudge and return, a loop of period 3) is re-transformed to the
// same bits. Vertices count as transforms do: an instance whose vertices are newer than the
// target copy's records (`slot`) or than the refit before's is dirty (st.vtx, vertex_dirty.h).
int uploadRefitInstances(ErrorSink* err, SceneStore& st, const ArkRTInstance* instances, uint32_t count, const std::vector<std::array<float, 12>>* have, int slot,
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
        const bool moved = allDirty || std::memcmp((*have)[ii].data(), M, sizeof(q.m)) != 0 || std::memcmp(st.instHost[ii].object_to_world, M, sizeof(q.m)) != 0 ||
                           st.vtx.dirty(ii, slot);
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

// What a host build hands to the upload (hostBuild)
struct HostBvh {
    std::vector<GpuBvh8Node> nodes;
    std::vector<GpuTriangle> tris;
    std::vector<uint32_t> perm, order;
};

// The world rebuild on the host: the three classes' BVHs from the snapshot's records (their
// vertices v0, v0 + e1, v0 + e2; each leaf record then replaced by its source record,
// bit for bit), the record order's source indices and the refit's level order.
bool hostBuildWorld(RebuildJob* job, const std::vector<GpuTriangle>& rec, int threads, HostBvh& out)
{
    std::vector<BuildTriangle> cls[3];
    for (size_t i = 0; i < rec.size(); ++i) {
        const GpuTriangle& g = rec[i];
        if (isHoleTriangle(g)) continue;
        uint32_t inst, flip;
        std::memcpy(&inst, &g.t2[1], 4);
        std::memcpy(&flip, &g.t2[3], 4);
        if (inst >= job->classOf.size()) {
            job->error = "record of an unknown instance";
            return false;
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
    WorldBvh8 w;
    BvhBuildOptions opt;
    opt.threads = threads;
    Bvh8CollapseOptions copt;
    copt.threads = threads;
    const bool ok = build_world_bvh8(cls, opt, copt, w, job->error);
    if (w.maxLeaf > static_cast<uint32_t>(kBvh8MaxLeafSize)) job->error = "BVH2 leaf over the leaf size";
    if (!ok) return false;
    out.perm.assign(w.tris.size(), 0xffffffffu);
    for (size_t i = 0; i < w.tris.size(); ++i) {
        GpuTriangle& g = w.tris[i];
        if (isHoleTriangle(g)) continue;
        uint32_t src;
        std::memcpy(&src, &g.t2[2], 4);
        out.perm[i] = src;
        g = rec[src];
    }
    std::copy(w.roots, w.roots + 3, job->roots);
    job->opaqueNodes = w.opaqueNodes;
    job->opaqueRecords = w.opaqueRecords;
    job->maxLeaf = w.maxLeaf;
    job->sah = w.sah;
    job->bvh.depth = w.depth;
    out.nodes.swap(w.nodes);
    out.tris.swap(w.tris);
    return bvhLevelOrder(out.nodes.data(), out.nodes.size(), job->roots, 3, out.order, job->bvh.levelOffsets);
}

// The sun rebuild on the host: the light-space BVH of job->dir from the snapshot's records
// (as set_scene builds it; `rec` freed once the builder has its input) and its level order.
bool hostBuildSun(RebuildJob* job, std::vector<GpuTriangle>& rec, int threads, HostBvh& out)
{
    SunBvhInput in;
    std::memcpy(in.frame, job->frame, sizeof(in.frame));
    sun_add_records(in, rec, threads);
    std::vector<GpuTriangle>().swap(rec);
    BvhBuildOptions opt;
    opt.threads = threads;
    Bvh8CollapseOptions copt;
    copt.threads = threads;
    Bvh8BuildResult r;
    const bool ok = build_sun_bvh(in, opt, copt, r) && !r.nodes.empty();
    job->bvh.inflateAbs = in.inflateAbs;
    job->bvh.depth = r.max_depth;
    out.nodes.swap(r.nodes);
    out.tris.swap(r.tris);
    const int32_t root = 0;
    return ok && bvhLevelOrder(out.nodes.data(), out.nodes.size(), &root, 1, out.order, job->bvh.levelOffsets);
}

// A job's host build on `s`: the snapshot downloaded, the kind's builder, the result
// uploaded into job->bvh (the world's perm with it).
bool hostBuild(RebuildJob* job, hipStream_t s, int threads)
{
    const bool world = job->kind == RebuildJob::World;
    bool ok = s && hipEventSynchronize(job->evSnap) == hipSuccess; // (no stream: the job's device could not be used)
    std::vector<GpuTriangle> rec(ok ? job->snapRecords : 0);
    ok = ok && hipMemcpyAsync(rec.data(), job->snap.ptr, rec.size() * sizeof(GpuTriangle), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) job->error = "snapshot download failed";
    HostBvh h;
    ok = ok && (world ? hostBuildWorld(job, rec, threads, h) : hostBuildSun(job, rec, threads, h));
    if (ok) {
        ok = (!world || (DeviceBvh::bytesFor(h.nodes.size(), h.tris.size()) < (1ull << 32) && job->perm.alloc(std::max<size_t>(16, h.perm.size() * 4)) == hipSuccess)) &&
             job->bvh.order.alloc(std::max<size_t>(16, h.order.size() * 4)) == hipSuccess &&
             (!world || hipMemcpyAsync(job->perm.ptr, h.perm.data(), h.perm.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess) &&
             hipMemcpyAsync(job->bvh.order.ptr, h.order.data(), h.order.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess && uploadBvh(h.nodes, h.tris, s, job->bvh) == hipSuccess;
        if (!ok && job->error.empty()) job->error = "upload failed";
    }
    return ok;
}

// What the two device builds differ in (LbvhGpuBuild): the world's three class ranges and
// its perm; the sun's one LBVH over every class's records, keyed and boxed in the sun's
// frame, its slots in ascending w.
void deviceBuildWorld(RebuildJob* job, LbvhGpuBuild& g)
{
    g.classHost.assign(job->classOf.begin(), job->classOf.end());
    g.perm = &job->perm;
    g.sah = job->sahPass;
    g.plan = job->planPass;
}

void deviceBuildSun(RebuildJob* job, LbvhGpuBuild& g)
{
    g.classHost.assign(job->instances, 0u); // one tree: only the instance count matters
    g.light = true;
    std::memcpy(g.frame, job->frame, sizeof(g.frame));
    g.slotRule = lbvh::kSlotsAscendingW;
    g.wBits = lbvh::kSunKeyBitsW;
    g.sah = job->sahPass;
    g.plan = job->planPass;
}

// A job's device build on `s` (lbvh_device_build.h; ARK_DDGI_FLAG_GPU_REBUILD / _SUN), which
// waits for the snapshot on the device: buildLbvhGpu's result and `why` into the job.
hipError_t deviceBuild(RebuildJob* job, hipStream_t s, std::string& why)
{
    if (job->snapRecords > 0x7fffffffull) {
        why = "no records";
        return hipSuccess;
    }
    const bool world = job->kind == RebuildJob::World;
    LbvhGpuBuild g;
    g.snap = job->snap.as<GpuTriangle>();
    g.evSnap = job->evSnap;
    g.records = static_cast<uint32_t>(job->snapRecords);
    g.bvh = &job->bvh;
    world ? deviceBuildWorld(job, g) : deviceBuildSun(job, g);
    const hipError_t e = buildLbvhGpu(g, s, why);
    if (world) {
        // (inflateAbs: worldCollect sets the installed one's)
        std::copy(g.roots, g.roots + 3, job->roots);
        job->opaqueNodes = g.opaqueNodes;
        job->opaqueRecords = g.opaqueRecords;
        job->maxLeaf = std::min<uint32_t>(g.prims, static_cast<uint32_t>(kBvh8MaxLeafSize));
        job->sah = 0.0f; // not evaluated on the device
    } else {
        job->bvh.inflateAbs = g.inflateAbs;
    }
    return e;
}

// A rebuild job's thread. tryDevice: the device build first, on a stream of the lowest
// priority; what becomes of it is deviceBuildOutcome's (scene_rebuild_policy.h). A scene
// the device build does not take (no records, 4 GiB, depth, node scratch, an error that is
// not a device fault) is built by the host within this job, from the same snapshot; a
// device fault fails the job (the world's: no more rebuilds of this scene; the sun's: not
// retried for this direction and version).
void runRebuildJob(RebuildJob* job, int device, int threads, bool tryDevice)
{
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = nullptr;
    auto openStream = [&](bool lowest) {
        hipError_t e = hipSetDevice(device);
        int least = 0, greatest = 0;
        if (e == hipSuccess && lowest) e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess) e = lowest ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        return e;
    };
    auto closeStream = [&] {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    };
    DeviceBuildOutcome outcome = DeviceBuildOutcome::HostBuild;
    if (tryDevice) {
        std::string why;
        hipError_t e = openStream(true);
        if (e == hipSuccess) e = deviceBuild(job, s, why);
        closeStream();
        outcome = deviceBuildOutcome(e == hipSuccess, isDeviceFault(e), !why.empty());
        if (outcome == DeviceBuildOutcome::Failed) job->error = std::string("device build: ") + hipGetErrorString(e);
        if (outcome == DeviceBuildOutcome::HostBuild) {
            // the partial result dropped
            job->bvh.release();
            job->bvh = DeviceBvh {};
            job->perm.release();
            job->roots[0] = job->roots[1] = job->roots[2] = -1;
            job->opaqueNodes = job->opaqueRecords = 0;
            job->gpuFallback = true;
        }
    }
    bool ok = outcome == DeviceBuildOutcome::Installed;
    job->gpu = ok;
    if (outcome == DeviceBuildOutcome::HostBuild) {
        (void)openStream(false);
        ok = hostBuild(job, s, threads);
        closeStream();
    }
    if (ok && job->coverWanted) {
        // the cover map of the same snapshot, on the device whoever built the BVH (a
        // failure leaves the scene without a map: the sun's rays are all traced)
        const auto tc = std::chrono::steady_clock::now();
        float L[3];
        sunRayDirection(job->coverDir, L);
        if (openStream(true) == hipSuccess && hipEventSynchronize(job->evSnap) == hipSuccess &&
            deviceBuildCoverMap(job->snap.as<GpuTriangle>(), job->snapRecords, job->coverFrame, L, cover::kDefaultBudget, s, job->coverGrid, job->coverBuf,
                                job->coverOk) != hipSuccess)
            job->coverOk = false;
        closeStream();
        job->coverMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tc).count();
    }
    job->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    job->ok = ok;
    job->done.store(true, std::memory_order_release);
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

// (set_scene and every install of world BVHs: the record order is a new one, so the
// contexts' seed caches, which hold record indices, start over - worldTopologySeq)
void setWorldRoots(SceneStore& st, const int32_t roots[3], uint32_t opaqueNodes, uint32_t opaqueRecords)
{
    st.args.root_opaque = roots[0];
    st.args.root_masked = roots[1];
    st.args.root_blend = roots[2];
    st.args.opaque_nodes = opaqueNodes;
    st.args.opaque_tri_first = 0u; // the opaque class is built first
    st.args.opaque_tri_end = roots[0] >= 0 ? opaqueRecords : 0u;
    ++st.worldTopologySeq;
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

// The light-space BVH `b` (its level order on the device, whoever built it) built for the
// sun direction `dir` in `frame` becomes the scene's: its nodes and records uploaded by the
// job (sunCollect: host null), or here from `host` (set_scene, synchronously).
int installSunBvh(ErrorSink* err, SceneStore& st, DeviceBvh& b, Bvh8BuildResult* host, const double* frame, const float* dir, hipStream_t s)
{
    ARK_HIP(replaceBvh(st, st.sun, b, s));
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

// The cover map no longer describes the front copy (a refit, an install): contexts stop
// using it at their next refreshScene (the version moves with every such change), the
// buffer is retired behind the launches that may still read it.
hipError_t clearCoverMap(SceneStore& st, hipStream_t s)
{
    // (the version moves here too: a call that fails further on must not leave a context
    // with the retired buffer's pointer in its kernel view)
    if (st.coverMap.buf.ptr) ++st.version;
    st.coverMap.valid = false;
    return retireBuffer(st, st.coverMap.buf, s);
}

void setCoverMap(SceneStore& st, DeviceBuffer& buf, const cover::Grid& grid, const float* dir, const double* frame, float ms)
{
    SceneStore::CoverMap& cm = st.coverMap;
    cm.buf = buf;
    buf = DeviceBuffer {};
    cm.grid = grid;
    std::memcpy(cm.dir, dir, sizeof(cm.dir));
    for (int k = 0; k < 9; ++k) cm.frame[k] = static_cast<float>(frame[k]);
    cm.valid = true;
    cm.buildMs = ms;
}

// Where an installed job's bookkeeping goes: the world's fields or the sun's
struct InstallBook {
    bool& gpuBuilt;        // SceneStore::worldGpuBuilt / sunGpuBuilt
    uint32_t& refitsSince; // SceneStore::refitsSinceBuild / sunRefitsSinceBuild
    uint32_t &installedBuilder, &gpuRebuilds, &builtRefitVersion; // ArkDdgiBvhStats, as is the build time
    float& buildMs;
};

// The end of an install of `job`'s result on `s` (sunCollect, worldCollect): its builder,
// time and snapshot noted, the new topology refitted forward when refits came in while it
// was built (every instance re-transformed: its records follow them), the spares dropped,
// the next traversal and refit ordered behind it, the scene's version bumped.
int finishInstall(SceneStore& st, const SceneCall& c, RebuildJob& job, InstallBook book, hipStream_t s)
{
    ErrorSink* err = c.err;
    book.buildMs = job.ms;
    book.gpuBuilt = job.gpu;
    book.installedBuilder = job.gpu ? 1u : 0u;
    if (job.gpu) book.gpuRebuilds++;
    const uint32_t refitsSince = book.refitsSince = st.refitCount - job.refitsAt; // refits since its snapshot
    book.builtRefitVersion = job.refitsAt;
    markTopologyChanged(st);
    // the job's cover map is the front copy's when no refit came in since its snapshot (the
    // records it was built from are the ones installed or kept); an older one goes
    if (job.coverOk && refitsSince == 0) {
        ARK_HIP(clearCoverMap(st, s));
        setCoverMap(st, job.coverBuf, job.coverGrid, job.coverDir, job.coverFrame, job.coverMs);
    } else if (refitsSince != 0) {
        ARK_HIP(clearCoverMap(st, s));
    }
    if (refitsSince) {
        if (const int rc = uploadRefitInstances(err, st, st.instHost.data(), static_cast<uint32_t>(st.instHost.size()), nullptr, st.front, s)) return rc;
        if (const int rc = enqueueRefit(err, st, s, st.world.buf, st.sun.buf, st.front)) return rc;
    }
    st.vtx.installed(st.front, refitsSince != 0);
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
        RebuildJob& j = *st.sunJob;
        if (j.gpuFallback) {
            // counted once, however many calls poll the job before the right one installs it
            st.bvhStats.sun_gpu_fallbacks++;
            j.gpuFallback = false;
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
            std::unique_ptr<RebuildJob> job = std::move(st.sunJob);
            job->t.join();
            ARK_HIP(sharedBegin(c));
            if (const int rc = installSunBvh(err, st, job->bvh, nullptr, job->frame, job->dir, s)) return rc;
            ARK_HIP(retireBuffer(st, job->snap, s));
            st.bvhMaxDepth = std::max(st.bvhMaxDepth, st.sun.depth);
            st.bvhStats.max_depth = st.bvhMaxDepth;
            st.bvhStats.sun_node_count = st.sun.nodeCount;
            st.bvhStats.sun_max_depth = st.sun.depth;
            st.bvhStats.sun_rebuilds = ++st.sunRebuilds;
            ArkDdgiBvhStats& b = st.bvhStats;
            return finishInstall(st, c, *job, { st.sunGpuBuilt, st.sunRefitsSinceBuild, b.sun_installed_builder, b.sun_gpu_rebuilds, b.sun_built_refit_version, b.sun_build_ms }, s);
        }
        // else: built for another context's sun, which installs it (or the caller has no
        // ordered stream now: its next call does)
    }
    return ARK_DDGI_OK;
}

// A new job's shared part: the scene's version and refit count, the snapshot on `s`, the
// thread - with half the host threads: the other half stays with the frames being
// enqueued meanwhile.
int launchJob(SceneStore& st, ErrorSink* err, RebuildJob& job, hipStream_t s, bool gpu, bool hasSun, const float* sunDir)
{
    job.version = st.version;
    job.refitsAt = st.refitCount;
    job.snapRecords = st.world.records;
    ARK_HIP(snapshotRecords(st, job.snap, job.evSnap, s));
    job.coverWanted = st.coverWanted && hasSun;
    if (job.coverWanted) {
        std::memcpy(job.coverDir, sunDir, sizeof(job.coverDir));
        double frame[3][3];
        sun_frame(sunDir, frame);
        std::memcpy(job.coverFrame, frame, sizeof(job.coverFrame));
    }
    job.t = std::thread(runRebuildJob, &job, st.device, std::max(1, st.buildThreads / 2), gpu);
    return ARK_DDGI_OK;
}

int sunStart(SceneStore& st, const SceneCall& c, hipStream_t s, bool gpu)
{
    auto job = std::make_unique<RebuildJob>();
    job->kind = RebuildJob::Sun;
    std::memcpy(job->dir, c.sunDir, sizeof(job->dir));
    double frame[3][3];
    sun_frame(job->dir, frame);
    std::memcpy(job->frame, frame, sizeof(job->frame));
    job->instances = static_cast<uint32_t>(st.instHost.size());
    job->sahPass = (c.flags & ARK_DDGI_FLAG_GPU_REBUILD_SAH) != 0;
    job->planPass = (c.flags & ARK_DDGI_FLAG_GPU_REBUILD_PLAN) != 0;
    if (const int rc = launchJob(st, c.err, *job, s, gpu, c.hasSun, c.sunDir)) return rc;
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
        std::unique_ptr<RebuildJob> job = std::move(st.worldJob);
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
        setWorldRoots(st, job->roots, job->opaqueNodes, job->opaqueRecords);
        st.args.tri_normals = st.triNormals.as<float4>();
        st.bvhMaxDepth = std::max(st.world.depth, st.sunArgs.sun_root >= 0 ? st.sun.depth : 0u);
        st.bvhStats.node_count = st.world.nodeCount;
        st.bvhStats.max_depth = st.bvhMaxDepth;
        st.bvhStats.max_leaf_size = job->maxLeaf;
        st.bvhStats.sah_cost = job->sah;
        st.bvhStats.node_bytes = st.world.nodeCount * sizeof(GpuBvh8Node);
        st.bvhStats.triangle_bytes = st.world.records * sizeof(GpuTriangle);
        st.bvhStats.bvh_rebuilds = ++st.worldRebuilds;
        ArkDdgiBvhStats& b = st.bvhStats;
        return finishInstall(st, c, *job, { st.worldGpuBuilt, st.refitsSinceBuild, b.bvh_installed_builder, b.bvh_gpu_rebuilds, b.bvh_built_refit_version, b.bvh_rebuild_ms }, s);
    }
    return ARK_DDGI_OK;
}

int worldStart(SceneStore& st, const SceneCall& c, hipStream_t s, bool gpu)
{
    auto job = std::make_unique<RebuildJob>();
    job->kind = RebuildJob::World;
    job->classOf = instanceClasses(st);
    job->sahPass = (c.flags & ARK_DDGI_FLAG_GPU_REBUILD_SAH) != 0;
    job->planPass = (c.flags & ARK_DDGI_FLAG_GPU_REBUILD_PLAN) != 0;
    if (const int rc = launchJob(st, c.err, *job, s, gpu, c.hasSun, c.sunDir)) return rc;
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

// every instance's object-space box (refitInflations) and every RT mesh's vertex span: the
// largest index any instance of it draws (which instances a vertex update touches)
void instanceObjectBoxes(const ArkDdgiScene* s, int threads, std::vector<std::array<float, 6>>& boxes, std::vector<MeshSpan>& spans)
{
    boxes.assign(s->instance_count, { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY });
    spans.assign(s->mesh_count, MeshSpan {});
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) {
        const ArkRTInstance& in = s->instances[ii];
        const ArkRTTriangleMesh& mesh = s->meshes[in.rt_mesh_index];
        std::array<float, 6>& box = boxes[ii];
        MeshSpan& span = spans[in.rt_mesh_index];
        span.first = mesh.first_vertex;
        std::mutex mu;
        parallelFor(static_cast<size_t>(in.triangle_count) * 3u, threads, [&](size_t b, size_t e) {
            float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
            uint32_t most = 0;
            for (size_t k = b; k < e; ++k) {
                most = std::max(most, s->indices[static_cast<size_t>(mesh.first_index) + k]);
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
            if (e > b) {
                span.maxIndex = std::max(span.maxIndex, most);
                span.used = true;
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
    for (int i = 0; i < kVertexStageSlots; ++i) {
        if (vstage[i]) (void)hipHostFree(vstage[i]);
        if (vstageDone[i]) (void)hipEventDestroy(vstageDone[i]);
    }
    for (hipEvent_t ev : { evFree[0], evFree[1], evFree[2], evInstalled, evGeometry, evPositionsRead })
        if (ev) (void)hipEventDestroy(ev);
    if (refitStream) (void)hipStreamDestroy(refitStream);
    world.release();
    sun.release();
    coverMap.buf.release();
    for (DeviceBuffer* b : { &triNormals, &indices, &vertices, &positions, &meshes, &materials, &instances, &texInfos, &texels, &refitInst, &recordMap, &triBase, &stageCounters, &spare[0].world,
                             &spare[0].sun, &spare[0].instances, &spare[1].world, &spare[1].sun, &spare[1].instances })
        b->release();
}

int buildScene(ErrorSink* err, const ArkDdgiScene* s, int device, int buildThreads, int sunBvh, bool coverMap, std::shared_ptr<SceneStore>& out)
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
        sb.nodeCount = r.nodes.size(); // (the install sizes the refit's boxes scratch from it, ahead of its upload)
        rc = upload(err, sb.order, order.data(), order.size());
        if (rc == 0) rc = installSunBvh(err, *st, sb, &r, &sunIn.frame[0][0], s->directional_light.world_space_direction, nullptr);
        sb.order.release(); // (a failure before the install took it)
        if (rc != 0) return rc;
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
    instanceObjectBoxes(s, opt.threads, st->instObjBox, st->meshSpans);
    st->vertexCount = s->vertex_count;
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
    setWorldRoots(*st, w.roots, w.opaqueNodes, w.opaqueRecords);
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
    // the sun's cover map, on the device from the records just uploaded (no map: a scene
    // it does not take, sun_cover_map.h; every sun ray is then traced)
    st->coverWanted = coverMap;
    if (coverMap && s->has_directional_light && st->world.records > 0) {
        const auto tc = std::chrono::steady_clock::now();
        double frame[3][3];
        sun_frame(s->directional_light.world_space_direction, frame);
        float L[3];
        sunRayDirection(s->directional_light.world_space_direction, L);
        cover::Grid grid {};
        DeviceBuffer buf;
        bool ok = false;
        ARK_HIP(deviceBuildCoverMap(st->world.tris(st->world.buf), st->world.records, &frame[0][0], L, cover::kDefaultBudget, nullptr, grid, buf, ok));
        if (ok) setCoverMap(*st, buf, grid, s->directional_light.world_space_direction, &frame[0][0], std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tc).count());
    }
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
        st.vtx.copied(ts, fs);
        tgt.valid = true;
    }
    // the instance table of the shading kernels (set_scene's determinant and rows)
    std::vector<GpuInstance> ginst(count);
    for (uint32_t ii = 0; ii < count; ++ii) ginst[ii] = gpuInstance(instances[ii], st.meshHost[instances[ii].rt_mesh_index]);
    ARK_HIP(stagedUpload(st, tgt.instances.ptr, ginst.data(), count * sizeof(GpuInstance), rs));
    int rc;
    if ((rc = uploadRefitInstances(err, st, instances, count, &st.xf[ts], ts, rs)) != 0) return rc;
    if ((rc = enqueueRefit(err, st, rs, tgt.world, tgt.sun, ts)) != 0) return rc;
    ARK_HIP(geometryChanged(st, rs));
    ARK_HIP(sharedEnd(c, rs));
    return ARK_DDGI_OK;
}

// set_instances' topology rules: the scene's instance list with new transforms
int validateInstances(ErrorSink* err, const SceneStore& st, const ArkRTInstance* instances, uint32_t count)
{
    if (count != st.instHost.size() || (count && !instances))
        return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: %u instances, the scene has %zu", count, st.instHost.size());
    for (uint32_t i = 0; i < count; ++i) {
        const ArkRTInstance &a = instances[i], &b = st.instHost[i];
        if (a.rt_mesh_index != b.rt_mesh_index || a.triangle_count != b.triangle_count || a.hit_mask != b.hit_mask)
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: instance %u changed its mesh, triangle count or hit mask (a set_scene builds a new scene)", i);
        for (float v : a.object_to_world)
            if (!std::isfinite(v)) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "set_instances: instance %u: non-finite transform", i);
    }
    return ARK_DDGI_OK;
}

// The vertex ranges of one ark_ddgi_update_geometry call, checked (validateVertexUpdates):
// the instances their positions touch (refitted, their object-space boxes renewed) and
// those their other vertex data touches (shading records rewritten).
struct VertexWrites {
    const ArkDdgiVertexUpdate* updates = nullptr;
    uint32_t count = 0;
    std::vector<uint8_t> touchedPositions, touchedVertices; // per instance
    bool anyPositions = false, anyVertices = false, devicePositions = false;
};

// Every reason to refuse a call's vertex ranges, before anything changes
int validateVertexUpdates(ErrorSink* err, const SceneStore& st, const ArkDdgiVertexUpdate* updates, uint32_t n, VertexWrites& vw)
{
    if (n && !updates) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: null updates");
    std::vector<uint32_t> instMesh(st.instHost.size());
    for (size_t i = 0; i < instMesh.size(); ++i) instMesh[i] = st.instHost[i].rt_mesh_index;
    vw.updates = updates;
    vw.count = n;
    vw.touchedPositions.assign(instMesh.size(), 0);
    vw.touchedVertices.assign(instMesh.size(), 0);
    for (uint32_t u = 0; u < n; ++u) {
        const ArkDdgiVertexUpdate& q = updates[u];
        if (q.struct_size != sizeof(ArkDdgiVertexUpdate)) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: update %u: bad ArkDdgiVertexUpdate", u);
        if (q.flags & ~ARK_DDGI_VERTICES_DEVICE) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: update %u: unknown flags 0x%x", u, q.flags);
        if (!vertexRangeInPool(q.first_vertex, q.vertex_count, st.vertexCount))
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: update %u: vertices [%u, +%u) outside the pools' %llu", u, q.first_vertex, q.vertex_count,
                             static_cast<unsigned long long>(st.vertexCount));
        if (!q.positions && !q.vertices) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: update %u: neither positions nor vertices", u);
        const bool device = (q.flags & ARK_DDGI_VERTICES_DEVICE) != 0;
        if (q.positions && device) {
            bool ok = true, zero = true;
            for (int a = 0; a < 6; ++a) {
                ok = ok && std::isfinite(q.bounds[a]);
                zero = zero && q.bounds[a] == 0.0f;
            }
            for (int a = 0; a < 3; ++a) ok = ok && q.bounds[a] <= q.bounds[3 + a];
            if (!ok || zero) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: update %u: device positions need finite bounds (lo <= hi)", u);
        }
        if (q.positions && !device)
            for (size_t k = 0; k < static_cast<size_t>(q.vertex_count) * 3u; ++k)
                if (!std::isfinite(q.positions[k]))
                    return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "update_geometry: update %u: position %zu is not finite", u, k / 3u);
        if (q.positions) {
            touchedInstances(st.meshSpans, instMesh, q.first_vertex, q.vertex_count, vw.touchedPositions);
            vw.anyPositions = vw.anyPositions || q.vertex_count != 0;
            vw.devicePositions = vw.devicePositions || (device && q.vertex_count != 0);
        }
        if (q.vertices) {
            touchedInstances(st.meshSpans, instMesh, q.first_vertex, q.vertex_count, vw.touchedVertices);
            vw.anyVertices = vw.anyVertices || q.vertex_count != 0;
        }
    }
    return ARK_DDGI_OK;
}

// The object-space boxes of the instances the new positions touch (refitInflations): of
// the part of a range inside the mesh's span - the host positions', or a device source's
// `bounds`, which k_stage_vertices clamps into - replacing the old box when a host range
// covers the whole span, else joined with it (larger bounds only loosen the boxes).
void renewObjectBoxes(SceneStore& st, const VertexWrites& vw)
{
    for (uint32_t u = 0; u < vw.count; ++u) {
        const ArkDdgiVertexUpdate& q = vw.updates[u];
        if (!q.positions || !q.vertex_count) continue;
        for (size_t m = 0; m < st.meshSpans.size(); ++m) {
            const MeshSpan& sp = st.meshSpans[m];
            if (!spanTouched(sp, q.first_vertex, q.vertex_count)) continue;
            float box[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
            if (q.flags & ARK_DDGI_VERTICES_DEVICE) {
                std::copy(q.bounds, q.bounds + 6, box);
            } else {
                const int64_t lo = std::max<int64_t>(sp.first, q.first_vertex), hi = std::min<int64_t>(sp.first + sp.maxIndex, static_cast<int64_t>(q.first_vertex) + q.vertex_count - 1);
                for (int64_t v = lo; v <= hi; ++v) {
                    const float* P = q.positions + (v - q.first_vertex) * 3;
                    for (int a = 0; a < 3; ++a) {
                        box[a] = std::min(box[a], P[a]);
                        box[3 + a] = std::max(box[3 + a], P[a]);
                    }
                }
            }
            // (a device source never replaces: a position the kernel drops as non-finite keeps
            // its old value, which the old box holds and `bounds` need not)
            const bool whole = !(q.flags & ARK_DDGI_VERTICES_DEVICE) && spanCovered(sp, q.first_vertex, q.vertex_count);
            for (size_t i = 0; i < st.instHost.size(); ++i) {
                if (st.instHost[i].rt_mesh_index != m || !st.instHost[i].triangle_count) continue;
                std::array<float, 6>& b = st.instObjBox[i];
                for (int a = 0; a < 3; ++a) {
                    b[a] = whole ? box[a] : std::min(b[a], box[a]);
                    b[3 + a] = whole ? box[3 + a] : std::max(b[3 + a], box[3 + a]);
                }
            }
        }
    }
}

// One pool's part of a call's vertex ranges into the pool on `s` (k_stage_vertices):
// `floatsPerVertex` 3, the positions pool, or 9, the other vertex data. The host sources
// share one slot of the vertex ranges' own staging ring, each placed at its destination's 16-B alignment;
// device sources are read where they are, positions checked against their bounds.
int stageVertexRanges(ErrorSink* err, SceneStore& st, const VertexWrites& vw, bool positions, hipStream_t s)
{
    const uint32_t fpv = positions ? 3u : 9u;
    float* pool = positions ? st.positions.as<float>() : st.vertices.as<float>();
    auto source = [&](const ArkDdgiVertexUpdate& q) { return positions ? q.positions : reinterpret_cast<const float*>(q.vertices); };
    size_t bytes = 0;
    for (uint32_t u = 0; u < vw.count; ++u)
        if (source(vw.updates[u]) && !(vw.updates[u].flags & ARK_DDGI_VERTICES_DEVICE)) bytes += static_cast<size_t>(vw.updates[u].vertex_count) * fpv * 4u + 32u;
    int slot = -1;
    if (bytes) ARK_HIP(vertexStageAcquire(st, bytes, slot));
    size_t at = 0;
    // (a failure below still releases the slot behind the launches made so far: its next
    // user must not fill it while one of them reads it)
    hipError_t e = hipSuccess;
    for (uint32_t u = 0; u < vw.count && e == hipSuccess; ++u) {
        const ArkDdgiVertexUpdate& q = vw.updates[u];
        const float* src = source(q);
        const uint64_t words = static_cast<uint64_t>(q.vertex_count) * fpv;
        if (!src || !words) continue;
        float* dst = pool + static_cast<uint64_t>(q.first_vertex) * fpv;
        StageCheck chk {};
        if (q.flags & ARK_DDGI_VERTICES_DEVICE) {
            if (positions) {
                if (!st.stageCounters.ptr) {
                    if ((e = st.stageCounters.alloc(16)) == hipSuccess) e = hipMemsetAsync(st.stageCounters.ptr, 0, 16, s);
                    if (e != hipSuccess) break;
                }
                std::copy(q.bounds, q.bounds + 3, chk.lo);
                std::copy(q.bounds + 3, q.bounds + 6, chk.hi);
                chk.enabled = 1;
            }
        } else {
            at = ((at + 15u) & ~static_cast<size_t>(15u)) + (reinterpret_cast<uintptr_t>(dst) & 15u);
            float* staged = reinterpret_cast<float*>(static_cast<char*>(st.vstage[slot]) + at);
            std::memcpy(staged, src, words * 4u);
            at += words * 4u;
            src = staged;
        }
        e = launch_stage_vertices(src, dst, words, chk, st.stageCounters.as<unsigned long long>(), s);
    }
    if (slot >= 0) {
        const hipError_t r = vertexStageRelease(st, slot, s);
        if (e == hipSuccess) e = r;
    }
    if (e != hipSuccess) return err->hipFail(e, "staging vertex ranges");
    return ARK_DDGI_OK;
}

// The map global triangle -> world record of the front copy's record order on `s`,
// allocated at its first use and filled again after every installed world rebuild
int ensureRecordMap(ErrorSink* err, SceneStore& st, hipStream_t s)
{
    const uint32_t instances = static_cast<uint32_t>(st.instHost.size());
    if (st.triBaseHost.empty()) {
        uint64_t total = 0;
        std::vector<uint32_t> base(instances + 1u);
        for (uint32_t i = 0; i < instances; ++i) {
            base[i] = static_cast<uint32_t>(total);
            total += st.instHost[i].triangle_count;
        }
        if (total >= 0xffffffffull) return err->fail(ARK_DDGI_E_UNSUPPORTED, "update_geometry: %llu triangles", static_cast<unsigned long long>(total));
        base[instances] = static_cast<uint32_t>(total);
        if (const int rc = upload(err, st.triBase, base.data(), base.size())) return rc;
        st.triBaseHost.swap(base);
    }
    const uint32_t total = st.triBaseHost[instances];
    if (!st.recordMap.ptr) {
        ARK_HIP(st.recordMap.alloc(std::max<size_t>(16, static_cast<size_t>(total) * 4u)));
        ++st.recordMapAllocs;
        st.recordMapSeq = st.worldTopologySeq - 1u; // not of this order
    }
    if (st.recordMapSeq != st.worldTopologySeq) {
        ARK_HIP(launch_fill_u32(st.recordMap.ptr, std::max<uint64_t>(4, total), 0xffffffffu, s));
        ARK_HIP(launch_record_map(st.args.tris, static_cast<uint32_t>(st.world.records), st.triBase.as<uint32_t>(), instances, st.recordMap.as<uint32_t>(), s));
        st.recordMapSeq = st.worldTopologySeq;
        ++st.recordMapFills;
    }
    return ARK_DDGI_OK;
}

// The other vertex data of a call's ranges and what follows from it, on the caller's
// stream `s` (behind the frame in flight, which reads both, and behind this call's refit):
// the vertex pool, then the shading records of the instances the ranges touch.
int writeSurfaceData(ErrorSink* err, SceneStore& st, const VertexWrites& vw, hipStream_t s)
{
    int rc;
    if ((rc = stageVertexRanges(err, st, vw, false, s)) != 0) return rc;
    if ((rc = ensureRecordMap(err, st, s)) != 0) return rc;
    SurfaceJobs jobs {};
    uint32_t n = 0;
    auto flush = [&]() -> hipError_t {
        const hipError_t e = launch_update_surface_records(jobs, n, st.recordMap.as<uint32_t>(), static_cast<uint32_t>(st.world.records), st.indices.as<uint32_t>(),
                                                           st.vertices.as<float>(), st.triNormals.as<float4>(), s);
        n = 0;
        return e;
    };
    for (size_t i = 0; i < st.instHost.size(); ++i) {
        if (!vw.touchedVertices[i] || !st.instHost[i].triangle_count) continue;
        const ArkRTTriangleMesh& mesh = st.meshHost[st.instHost[i].rt_mesh_index];
        jobs.job[n++] = { static_cast<uint32_t>(i), st.triBaseHost[i], st.instHost[i].triangle_count, static_cast<uint32_t>(mesh.first_index), mesh.first_vertex };
        if (n == kSurfaceJobsPerLaunch) ARK_HIP(flush());
    }
    ARK_HIP(flush());
    return ARK_DDGI_OK;
}

int refitScene(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t s, const VertexWrites* vw);

} // namespace

int sceneSetInstances(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t s)
{
    if (const int rc = validateInstances(c.err, st, instances, count)) return rc;
    return refitScene(st, c, instances, count, s, nullptr);
}

int sceneUpdateGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count,
                        hipStream_t s)
{
    // (a copy: the refit ends by writing the new transforms into instHost)
    const std::vector<ArkRTInstance> kept = (!instances && !count) ? st.instHost : std::vector<ArkRTInstance>();
    if (!instances && !count) {
        instances = kept.data();
        count = static_cast<uint32_t>(kept.size());
    }
    int rc;
    if ((rc = validateInstances(c.err, st, instances, count)) != 0) return rc;
    VertexWrites vw;
    if ((rc = validateVertexUpdates(c.err, st, updates, updateCount, vw)) != 0) return rc;
    if ((rc = refitScene(st, c, instances, count, s, &vw)) != 0) return rc;
    // (the calls that went through: a refused or failed one counts nothing)
    ++st.geometryCalls;
    for (uint32_t u = 0; u < updateCount; ++u) st.verticesWritten += updates[u].vertex_count;
    return ARK_DDGI_OK;
}

int sceneGeometryStats(SceneStore& st, ErrorSink* err, uint64_t* out)
{
    out[0] = st.geometryCalls;
    out[1] = st.verticesWritten;
    out[2] = out[3] = 0;
    if (st.stageCounters.ptr) {
        ARK_HIP(hipStreamSynchronize(st.refitStream));
        ARK_HIP(hipMemcpy(out + 2, st.stageCounters.ptr, 16, hipMemcpyDeviceToHost));
    }
    return ARK_DDGI_OK;
}

hipError_t scenePositionsRead(SceneStore& st, hipStream_t s)
{
    if (!st.positionsStaged) return hipSuccess; // (the first staging waits for the caller's stream)
    hipError_t e = hipSuccess;
    if (!st.evPositionsRead) e = hipEventCreateWithFlags(&st.evPositionsRead, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(st.evPositionsRead, s);
    st.positionsReadValid = e == hipSuccess;
    return e;
}

namespace {

// The refit of ark_ddgi_set_instances and ark_ddgi_update_geometry (vw: its vertex ranges,
// checked; null: none), the arguments valid
int refitScene(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t s, const VertexWrites* vw)
{
    ErrorSink* err = c.err;
    ARK_HIP(sharedBegin(c));
    // the cover map is of the geometry before this refit
    ARK_HIP(clearCoverMap(st, s));
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
    if (vw && vw->anyPositions) {
        // The new positions, on the refit stream ahead of the refit that reads them. The
        // pool's other readers are the earlier refits (this stream), an install's forward
        // refit (evInstalled above) and the AO bake (evPositionsRead) - not the frame in
        // flight, beside which the refit keeps running. A device source is the caller's
        // work on `s`: only then does the stream wait for `s` as it stands (evFree[fs]) -
        // and at the scene's first staging, before which no bake left an event.
        if (st.positionsReadValid) {
            ARK_HIP(hipStreamWaitEvent(st.refitStream, st.evPositionsRead, 0));
            st.positionsReadValid = false;
        }
        if (vw->devicePositions || !st.positionsStaged) ARK_HIP(hipStreamWaitEvent(st.refitStream, st.evFree[fs], 0));
        st.positionsStaged = true;
        // the touched instances' vertices are newer than every copy's records from here on,
        // whatever becomes of this refit
        st.vtx.begin(count);
        for (uint32_t ii = 0; ii < count; ++ii)
            if (vw->touchedPositions[ii]) st.vtx.touch(ii);
        renewObjectBoxes(st, *vw);
        // A failure here (a HIP launch or allocation error) leaves the pool partly written
        // and the front copy's records of the old positions: the versions above keep the
        // touched instances dirty for every copy, so the next refit that succeeds
        // re-derives them from whatever the pool then holds, reaching every node; until
        // then only the bake, which reads the pool itself, can see the partial write. The
        // caller sends the ranges again.
        if ((rc = stageVertexRanges(err, st, *vw, true, st.refitStream)) != 0) {
            st.refitFull = true;
            return rc;
        }
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
    st.vtx.refitted(ts);
    rotateGeometry(st);
    // the caller's stream follows the refit (what it runs next sees the new geometry); the
    // contexts' next traversals on their traversal streams wait for it too (geometrySeq)
    ARK_HIP(hipStreamWaitEvent(s, st.evGeometry, 0));
    for (uint32_t ii = 0; ii < count; ++ii) std::memcpy(st.instHost[ii].object_to_world, instances[ii].object_to_world, sizeof(float) * 12);
    ++st.version;
    ++st.refitsSinceBuild;
    ++st.sunRefitsSinceBuild;
    st.bvhStats.refit_version = ++st.refitCount;
    if (vw && vw->anyVertices) {
        // The vertex pool (the alpha test of every traversal, the reflections, the bake) and
        // the shading records (every k_shade) on `s`: behind the frame in flight, which
        // reads the old ones, and - evGeometry recorded again - ahead of the next
        // traversal, whichever stream it runs on.
        // A failure here comes after the refitted copy became the front one: its records
        // are of the new positions while the vertex pool or the shading records may still
        // be the old ones. Nothing is out of bounds or stale by pointer (both buffers are
        // the same ones); the caller sees the error and sends the ranges' `vertices` again,
        // which rewrites both whatever state they are in. The map is filled anew then.
        if ((rc = writeSurfaceData(err, st, *vw, s)) != 0) {
            st.recordMapSeq = st.worldTopologySeq - 1u;
            return rc;
        }
        ARK_HIP(geometryChanged(st, s));
        ARK_HIP(sharedEnd(c, s));
    }
    // background rebuilds of the loosened BVHs (world and light-space), from a snapshot
    // taken on s behind this refit
    return sceneMaintenance(st, c, s);
}

} // namespace

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

namespace {

// The check of an installed BVH8 set `b` (`name`: "world" / "sun"), its front copy's nodes
// and records downloaded: check_bvh8_full (classOf: the instances' classes, or null: one
// tree for every class; lightFrame: the boxes hold light coordinates), the structure, the
// device build's breadth-first order, the refit's level order on the device against the
// one recomputed from the downloaded nodes (levelOffsets null: none yet), the live
// records' digest. `violations`: the caller's own, counted in.
int installedBvhCheck(ErrorSink* err, const char* name, const DeviceBvh& b, const GpuBvh8Node* devNodes, const GpuTriangle* devTris, const std::vector<uint32_t>* levelOffsets,
                      const int32_t* roots, int rootCount, const std::vector<int>* classOf, const double* lightFrame, bool deviceBuilt, uint64_t violations, uint64_t* out)
{
    std::vector<GpuBvh8Node> nodes(b.nodeCount);
    std::vector<GpuTriangle> tris(b.records);
    std::vector<uint32_t> order(nodes.size());
    if (!nodes.empty()) ARK_HIP(hipMemcpy(nodes.data(), devNodes, nodes.size() * sizeof(GpuBvh8Node), hipMemcpyDeviceToHost));
    if (!tris.empty()) ARK_HIP(hipMemcpy(tris.data(), devTris, tris.size() * sizeof(GpuTriangle), hipMemcpyDeviceToHost));
    if (!order.empty() && b.order.bytes >= order.size() * 4) ARK_HIP(hipMemcpy(order.data(), b.order.ptr, order.size() * 4, hipMemcpyDeviceToHost));
    Bvh8CheckResult c = check_bvh8_full(nodes, tris, roots, rootCount, classOf, nullptr, lightFrame);
    c.violations += violations;
    std::string why;
    if (!checkBvh8Structure(nodes, tris, roots, rootCount, why)) c.violations++;
    if (c.nodes != nodes.size()) c.violations++; // a node outside the roots' trees
    if (deviceBuilt) c.violations += c.notBreadthFirst; // the device build's order (the host collapse's: breadth first per subtree block)
    std::vector<uint32_t> wantOrder, wantOffsets;
    if (!bvhLevelOrder(nodes.data(), nodes.size(), roots, rootCount, wantOrder, wantOffsets)) {
        c.violations++;
    } else if (levelOffsets && (wantOrder != order || wantOffsets != *levelOffsets)) {
        c.violations++;
        why += " level order";
    }
    uint64_t live = 0, digest = 0;
    for (const GpuTriangle& g : tris) {
        if (isHoleTriangle(g)) continue;
        ++live;
        uint64_t h = 1469598103934665603ull;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(&g);
        for (size_t k = 0; k < sizeof(GpuTriangle); ++k) h = (h ^ p[k]) * 1099511628211ull;
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
    out[7] = deviceBuilt ? 1u : 0u;
    if (c.violations) err->lastError = std::string(name) + " BVH check: " + std::to_string(c.violations) + " violations" + (why.empty() ? "" : " (" + why + ")");
    return c.violations ? 1 : ARK_DDGI_OK;
}

} // namespace

int sceneWorldBvhCheck(const SceneStore& st, ErrorSink* err, uint64_t* out)
{
    const std::vector<int> classOf = instanceClasses(st);
    const int32_t roots[3] = { st.args.root_opaque, st.args.root_masked, st.args.root_blend };
    const int32_t opaqueEnd = roots[1] >= 0 ? roots[1] : roots[2] >= 0 ? roots[2] : static_cast<int32_t>(st.world.nodeCount);
    const uint64_t violations = roots[0] >= 0 && st.args.opaque_nodes != static_cast<uint32_t>(opaqueEnd - roots[0]) ? 1u : 0u;
    // (no level order before the first refit after set_scene)
    return installedBvhCheck(err, "world", st.world, st.args.nodes, st.args.tris, st.world.levelOffsets.empty() ? nullptr : &st.world.levelOffsets, roots, 3, &classOf, nullptr,
                             st.worldGpuBuilt, violations, out);
}

int sceneSunBvhCheck(const SceneStore& st, ErrorSink* err, uint64_t* out)
{
    std::fill(out, out + 8, uint64_t(0));
    if (st.sunArgs.sun_root < 0 || !st.sun.nodeCount) return 1; // no light-space BVH
    const int32_t root = 0;
    return installedBvhCheck(err, "sun", st.sun, st.sunArgs.sun_nodes, st.sunArgs.sun_tris, &st.sun.levelOffsets, &root, 1, nullptr, st.sunFrameD, st.sunGpuBuilt, 0, out);
}

int sceneRefitReach(const SceneStore& st, ErrorSink* err, uint64_t* out)
{
    std::fill(out, out + 4, uint64_t(0));
    // the nodes k_refit_nodes found live: masks[n] & dirty (masks of this topology only
    // once a refit has computed them)
    auto reach = [&](const DeviceBvh& b, uint64_t* o) -> int {
        if (!b.masksValid || !b.nodeCount || b.masks.bytes < b.nodeCount * 8) return ARK_DDGI_OK;
        std::vector<uint64_t> m(b.nodeCount);
        ARK_HIP(hipMemcpy(m.data(), b.masks.ptr, m.size() * 8, hipMemcpyDeviceToHost));
        o[0] = b.nodeCount;
        for (uint64_t v : m) o[1] += (v & b.refitDirty) != 0;
        return ARK_DDGI_OK;
    };
    if (const int rc = reach(st.world, out)) return rc;
    if (st.sunArgs.sun_root >= 0 && st.sun.records) return reach(st.sun, out + 2);
    return ARK_DDGI_OK;
}

} // namespace ark

