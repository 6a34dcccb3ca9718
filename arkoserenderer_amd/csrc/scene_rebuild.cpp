// scene_rebuild.cpp — the background rebuilds of the world BVHs and the light-space sun BVH
// (RebuildJob): the jobs' host and device builds, and what collects, starts and installs them.
#include <chrono>

#include "lbvh_device_build.h"
#include "scene_store_internal.h"
#include "sun_bvh.h"

namespace ark {

namespace {

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

// Where an installed job's bookkeeping goes: the world's fields or the sun's
struct InstallBook {
    bool& gpuBuilt;        // SceneStore::worldGpuBuilt / sunGpuBuilt
    uint32_t& refitsSince; // SceneStore::refitsSinceBuild / sunRefitsSinceBuild
    uint32_t &installedBuilder, &gpuRebuilds, &builtRefitVersion; // ArkDdgiBvhStats, as is the build time
    float& buildMs;
};

// The end of an install of `job`'s result on `s` (sunCollect, worldCollect): its builder,
// time and snapshot noted, the new topology refitted forward when refits came in while it
// was built (every instance re-transformed: its records follow them), the spares dropped -
// retired behind everything enqueued so far, copied anew by the next refit, which waits for
// the install (evInstalled) - the next traversal ordered behind it, the scene's version bumped.
int finishInstall(SceneStore& st, const SceneCall& c, RebuildJob& job, InstallBook book, hipStream_t s)
{
    ErrorSink* err = c.err;
    book.buildMs = job.ms;
    book.gpuBuilt = job.gpu;
    book.installedBuilder = job.gpu ? 1u : 0u;
    if (job.gpu) book.gpuRebuilds++;
    const uint32_t refitsSince = book.refitsSince = st.refitCount - job.refitsAt; // refits since its snapshot
    book.builtRefitVersion = job.refitsAt;
    st.world.masksValid = st.sun.masksValid = false;
    st.book.installed(refitsSince != 0);
    // the job's cover map is the front copy's when no refit came in since its snapshot (the
    // records it was built from are the ones installed or kept); an older one goes
    if (job.coverOk && refitsSince == 0) {
        ARK_HIP(clearCoverMap(st, s));
        setCoverMap(st, job.coverBuf, job.coverGrid, job.coverDir, job.coverFrame, job.coverMs);
    } else if (refitsSince != 0) {
        ARK_HIP(clearCoverMap(st, s));
    }
    if (refitsSince) {
        if (const int rc = uploadRefitInstances(err, st, st.instHost.data(), static_cast<uint32_t>(st.instHost.size()), CopyBook::Forward, s)) return rc;
        if (const int rc = enqueueRefit(err, st, s, st.world.buf, st.sun.buf, st.book.front())) return rc;
    }
    ARK_HIP(dropSpares(st, s));
    const hipError_t installed = hipEventRecord(st.evInstalled, s);
    st.installValid = installed == hipSuccess;
    ARK_HIP(installed);
    ARK_HIP(geometryChanged(st, s));
    ARK_HIP(sharedEnd(c, s));
    ++st.version;
    return ARK_DDGI_OK;
}

bool sameDir(const float* a, const float* b) { return std::memcmp(a, b, 3 * sizeof(float)) == 0; }

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

} // namespace

// The light-space BVH `b` (its level order on the device, whoever built it) built for the
// sun direction `dir` in `frame` becomes the scene's: its nodes and records uploaded by the
// job (sunCollect: host null), or here from `host` (set_scene, synchronously).
int installSunBvh(ErrorSink* err, SceneStore& st, DeviceBvh& b, Bvh8BuildResult* host, const double* frame, const float* dir, hipStream_t s)
{
    ARK_HIP(replaceBvh(st, st.sun, b, s));
    ARK_HIP(growBoxes(st, st.sun, s));
    if (host) ARK_HIP(uploadBvh(host->nodes, host->tris, nullptr, st.sun));
    st.sunArgs.sun_root = 0;
    setGeometryArgs(st);
    for (int k = 0; k < 9; ++k) {
        st.sunArgs.sun_frame[k] = static_cast<float>(frame[k]);
        st.sunFrameD[k] = frame[k];
    }
    std::memcpy(st.sunDirBuilt, dir, sizeof(st.sunDirBuilt));
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
        setGeometryArgs(st);
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

} // namespace ark
