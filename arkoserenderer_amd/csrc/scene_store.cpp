// scene_store.cpp — the device scene's lifetime and what its maintenance shares: retired
// buffers, the pinned staging, the kernel views, the cover map, the maintenance entry points.
#include "scene_store_internal.h"

namespace ark {

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
    int i = 0;
    hipError_t e = st.stage.acquire(bytes, i);
    if (e != hipSuccess) return e;
    std::memcpy(st.stage.slot[i], src, bytes);
    if ((e = hipMemcpyAsync(dst, st.stage.slot[i], bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    return st.stage.release(i, s);
}

// The spare geometry copies retired behind everything enqueued on `s` so far.
hipError_t dropSpares(SceneStore& st, hipStream_t s)
{
    hipError_t e = hipSuccess;
    for (GeometryCopy& c : st.spare)
        for (DeviceBuffer* b : { &c.world, &c.sun, &c.instances })
            if (e == hipSuccess) e = retireBuffer(st, *b, s);
    st.book.sparesDropped();
    return e;
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

// The kernels' view of the front copy: the world BVHs and, while one is installed (sun_root), the sun BVH
void setGeometryArgs(SceneStore& st)
{
    st.args.nodes = st.world.nodes(st.world.buf);
    st.args.tris = st.world.tris(st.world.buf);
    st.args.tri_byte_offset = static_cast<uint32_t>(st.world.triOffset);
    st.args.instances = st.instances.as<GpuInstance>();
    if (st.sunArgs.sun_root >= 0 && st.sun.buf.ptr) {
        st.sunArgs.sun_nodes = st.sun.nodes(st.sun.buf);
        st.sunArgs.sun_tris = st.sun.tris(st.sun.buf);
    }
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
    stage.destroy();
    vstage.destroy();
    destroySkinSet(skins);
    for (hipEvent_t ev : { frontFree, spare[0].free, spare[1].free, evInstalled, evGeometry, evPositionsRead })
        if (ev) (void)hipEventDestroy(ev);
    if (refitStream) (void)hipStreamDestroy(refitStream);
    world.release();
    sun.release();
    coverMap.buf.release();
    for (DeviceBuffer* b : { &triNormals, &indices, &vertices, &positions, &meshes, &materials, &instances, &texInfos, &texels, &refitInst, &recordMap, &triBase, &stageCounters, &spare[0].world,
                             &spare[0].sun, &spare[0].instances, &spare[1].world, &spare[1].sun, &spare[1].instances })
        b->release();
}

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

} // namespace ark
