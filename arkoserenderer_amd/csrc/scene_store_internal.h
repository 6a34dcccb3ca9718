// scene_store_internal.h — what scene_store.cpp and scene_{build,rebuild,refit,debug}.cpp share
// and nothing else includes: the rebuild job, and each file's functions that another one calls.
#pragma once

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>

#include "bvh_builder.h"
#include "scene_store.h"
#include "sun_cover_build.h"

// (every function of the store that can fail has an ErrorSink* err in scope)
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

template<typename T>
int upload(ErrorSink* err, DeviceBuffer& buf, const T* data, size_t count)
{
    size_t bytes = count * sizeof(T);
    ARK_HIP(buf.alloc(std::max<size_t>(bytes, 16)));
    if (bytes) ARK_HIP(hipMemcpy(buf.ptr, data, bytes, hipMemcpyHostToDevice));
    return ARK_DDGI_OK;
}

// scene_store.cpp
hipError_t retireBuffer(SceneStore& st, DeviceBuffer& b, hipStream_t s);
hipError_t stagedUpload(SceneStore& st, void* dst, const void* src, size_t bytes, hipStream_t s);
hipError_t dropSpares(SceneStore& st, hipStream_t s);
hipError_t sharedBegin(const SceneCall& c);
hipError_t sharedEnd(const SceneCall& c, hipStream_t s);
hipError_t geometryChanged(SceneStore& st, hipStream_t s);
std::vector<int> instanceClasses(const SceneStore& st);
void setGeometryArgs(SceneStore& st);
void setWorldRoots(SceneStore& st, const int32_t roots[3], uint32_t opaqueNodes, uint32_t opaqueRecords);
hipError_t clearCoverMap(SceneStore& st, hipStream_t s);
void setCoverMap(SceneStore& st, DeviceBuffer& buf, const cover::Grid& grid, const float* dir, const double* frame, float ms);
GpuInstance gpuInstance(const ArkRTInstance& inst, const ArkRTTriangleMesh& mesh); // scene_build.cpp
// scene_rebuild.cpp
int installSunBvh(ErrorSink* err, SceneStore& st, DeviceBvh& b, Bvh8BuildResult* host, const double* frame, const float* dir, hipStream_t s);
int worldCollect(SceneStore& st, const SceneCall& c, hipStream_t s);
int sunCollect(SceneStore& st, const SceneCall& c, hipStream_t s, bool mayEnqueue);
int startRebuild(SceneStore& st, const SceneCall& c, hipStream_t s, bool sunOnly);
// scene_refit.cpp
int uploadRefitInstances(ErrorSink* err, SceneStore& st, const ArkRTInstance* instances, uint32_t count, CopyBook::Refit which, hipStream_t s);
int enqueueRefit(ErrorSink* err, SceneStore& st, hipStream_t s, const DeviceBuffer& world, const DeviceBuffer& sun, int slot);
// sceneUpdateGeometry for device sources that the call itself produces (scene_skin.cpp):
// `produce` enqueues their producers on `s` once every argument has been accepted, ahead of
// the refit; trusted[u]: update u's bounds hold every position its source will contain.
int sceneProducedGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count,
                          hipStream_t s, const uint8_t* trusted, const std::function<int()>* produce);

} // namespace ark
