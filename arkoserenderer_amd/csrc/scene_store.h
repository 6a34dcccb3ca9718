// scene_store.h — the scene of the DDGI contexts on the device (include/ark_ddgi.h:
// ark_ddgi_set_scene, _share_scene, _set_instances) and what maintains it: the
// stream-ordered refits of its three geometry copies and the background rebuilds of its
// BVHs. ddgi_context.h holds the contexts; a store knows none of them, and contexts that
// share a store call into it one at a time (the C ABI's rule for one GPU's contexts).
//
// Stream order is a precondition, not a call. Every entry point that takes a stream `s`
// requires that the caller has ordered `s` behind everything its context enqueued before
// (ddgi_context.h: orderBegin); whatever it enqueues - an install on `s`, a snapshot on `s`,
// a refit on the store's own stream that `s` then waits for - is ordered behind that point,
// and the caller ends the operation on `s` (orderEnd). After any scene call the caller
// compares SceneStore::version with the one its kernel view was derived at and derives it
// again when it moved (refreshScene); before its next traversal it waits for evGeometry
// when geometrySeq moved.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ark_ddgi.h"
#include "copy_book.h"
#include "ddgi_kernels.h"
#include "device_bvh.h"
#include "scene_rebuild_policy.h"

namespace ark {

// Where a failing call leaves its message (ark_ddgi_last_error): a context is one.
struct ErrorSink {
    std::string lastError;
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

// returns sink->hipFail(...) from the enclosing function when a HIP call fails
#define ARK_HIP_TO(sink, expr)                                          \
    do {                                                                \
        hipError_t _e = (expr);                                         \
        if (_e != hipSuccess) return (sink)->hipFail(_e, #expr);        \
    } while (0)

struct RebuildJob; // a background rebuild (scene_store_internal.h)

// A buffer replaced while launches enqueued before may still read it: freed once `done`
// (recorded behind them) has completed.
struct Retired {
    DeviceBuffer buf;
    hipEvent_t done = nullptr;
};

// Pinned host staging for stream-ordered uploads, a ring of N buffers made at first use:
// acquire hands out the next one, free for the host to fill (its last reader, a few calls
// back, has run) and grown to `need`; release records its reader's end on the reader's stream.
template<int N>
struct PinnedRing {
    void* slot[N] {};
    size_t bytes[N] {};
    hipEvent_t done[N] {};
    int next = 0;
    hipError_t acquire(size_t need, int& i)
    {
        i = next;
        next = (i + 1) % N;
        hipError_t e = hipSuccess;
        if (!done[i] && (e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming)) != hipSuccess) return e;
        if (bytes[i]) (void)hipEventSynchronize(done[i]); // its last copy (an earlier frame's) has run
        if (bytes[i] < need) {
            if (slot[i]) (void)hipHostFree(slot[i]);
            slot[i] = nullptr;
            bytes[i] = 0;
            if ((e = hipHostMalloc(&slot[i], need, hipHostMallocDefault)) != hipSuccess) return e;
            bytes[i] = need;
        }
        return hipSuccess;
    }
    hipError_t release(int i, hipStream_t s) { return hipEventRecord(done[i], s); }
    void destroy()
    {
        for (int i = 0; i < N; ++i) {
            if (slot[i]) (void)hipHostFree(slot[i]);
            if (done[i]) (void)hipEventDestroy(done[i]);
        }
    }
};

// A spare geometry copy on the device (the front one's buffers are DeviceBvh::buf and
// SceneStore::instances): both BVHs, the instance table, the event that ends with its last readers.
struct GeometryCopy {
    DeviceBuffer world, sun, instances;
    hipEvent_t free = nullptr;
    bool freeValid = false;
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
    // The sun's cover map (sun_cover_map.h), a sibling product of the sun BVH whichever BVH
    // the sun's rays traverse: built on the device from the world records at set_scene and
    // by every background rebuild job (from its snapshot), for the sun direction `dir`.
    // A stale map is wrong, not slow: `valid` is cleared and the buffer retired the moment
    // the geometry it was built from changes (a refit, an install whose job saw refits come
    // in); a context uses it only while valid, for exactly this direction, with a tmax the
    // grid was checked for (ark_ddgi.cpp deriveSceneArgs).
    struct CoverMap {
        DeviceBuffer buf;
        cover::Grid grid {};
        float dir[3] { 0, 0, 0 };
        float frame[9] {}; // sun_frame(dir) in fp32: sunCoords' rows
        bool valid = false;
        float buildMs = 0.0f;
    } coverMap;
    bool coverWanted = false; // set_scene: not disabled by ARK_DDGI_FLAG_NO_SUN_COVER_MAP
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
    // the refit's transforms as uploaded last (refitInflations reads them; which are dirty: book)
    std::vector<RefitInstance> refitHost;
    // pinned staging of the per-frame uploads, a ring: a slot is reused once its copy (a
    // few calls back) has run, so the host runs up to kStageSlots / 2 frames of
    // set_instances_async ahead of the device (two slots: one frame, and every call
    // waited for the previous frame's refit)
    static constexpr int kStageSlots = 8;
    PinnedRing<kStageSlots> stage;
    // ark_ddgi_update_geometry's host vertex ranges have a ring of their own (allocated at
    // the first such call), so that a deform call takes the two slots above that a rigid one
    // takes and the host runs as far ahead; a call's ranges take one slot per pool here, the
    // vertex data's released only behind the frame in flight, so the large ranges run two
    // calls ahead and at most kVertexStageSlots buffers of the largest call stay pinned
    static constexpr int kVertexStageSlots = 4;
    PinnedRing<kVertexStageSlots> vstage;
    // object-space bounds of every instance's triangles (set_scene): the refit's world and
    // light-space bounds, for its box inflation, from the instances' transforms on the host
    std::vector<std::array<float, 6>> instObjBox;
    // The three geometry copies: the front one (world.buf, sun.buf, instances, frontFree) and
    // the spares, spare[0] the next refit's target. What each holds: the book (copy_book.h).
    GeometryCopy spare[2];
    CopyBook book;
    // the light-space BVH follows the sun: set_scene chose it (sunWanted), and after a
    // sun-direction change it is rebuilt in the background (sceneSunStep)
    bool sunWanted = false;
    int buildThreads = 16;
    std::unique_ptr<RebuildJob> sunJob;
    uint32_t sunRebuilds = 0;
    // rebuild requests (sceneSunStep): the sun direction the contexts sharing this scene
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
    std::unique_ptr<RebuildJob> worldJob;
    uint32_t worldRebuilds = 0, refitCount = 0;
    bool worldRebuildFailed = false;
    // ARK_DDGI_FLAG_GPU_REBUILD: the installed world BVHs are a device build (an LBVH: once
    // the motion stops one host rebuild replaces it, rebuildToStart)
    bool worldGpuBuilt = false;
    // ARK_DDGI_FLAG_GPU_REBUILD_SUN: the same for the installed light-space sun BVH
    bool sunGpuBuilt = false;
    // the background build started last (rebuildToStart: loosened BVHs take turns)
    uint8_t lastBackground = kBackgroundNone;
    std::vector<Retired> retired;
    // The order of the writes to the three geometry copies, owned with them (the contexts
    // sharing the store see one record of who read which copy): refits run on refitStream,
    // at the device's highest priority (its per-level launches are dispatched ahead of the
    // frame in flight's work when both wait for a CU). A copy's `free` event (frontFree: the
    // front one's; they rotate with the buffers) ends with the operations that read it
    // while it was the front one (recorded when a refit swapped it out, on the refitting
    // call's stream, which follows the others); evInstalled with the last install (a
    // rebuild installed on a caller's stream writes the front copy).
    // evGeometry ends with the last refit or install, geometrySeq counts its recordings: a
    // context's next traversal waits for it when the count has moved since its last wait.
    hipStream_t refitStream = nullptr;
    hipEvent_t frontFree = nullptr;
    bool frontFreeValid = false;
    hipEvent_t evInstalled = nullptr;
    bool installValid = false;
    hipEvent_t evGeometry = nullptr;
    uint32_t geometrySeq = 0;
    // counts the record orders of the world BVHs (set_scene, every installed world rebuild;
    // a refit keeps the order, in all three copies): a context resets its seed cache, whose
    // words are record indices, on its traversal stream when this has moved (ddgi_frame.cpp
    // traversalPart, behind its wait for evGeometry and ahead of the traversal)
    uint32_t worldTopologySeq = 0;
    // Deforming meshes (ark_ddgi_update_geometry; DESIGN §1 "Deforming meshes"). The pools'
    // vertex count and every RT mesh's vertex span (set_scene). Everything below is
    // allocated at the first update call: a scene that never makes one holds none of it.
    uint64_t vertexCount = 0;
    std::vector<MeshSpan> meshSpans;
    // global triangle -> world record index (k_record_map; triBase: the instances' first
    // global triangles, on the host and the device), filled at the first update that
    // rewrites shading records and again after each installed world rebuild (recordMapSeq
    // against worldTopologySeq)
    DeviceBuffer recordMap, triBase;
    std::vector<uint32_t> triBaseHost;
    uint32_t recordMapSeq = 0, recordMapAllocs = 0, recordMapFills = 0;
    // k_stage_vertices' counts of dropped and clamped device-source positions
    DeviceBuffer stageCounters;
    uint64_t geometryCalls = 0, verticesWritten = 0;
    // ends with the last operation outside the refit stream that reads the positions pool
    // (the AO bake): the next staging of positions, on the refit stream, waits for it
    hipEvent_t evPositionsRead = nullptr;
    bool positionsReadValid = false, positionsStaged = false;
    // Skins (ark_ddgi_register_skin; DESIGN §1 "Skinning"; scene_skin.cpp): made by the first
    // registration, so a scene without a skin allocates and launches nothing for them
    struct SkinSet* skins = nullptr;
    SceneStore();
    SceneStore(const SceneStore&) = delete;
    SceneStore& operator=(const SceneStore&) = delete;
    ~SceneStore(); // after a device sync: joins the jobs, frees the copies, the stream and the events
};

// What a scene call needs from the context that makes it.
struct SceneCall {
    ErrorSink* err;   // where a failure's message goes
    uint32_t flags;   // ArkDdgiDesc.flags
    bool hasSun;      // the context's sun (ark_ddgi_set_lights) ...
    float sunDir[3];  // ... and its direction
    bool shared;      // other contexts use the store too
};

// ark_ddgi_set_scene: the device scene of `s` built on `device` (the world BVHs, the
// light-space sun BVH when it pays or sunBvh forces it: 0 never, 1 always, -1 by cost).
// buildThreads: ArkDdgiDesc.build_threads. Synchronous; the device is idle.
// coverMap: the sun's cover map too, when the scene has a sun.
int buildScene(ErrorSink* err, const ArkDdgiScene* s, int device, int buildThreads, int sunBvh, bool coverMap, std::shared_ptr<SceneStore>& out);

// Everything an operation on `s` does to the scene first: buffers retired by earlier
// installs freed, finished rebuilds installed on `s`, new ones started (scene_rebuild_policy.h).
int sceneMaintenance(SceneStore& st, const SceneCall& c, hipStream_t s);

// ark_ddgi_set_lights: the request for the caller's sun direction noted, failed and stale
// sun builds dropped, and - only when mayEnqueue, i.e. `s` meets the precondition - a
// finished sun rebuild installed on `s` or a new one started (never a world rebuild).
int sceneSunStep(SceneStore& st, const SceneCall& c, hipStream_t s, bool mayEnqueue);
// whether such a step has an install or a start to consider (else the caller orders no stream)
bool sunStepMayEnqueue(const SceneStore& st, const SceneCall& c);
bool sunJobPending(const SceneStore& st);

// ark_ddgi_set_instances_async: the refit of the next spare copy to `instances` on the
// store's stream, which then becomes the front copy; `s` follows the refit.
int sceneSetInstances(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t s);
// ark_ddgi_update_geometry_async: the same refit with the vertex ranges `updates` written
// into the pools first - positions on the store's stream ahead of the refit, the other
// vertex data and the touched instances' shading records on `s`. instances null (count 0):
// the transforms stay.
int sceneUpdateGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count,
                        hipStream_t s);
// ark_ddgi_get_geometry_update_stats (waits for the refit stream)
int sceneGeometryStats(SceneStore& st, ErrorSink* err, uint64_t* out);
// An operation on `s` read the positions pool (the AO bake): the next vertex update follows it
hipError_t scenePositionsRead(SceneStore& st, hipStream_t s);

// ark_ddgi_register_skin / _unregister_skin (synchronous; unregistering waits for the device)
int sceneRegisterSkin(SceneStore& st, ErrorSink* err, const ArkDdgiSkinDesc* desc, uint32_t* outSkin);
int sceneUnregisterSkin(SceneStore& st, ErrorSink* err, uint32_t skin);
// ark_ddgi_skin_geometry_async: every pose's skin computed on `s` into the skin's own
// buffers (k_skin_vertices), which sceneUpdateGeometry's path then takes as device sources
// with the poses' host bounds - one refit for all of them and the transforms.
int sceneSkinGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiSkinPose* poses, uint32_t poseCount, const ArkRTInstance* instances, uint32_t count, hipStream_t s);
int sceneSkinViews(const SceneStore& st, ErrorSink* err, uint32_t skin, ArkDdgiSkinViews* out);
void sceneSkinStats(const SceneStore& st, uint64_t* out);
void destroySkinSet(struct SkinSet* set); // ~SceneStore (the device is idle)

// ark_ddgi_debug_scene_digest / _world_bvh_check over the front copy (the device is idle)
int sceneDigest(const SceneStore& st, ErrorSink* err, uint64_t* out);
int sceneWorldBvhCheck(const SceneStore& st, ErrorSink* err, uint64_t* out);
// ark_ddgi_debug_sun_bvh_installed_check over the front copy (1 with out zeroed: none installed)
int sceneSunBvhCheck(const SceneStore& st, ErrorSink* err, uint64_t* out);
// ark_ddgi_debug_refit_reach: the nodes of the world and the light-space BVHs and those the
// last refit reached (the node masks downloaded; the device is idle)
int sceneRefitReach(const SceneStore& st, ErrorSink* err, uint64_t* out);
// ark_ddgi_debug_rt_shadows_host_ctx: the front copy's triangle records (n x 12 words) and the
// instances' hit-mask classes, downloaded (the device is idle)
int sceneRecordsAndClasses(const SceneStore& st, ErrorSink* err, std::vector<uint32_t>& records, std::vector<int32_t>& classOf);

// ark_ddgi_debug_path_tracer_host_ctx: the front copy's records and instance table and the
// shading pools, downloaded (the device is idle); the lights are the calling context's
namespace pt {
struct HostScene;
}
int sceneHostCopy(const SceneStore& st, ErrorSink* err, pt::HostScene& out);

// SpotLightData as the closest hit reads it
GpuSpotLight gpuSpotLight(const ArkSpotLight& sl);

} // namespace ark
