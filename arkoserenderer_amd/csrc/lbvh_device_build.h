// lbvh_device_build.h — the device build of a BVH8 set from a snapshot of triangle records
// (ddgi_bvh_build.hip's kernels, rocPRIM's sort and the refit pass, driven from the host):
// the rebuild jobs' device variant (scene_rebuild.cpp: runRebuildJob) and the traced parity
// entry (ark_ddgi_debug_lbvh_device_parity, lbvh_device_build.cpp). Knows no SceneStore.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "device_bvh.h"
#include "lbvh_build.h"

namespace ark {

struct LbvhGpuTrace; // every stage's result on the host (lbvh_device_build.cpp: the parity entry)

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
    // ARK_DDGI_FLAG_GPU_REBUILD_SAH: the SAH pass over the radix tree's treelets
    // (k_lbvh_treelet_sah) before the collapse, which then decides by the pass's boxes
    bool sah = false;
    // ARK_DDGI_FLAG_GPU_REBUILD_PLAN (with sah; alone it does nothing): the pass splits down to
    // single primitives and plans its nodes, k_lbvh_upper_plan the nodes above the treelets,
    // and the collapse follows the picks (lbvh::planCut)
    bool plan = false;
    DeviceBvh* bvh = nullptr;          // out: buffer, level order (device and offsets), counts, depth
    DeviceBuffer* perm = nullptr;      // out: the record order's source indices (null: not wanted)
    LbvhGpuTrace* trace = nullptr;     // out: the stages' results (null in the product paths: nothing more is enqueued)
    // out
    int32_t roots[3] { -1, -1, -1 };
    uint32_t opaqueNodes = 0, prims = 0;
    uint32_t opaqueRecords = 0;        // the opaque class's records: [0, opaqueRecords) of the result's
    float inflateAbs = 0.0f;           // the boxes' absolute inflation (the sun's refit floor; the world keeps set_scene's)
    std::vector<uint32_t> order;       // the level order on the host
};

// The device build on `s`: hipSuccess and `why` empty when g.bvh holds the result; `why`
// set when the host has to build this scene.
hipError_t buildLbvhGpu(LbvhGpuBuild& g, hipStream_t s, std::string& why);

// Errors after which the device is not used again by the job (no host fallback)
bool isDeviceFault(hipError_t e);

} // namespace ark
