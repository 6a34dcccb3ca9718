// device_bvh.h — a BVH8 set in device memory as every builder hands it over (set_scene, the
// host rebuild jobs: uploadBvh; the device build: lbvh_device_build.h) and as the scene
// store keeps it (scene_store.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "ddgi_kernels.h"

namespace ark {

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
    // deepest first (uploaded by whoever built the BVH, before it is installed); the node
    // masks (k_node_masks: per topology); its boxes scratch, one for the three geometry
    // copies: after every refit boxes[n] is the box of the latest transforms of the
    // instances below n at the inflation boxesInflate, whichever copy that refit wrote (a
    // refit's dirty set holds every instance that changed since the refit before it, and
    // a refit at another inflation reaches every node: scene_refit.cpp)
    DeviceBuffer order, boxes, masks;
    std::vector<uint32_t> levelOffsets;
    bool masksValid = false;
    float boxesInflate = 0.0f;
    // the dirty word of the last refit (ark_ddgi_debug_refit_reach, while masksValid)
    uint64_t refitDirty = 0;
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
inline hipError_t uploadBvh(const std::vector<GpuBvh8Node>& nodes, std::vector<GpuTriangle>& tris, hipStream_t s, DeviceBvh& b)
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

} // namespace ark
