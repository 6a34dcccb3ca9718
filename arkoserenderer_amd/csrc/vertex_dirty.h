// vertex_dirty.h — which instances a vertex range update touches and which of them a refit
// must re-derive (ark_ddgi_update_geometry, scene_refit.cpp). Pure host code without a HIP
// dependency, so that it is tested on its own (tests/cpp/vertex_dirty_test.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ark {

// The vertices an RT mesh can reach: [first, first + maxIndex] of the scene's pools (first:
// ArkRTTriangleMesh.first_vertex; maxIndex: the largest index any of its instances'
// triangles holds, computed once at set_scene). used: an instance draws it.
struct MeshSpan {
    int64_t first = 0;
    uint32_t maxIndex = 0;
    bool used = false;
};

// [first, first + count) lies inside a pool of poolVertices (an empty range does anywhere
// up to the pool's end)
inline bool vertexRangeInPool(uint32_t first, uint32_t count, uint64_t poolVertices)
{
    return static_cast<uint64_t>(first) + count <= poolVertices;
}

// The span meets the range [first, first + count)
inline bool spanTouched(const MeshSpan& m, uint32_t first, uint32_t count)
{
    if (!m.used || count == 0) return false;
    const int64_t lo = m.first, hi = m.first + static_cast<int64_t>(m.maxIndex); // inclusive
    const int64_t rlo = first, rhi = static_cast<int64_t>(first) + count - 1;
    return lo <= rhi && rlo <= hi;
}

// The span lies wholly inside the range: the range's bounds are the mesh's new bounds
inline bool spanCovered(const MeshSpan& m, uint32_t first, uint32_t count)
{
    return m.used && count != 0 && m.first >= static_cast<int64_t>(first) &&
           m.first + static_cast<int64_t>(m.maxIndex) < static_cast<int64_t>(first) + count;
}

// Flags, in `touched` (one per instance; flags already set stay, so that a call's ranges
// accumulate), the instances whose mesh's span meets the range. Two instances of one mesh
// are both touched; so are meshes with overlapping spans.
inline void touchedInstances(const std::vector<MeshSpan>& spans, const std::vector<uint32_t>& instanceMesh, uint32_t first, uint32_t count, std::vector<uint8_t>& touched)
{
    if (touched.size() < instanceMesh.size()) touched.resize(instanceMesh.size(), 0);
    for (size_t i = 0; i < instanceMesh.size(); ++i) {
        const uint32_t m = instanceMesh[i];
        if (m < spans.size() && spanTouched(spans[m], first, count)) touched[i] = 1;
    }
}

// The vertex versions of a scene's instances against its three geometry copies (a member
// of their book, copy_book.h; DESIGN §1 "Deforming meshes"). seq counts the update calls that touched an instance; inst[i] is the
// call that touched instance i last; copy[slot] the call up to which the slot's records
// were re-derived; scratch the call up to which the shared boxes scratch was (the refit
// before, whichever copy it wrote).
struct VertexVersions {
    uint64_t seq = 0;
    std::vector<uint64_t> inst;
    uint64_t copy[3] = { 0, 0, 0 };
    uint64_t scratch = 0;

    bool inUse() const { return seq != 0; }
    // a new update call over `instances` instances; touch() follows for each touched one
    void begin(size_t instances)
    {
        if (inst.size() != instances) inst.assign(instances, 0);
        ++seq;
    }
    void touch(size_t i) { inst[i] = seq; }
    // A refit of `slot` must re-derive instance i's records: its vertices are newer than
    // the slot's records, or newer than the refit before's (the boxes scratch of the nodes
    // above it is then of its old vertices: "What a partial refit may skip")
    bool dirty(size_t i, int slot) const { return i < inst.size() && (inst[i] > copy[slot] || inst[i] > scratch); }
    // the slot was refitted (every dirty instance re-derived from the pools as they are)
    void refitted(int slot) { copy[slot] = scratch = seq; }
    // the slot's contents were copied from another's
    void copied(int dst, int src) { copy[dst] = copy[src]; }
    // An install put a job's snapshot of the front copy's records back into `front`. Its
    // forward refit (run when refits - vertex updates are refits - came in since the
    // snapshot) re-derives every instance, and so every one updated since; without one
    // nothing was updated since and the records are as current as the front copy's were.
    void installed(int front, bool forwardRefit)
    {
        if (forwardRefit) copy[front] = scratch = seq;
    }
};

} // namespace ark
