// scene_refit.cpp — the stream-ordered refit of the next geometry copy
// (ark_ddgi_set_instances) and the vertex ranges ark_ddgi_update_geometry writes ahead of it.
#include <cmath>

#include "scene_store_internal.h"

namespace ark {

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
// new), or every node (the book's `full`, or an inflation other than the one the copy's boxes
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
    args.dirty = (st.book.full || args.inflate != held || args.inflate != b.boxesInflate) ? ~0ull : dirty;
    b.refitDirty = args.dirty;
    for (size_t l = 0; l + 1 < lv.size(); ++l)
        ARK_HIP(launch_refit_nodes(nodes, tris, b.boxes.as<float>(), order + lv[l], lv[l + 1] - lv[l], args, b.masks.as<uint64_t>(), st.refitInst.as<RefitInstance>(),
                                   st.indices.as<uint32_t>(), st.positions.as<float>(), s));
    held = args.inflate;
    b.boxesInflate = args.inflate;
    return ARK_DDGI_OK;
}

// The refitted spare becomes the front copy, that one the last spare (CopyBook::refitted): events and views follow
void rotateGeometry(SceneStore& st)
{
    const GeometryCopy old { st.world.buf, st.sun.buf, st.instances, st.frontFree, st.frontFreeValid }, tgt = st.spare[0];
    st.world.buf = tgt.world;
    st.sun.buf = tgt.sun;
    st.instances = tgt.instances;
    st.frontFree = tgt.free;
    st.frontFreeValid = tgt.freeValid;
    st.spare[0] = st.spare[1];
    st.spare[1] = old;
    setGeometryArgs(st);
}

// The refit proper: the target spare st.spare[0] brought to `instances` on the refit
// stream (copied from the front copy first when it holds nothing valid: a new scene or an
// installed rebuild; what it replaces retired behind `last`). Any failure in here leaves
// the spare's contents unknown (sceneSetInstances).
int refitSpare(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t last)
{
    ErrorSink* err = c.err;
    GeometryCopy& tgt = st.spare[0];
    const hipStream_t rs = st.refitStream;
    if (!st.book.targetValid()) {
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
        st.book.copied();
    }
    // the instance table of the shading kernels (set_scene's determinant and rows)
    std::vector<GpuInstance> ginst(count);
    for (uint32_t ii = 0; ii < count; ++ii) ginst[ii] = gpuInstance(instances[ii], st.meshHost[instances[ii].rt_mesh_index]);
    ARK_HIP(stagedUpload(st, tgt.instances.ptr, ginst.data(), count * sizeof(GpuInstance), rs));
    int rc;
    if ((rc = uploadRefitInstances(err, st, instances, count, CopyBook::Target, rs)) != 0) return rc;
    if ((rc = enqueueRefit(err, st, rs, tgt.world, tgt.sun, st.book.target())) != 0) return rc;
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
    // per update, or null: a device source whose bounds are known to hold every position it
    // will write, all of them finite (a skin's: sceneSkinGeometry) - nothing is dropped
    const uint8_t* trusted = nullptr;
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
            // (a trusted one does: without it a walking character's box, and the refit's
            // inflation step with it, would grow for ever)
            const bool whole = (!(q.flags & ARK_DDGI_VERTICES_DEVICE) || (vw.trusted && vw.trusted[u])) && spanCovered(sp, q.first_vertex, q.vertex_count);
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
    if (bytes) ARK_HIP(st.vstage.acquire(bytes, slot));
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
            float* staged = reinterpret_cast<float*>(static_cast<char*>(st.vstage.slot[slot]) + at);
            std::memcpy(staged, src, words * 4u);
            at += words * 4u;
            src = staged;
        }
        e = launch_stage_vertices(src, dst, words, chk, st.stageCounters.as<unsigned long long>(), s);
    }
    if (slot >= 0) {
        const hipError_t r = st.vstage.release(slot, s);
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
    // read it (while it was the front one: its `free` event) and the last install; the frames in
    // flight keep reading the front copy. The copy swapped out here is free once the
    // operations enqueued so far are done.
    ARK_HIP(hipEventRecord(st.frontFree, s));
    st.frontFreeValid = true;
    if (st.spare[0].freeValid) ARK_HIP(hipStreamWaitEvent(st.refitStream, st.spare[0].free, 0));
    if (st.installValid) {
        ARK_HIP(hipStreamWaitEvent(st.refitStream, st.evInstalled, 0));
        st.installValid = false;
    }
    if (vw && vw->anyPositions) {
        // The new positions, on the refit stream ahead of the refit that reads them. The
        // pool's other readers are the earlier refits (this stream), an install's forward
        // refit (evInstalled above) and the AO bake (evPositionsRead) - not the frame in
        // flight, beside which the refit keeps running. A device source is the caller's
        // work on `s`: only then does the stream wait for `s` as it stands (frontFree) -
        // and at the scene's first staging, before which no bake left an event.
        if (st.positionsReadValid) {
            ARK_HIP(hipStreamWaitEvent(st.refitStream, st.evPositionsRead, 0));
            st.positionsReadValid = false;
        }
        if (vw->devicePositions || !st.positionsStaged) ARK_HIP(hipStreamWaitEvent(st.refitStream, st.frontFree, 0));
        st.positionsStaged = true;
        // the touched instances' vertices are newer than every copy's records from here on,
        // whatever becomes of this refit
        st.book.vertexUpdate(vw->touchedPositions);
        renewObjectBoxes(st, *vw);
        // A failure here (a HIP launch or allocation error) leaves the pool partly written
        // and the front copy's records of the old positions: the versions above keep the
        // touched instances dirty for every copy, so the next refit that succeeds
        // re-derives them from whatever the pool then holds, reaching every node; until
        // then only the bake, which reads the pool itself, can see the partial write. The
        // caller sends the ranges again.
        if ((rc = stageVertexRanges(err, st, *vw, true, st.refitStream)) != 0) {
            st.book.targetUnknown();
            return rc;
        }
    }
    if ((rc = refitSpare(st, c, instances, count, s)) != 0) {
        // the spare may be half written and the book no longer describes it: the next
        // refit copies the front one anew and reaches every node
        st.book.targetUnknown();
        return rc;
    }
    // the refitted copy becomes the front one
    st.book.refitted(instances, count);
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

// The refit of the copy (`world`, `sun`; slot: the transforms and inflations it holds) of
// every BVH of the scene on `s`: the records of the dirty instances (st.refitInst's
// flags, CopyBook::dirty) re-transformed, the boxes and planes above them recomputed - the
// world BVHs, then the light-space sun BVH (its boxes of the records' light coordinates).
// The boxes' inflations from the instances' bounds (refitInflations, host).
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
    if (const int rc = refitBvh(err, st, st.world, world, a, dirty, st.book.inflation(slot, 0), s)) return rc;
    if (st.sunArgs.sun_root >= 0 && st.sun.records && !st.sun.levelOffsets.empty()) {
        std::memcpy(a.frame, st.sunFrameD, sizeof(a.frame));
        a.inflate = inflationStep(inflateLight);
        a.light = 1;
        if (const int rc = refitBvh(err, st, st.sun, sun, a, dirty, st.book.inflation(slot, 1), s)) return rc;
    }
    return ARK_DDGI_OK;
}

// The refit's transforms of `instances` on the device (stream-ordered), with the dirty flag
// of each as the book decides it (CopyBook::dirty; Forward: an install's, every one).
int uploadRefitInstances(ErrorSink* err, SceneStore& st, const ArkRTInstance* instances, uint32_t count, CopyBook::Refit which, hipStream_t s)
{
    if (st.refitHost.size() != count) st.refitHost.assign(count, RefitInstance {});
    if (!st.refitInst.ptr || st.refitInst.bytes < std::max<size_t>(16, count * sizeof(RefitInstance))) ARK_HIP(st.refitInst.alloc(std::max<size_t>(16, count * sizeof(RefitInstance))));
    for (uint32_t ii = 0; ii < count; ++ii) {
        const float* M = instances[ii].object_to_world;
        const float det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
        const ArkRTTriangleMesh& mesh = st.meshHost[instances[ii].rt_mesh_index];
        RefitInstance& q = st.refitHost[ii];
        std::memcpy(q.m, M, sizeof(q.m));
        q.first_vertex = mesh.first_vertex;
        q.first_index = static_cast<uint32_t>(mesh.first_index);
        q.flip = det < 0.0f ? 1u : 0u;
        q.dirty = st.book.dirty(which, ii, M) ? 1u : 0u;
    }
    ARK_HIP(stagedUpload(st, st.refitInst.ptr, st.refitHost.data(), count * sizeof(RefitInstance), s));
    return ARK_DDGI_OK;
}

int sceneSetInstances(SceneStore& st, const SceneCall& c, const ArkRTInstance* instances, uint32_t count, hipStream_t s)
{
    if (const int rc = validateInstances(c.err, st, instances, count)) return rc;
    return refitScene(st, c, instances, count, s, nullptr);
}

int sceneUpdateGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count,
                        hipStream_t s)
{
    return sceneProducedGeometry(st, c, updates, updateCount, instances, count, s, nullptr, nullptr);
}

int sceneProducedGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiVertexUpdate* updates, uint32_t updateCount, const ArkRTInstance* instances, uint32_t count,
                          hipStream_t s, const uint8_t* trusted, const std::function<int()>* produce)
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
    vw.trusted = trusted;
    // (nothing was enqueued for a refused call)
    if (produce && (rc = (*produce)()) != 0) return rc;
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

} // namespace ark
