// scene_skin.cpp — a scene's skins on the device (ark_ddgi_register_skin,
// ark_ddgi_skin_geometry; DESIGN §1 "Skinning"): the registered arrays, the buffers
// k_skin_vertices writes, the per-call pose upload, and the debug entries that compare the
// kernel with its host restatement.
#include <chrono>
#include <cmath>
#include <cstring>

#include "../../include/ark_ddgi_debug.h"
#include "scene_store_internal.h"
#include "skinning_host.h"

namespace ark {

// A skin's device side. The kernel writes into buffers the skin owns, never into the pools
// (k_stage_vertices stays their only writer). Positions have two buffers, written in turn:
// a run reads the one before for its velocity while it writes the other, and the staging
// of the call before, which may still read the one before on the refit stream, is never
// overwritten by the next run. The run after next writes it again; that run's stream
// follows the call in between, whose stream waited for its refit behind that staging (the
// refit stream runs in order), so no host wait and no event per skin is needed. A call
// that failed half way waited for nothing: the next call's stream then waits for the refit
// stream as it stands (SkinSet::fence).
struct DeviceSkin {
    DeviceBuffer bindPositions, bindVertices, morph, skinning;
    DeviceBuffer outPositions[2], outVertices, outVelocities;
    DeviceBuffer pose; // the joints' rows, then the morph weights: rewritten by every call, in stream order
    uint32_t runs = 0;
    int latest = 0; // outPositions[latest]: the last run's
    void release()
    {
        for (DeviceBuffer* b : { &bindPositions, &bindVertices, &morph, &skinning, &outPositions[0], &outPositions[1], &outVertices, &outVelocities, &pose }) b->release();
    }
};

struct SkinSet {
    skin::Registry reg;
    std::vector<DeviceSkin> dev; // by handle
    static constexpr int kPoseSlots = 4;
    PinnedRing<kPoseSlots> poseRing; // a call's poses, pinned: the host runs up to three calls ahead
    hipEvent_t fence = nullptr;
    bool needFence = false;
    uint64_t calls = 0, vertices = 0, rejected = 0;
};

void destroySkinSet(SkinSet* set)
{
    if (!set) return;
    for (DeviceSkin& d : set->dev) d.release();
    set->poseRing.destroy();
    if (set->fence) (void)hipEventDestroy(set->fence);
    delete set;
}

namespace {

size_t poseFloats(const skin::SkinHost& h) { return 12u * static_cast<size_t>(h.jointCount) + h.morphCount; }

// the registered arrays on the device and the output buffers (synchronous)
hipError_t uploadSkin(const skin::SkinHost& h, DeviceSkin& d)
{
    const size_t n = h.vertexCount;
    auto put = [](DeviceBuffer& b, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = b.alloc(std::max<size_t>(16, bytes));
        if (e == hipSuccess && bytes) e = hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = put(d.bindPositions, h.positions.data(), 12u * n);
    if (e == hipSuccess) e = put(d.bindVertices, h.vertices.data(), 36u * n);
    if (e == hipSuccess && h.morphCount) e = put(d.morph, h.morph.data(), 36u * n * h.morphCount);
    if (e == hipSuccess && h.skeleton) {
        std::vector<uint32_t> rows(8u * n); // ArkSkinningVertex: four indices, four weights
        for (size_t i = 0; i < n; ++i) {
            std::memcpy(&rows[8 * i], &h.indices[4 * i], 16);
            std::memcpy(&rows[8 * i + 4], &h.weights[4 * i], 16);
        }
        e = put(d.skinning, rows.data(), 32u * n);
    }
    for (DeviceBuffer* b : { &d.outPositions[0], &d.outPositions[1], &d.outVelocities })
        if (e == hipSuccess) e = b->alloc(12u * n);
    if (e == hipSuccess) e = d.outVertices.alloc(36u * n);
    if (e == hipSuccess) e = d.pose.alloc(std::max<size_t>(16, 4u * poseFloats(h)));
    return e;
}

SkinArgs skinArgs(const skin::SkinHost& h, const DeviceSkin& d, const float* prev, float* outPositions, float* outVertices, float* outVelocities)
{
    SkinArgs a {};
    a.bindPositions = d.bindPositions.as<float>();
    a.bindVertices = d.bindVertices.as<float>();
    a.morph = d.morph.as<float>();
    a.skinning = h.skeleton ? d.skinning.as<uint4>() : nullptr;
    a.joints = d.pose.as<float>();
    a.morphWeights = d.pose.as<float>() + 12u * static_cast<size_t>(h.jointCount);
    a.prev = prev;
    a.outPositions = outPositions;
    a.outVertices = outVertices;
    a.outVelocities = outVelocities;
    a.vertexCount = h.vertexCount;
    a.morphCount = h.morphCount;
    a.jointCount = h.jointCount;
    return a;
}

// a pose as the kernel reads it: the joints' rows 0-2, then the morph weights
void packPose(const skin::SkinHost& h, const ArkDdgiSkinPose& p, float* out)
{
    if (h.skeleton) skin::jointRows(p.joint_matrices, h.jointCount, out);
    for (uint32_t k = 0; k < h.morphCount; ++k) out[12u * h.jointCount + k] = p.morph_weights[k];
}

// a pose's arguments (not its values: poseBound)
const char* poseArguments(const skin::SkinHost* h, const ArkDdgiSkinPose& p)
{
    if (p.struct_size != sizeof(ArkDdgiSkinPose)) return "bad ArkDdgiSkinPose";
    if (!h) return "unknown skin";
    if (h->skeleton && !p.joint_matrices) return "null joint_matrices";
    if (h->morphCount && !p.morph_weights) return "null morph_weights";
    return nullptr;
}

} // namespace

int sceneRegisterSkin(SceneStore& st, ErrorSink* err, const ArkDdgiSkinDesc* desc, uint32_t* outSkin)
{
    if (!outSkin) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "register_skin: null out_skin");
    std::unique_ptr<skin::SkinHost> h;
    std::string why;
    if (const int rc = skin::buildSkin(desc, h, why)) return err->fail(rc, "%s", why.c_str());
    if (!vertexRangeInPool(h->firstVertex, h->vertexCount, st.vertexCount))
        return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "register_skin: vertices [%u, +%u) outside the pools' %llu", h->firstVertex, h->vertexCount,
                         static_cast<unsigned long long>(st.vertexCount));
    DeviceSkin d;
    const hipError_t e = uploadSkin(*h, d);
    if (e != hipSuccess) {
        d.release();
        return e == hipErrorOutOfMemory ? err->fail(ARK_DDGI_E_OUT_OF_MEMORY, "register_skin: out of device memory") : err->hipFail(e, "register_skin");
    }
    if (!st.skins) st.skins = new SkinSet;
    *outSkin = static_cast<uint32_t>(st.skins->reg.skins.size());
    st.skins->reg.skins.push_back(std::move(h));
    st.skins->dev.push_back(d);
    return ARK_DDGI_OK;
}

int sceneUnregisterSkin(SceneStore& st, ErrorSink* err, uint32_t handle)
{
    if (!st.skins || !st.skins->reg.get(handle)) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "unregister_skin: unknown skin %u", handle);
    ARK_HIP(hipDeviceSynchronize()); // (rare; staging or a consumer of the views may still read its buffers)
    st.skins->reg.remove(handle);
    st.skins->dev[handle].release();
    return ARK_DDGI_OK;
}

int sceneSkinGeometry(SceneStore& st, const SceneCall& c, const ArkDdgiSkinPose* poses, uint32_t poseCount, const ArkRTInstance* instances, uint32_t count, hipStream_t s)
{
    ErrorSink* err = c.err;
    if (poseCount && !poses) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "skin_geometry: null poses");
    if (poseCount && !st.skins) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "skin_geometry: the scene has no skin");
    if (!poseCount) return sceneUpdateGeometry(st, c, nullptr, 0, instances, count, s);
    SkinSet& set = *st.skins;
    // every reason to refuse the poses, and their bounds, before anything is enqueued
    std::vector<ArkDdgiVertexUpdate> updates(poseCount);
    std::vector<size_t> at(poseCount);
    std::vector<float> packed;
    auto refuse = [&](uint32_t p, const char* why) {
        ++set.rejected;
        return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "skin_geometry: pose %u: %s", p, why);
    };
    for (uint32_t p = 0; p < poseCount; ++p) {
        const skin::SkinHost* h = poses[p].struct_size == sizeof(ArkDdgiSkinPose) ? set.reg.get(poses[p].skin) : nullptr;
        if (const char* why = poseArguments(h, poses[p])) return refuse(p, why);
        for (uint32_t q = 0; q < p; ++q)
            if (poses[q].skin == poses[p].skin) return refuse(p, "a skin twice in one call");
        at[p] = packed.size();
        packed.resize(at[p] + ((poseFloats(*h) + 3u) & ~static_cast<size_t>(3u)));
        packPose(*h, poses[p], packed.data() + at[p]);
        const DeviceSkin& d = set.dev[poses[p].skin];
        ArkDdgiVertexUpdate& u = updates[p];
        u = ArkDdgiVertexUpdate {};
        u.struct_size = sizeof(ArkDdgiVertexUpdate);
        u.first_vertex = h->firstVertex;
        u.vertex_count = h->vertexCount;
        u.flags = ARK_DDGI_VERTICES_DEVICE;
        u.positions = d.outPositions[d.latest ^ 1].as<float>();
        u.vertices = d.outVertices.as<ArkRTVertex>();
        std::string why;
        if (!skin::poseBound(*h, packed.data() + at[p], packed.data() + at[p] + 12u * h->jointCount, u.bounds, why)) return refuse(p, why.c_str());
    }
    // the runs on `s`, once the refit's own arguments have been accepted too
    bool produced = false;
    const std::function<int()> produce = [&]() -> int {
        produced = true;
        if (set.needFence) {
            if (!set.fence) ARK_HIP(hipEventCreateWithFlags(&set.fence, hipEventDisableTiming));
            ARK_HIP(hipEventRecord(set.fence, st.refitStream));
            ARK_HIP(hipStreamWaitEvent(s, set.fence, 0));
            set.needFence = false;
        }
        int slot = -1;
        ARK_HIP(set.poseRing.acquire(packed.size() * 4u, slot));
        std::memcpy(set.poseRing.slot[slot], packed.data(), packed.size() * 4u);
        hipError_t e = hipSuccess;
        for (uint32_t p = 0; p < poseCount && e == hipSuccess; ++p) {
            const skin::SkinHost& h = *set.reg.get(poses[p].skin);
            DeviceSkin& d = set.dev[poses[p].skin];
            if (poseFloats(h)) e = hipMemcpyAsync(d.pose.ptr, static_cast<const float*>(set.poseRing.slot[slot]) + at[p], poseFloats(h) * 4u, hipMemcpyHostToDevice, s);
            const int target = d.latest ^ 1;
            if (e == hipSuccess)
                e = launch_skin_vertices(skinArgs(h, d, d.runs ? d.outPositions[d.latest].as<float>() : nullptr, d.outPositions[target].as<float>(), d.outVertices.as<float>(),
                                                  d.outVelocities.as<float>()),
                                         s);
            if (e == hipSuccess) {
                d.latest = target;
                ++d.runs;
            }
        }
        // (the slot's copies are on `s` whatever came of the launches)
        const hipError_t r = set.poseRing.release(slot, s);
        if (e == hipSuccess) e = r;
        if (e != hipSuccess) return err->hipFail(e, "skinning");
        return ARK_DDGI_OK;
    };
    const std::vector<uint8_t> trusted(poseCount, 1);
    const int rc = sceneProducedGeometry(st, c, updates.data(), poseCount, instances, count, s, trusted.data(), &produce);
    if (rc != 0) {
        // a failure behind the runs may leave runs and stagings enqueued that no stream waited for
        set.needFence = set.needFence || produced;
        return rc;
    }
    ++set.calls;
    for (uint32_t p = 0; p < poseCount; ++p) set.vertices += updates[p].vertex_count;
    return ARK_DDGI_OK;
}

int sceneSkinViews(const SceneStore& st, ErrorSink* err, uint32_t handle, ArkDdgiSkinViews* out)
{
    const skin::SkinHost* h = st.skins ? st.skins->reg.get(handle) : nullptr;
    if (!h || !out) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "get_skin_views: unknown skin %u", handle);
    const DeviceSkin& d = st.skins->dev[handle];
    *out = ArkDdgiSkinViews {};
    out->vertex_count = h->vertexCount;
    out->runs = d.runs;
    if (d.runs) {
        out->positions = d.outPositions[d.latest].as<float>();
        out->vertices = d.outVertices.as<ArkRTVertex>();
        out->velocities = d.outVelocities.as<float>();
    }
    return ARK_DDGI_OK;
}

void sceneSkinStats(const SceneStore& st, uint64_t* out)
{
    out[0] = st.skins ? st.skins->calls : 0;
    out[1] = st.skins ? st.skins->vertices : 0;
    out[2] = st.skins ? st.skins->rejected : 0;
    out[3] = st.skins ? st.skins->reg.live() : 0;
}

} // namespace ark

extern "C" int ark_ddgi_debug_skin_host(const ArkDdgiSkinDesc* desc, const ArkDdgiSkinPose* pose, const float* prev_positions, float* out_positions, ArkRTVertex* out_vertices,
                                        float* out_velocities, float* out_bounds)
{
    using namespace ark;
    if (!pose || !out_positions || !out_vertices || !out_velocities || !out_bounds) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::unique_ptr<skin::SkinHost> h;
    std::string why;
    if (const int rc = skin::buildSkin(desc, h, why)) return rc;
    if (poseArguments(h.get(), *pose)) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::vector<float> packed(poseFloats(*h) + 1u);
    packPose(*h, *pose, packed.data());
    if (!skin::poseBound(*h, packed.data(), packed.data() + 12u * h->jointCount, out_bounds, why)) return ARK_DDGI_E_INVALID_ARGUMENT;
    skin::skinRun(*h, packed.data(), packed.data() + 12u * h->jointCount, prev_positions, out_positions, reinterpret_cast<float*>(out_vertices), out_velocities);
    return ARK_DDGI_OK;
}

extern "C" int ark_ddgi_debug_skin_device_parity(int device, const ArkDdgiSkinDesc* desc, const ArkDdgiSkinPose* pose, const float* prev_positions, uint32_t dst_first_vertex,
                                                 uint64_t* out)
{
    using namespace ark;
    if (!pose || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::unique_ptr<skin::SkinHost> h;
    std::string why;
    if (const int rc = skin::buildSkin(desc, h, why)) return rc;
    if (poseArguments(h.get(), *pose)) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::vector<float> packed(poseFloats(*h) + 1u);
    packPose(*h, *pose, packed.data());
    float bounds[6];
    if (!skin::poseBound(*h, packed.data(), packed.data() + 12u * h->jointCount, bounds, why)) return ARK_DDGI_E_INVALID_ARGUMENT;
    const size_t n = h->vertexCount, first = dst_first_vertex, guard = 4, total = first + n + guard;
    std::vector<float> hp(3 * n), hv(9 * n), hvel(3 * n);
    skin::skinRun(*h, packed.data(), packed.data() + 12u * h->jointCount, prev_positions, hp.data(), hv.data(), hvel.data());

    if (hipSetDevice(device) != hipSuccess) return ARK_DDGI_E_DEVICE;
    // the outputs start at vertex dst_first_vertex of larger arrays, as a destination range
    // of the pools would, with the words around them marked
    constexpr uint32_t kMark = 0x7fc0beefu; // (a NaN no arithmetic produces)
    DeviceSkin d;
    DeviceBuffer dp, dv, dvel, dprev;
    hipStream_t s = nullptr;
    hipEvent_t ev[2] = { nullptr, nullptr };
    std::vector<uint32_t> gp(3 * total), gv(9 * total), gvel(3 * total);
    float ms = 0.0f;
    auto run = [&]() -> hipError_t {
        hipError_t e = uploadSkin(*h, d);
        if (e == hipSuccess) e = dp.alloc(12u * total);
        if (e == hipSuccess) e = dv.alloc(36u * total);
        if (e == hipSuccess) e = dvel.alloc(12u * total);
        if (e == hipSuccess && prev_positions) e = dprev.alloc(12u * n);
        if (e == hipSuccess && prev_positions) e = hipMemcpy(dprev.ptr, prev_positions, 12u * n, hipMemcpyHostToDevice);
        if (e == hipSuccess && poseFloats(*h)) e = hipMemcpy(d.pose.ptr, packed.data(), poseFloats(*h) * 4u, hipMemcpyHostToDevice);
        const std::vector<uint32_t> marks(9 * total, kMark);
        for (DeviceBuffer* b : { &dp, &dv, &dvel })
            if (e == hipSuccess) e = hipMemcpy(b->ptr, marks.data(), b->bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        for (hipEvent_t& x : ev)
            if (e == hipSuccess) e = hipEventCreate(&x);
        const SkinArgs a = skinArgs(*h, d, dprev.as<float>(), dp.as<float>() + 3u * first, dv.as<float>() + 9u * first, dvel.as<float>() + 3u * first);
        if (e == hipSuccess) e = launch_skin_vertices(a, s);
        // the same run again, timed (it writes the same words)
        if (e == hipSuccess) e = hipEventRecord(ev[0], s);
        if (e == hipSuccess) e = launch_skin_vertices(a, s);
        if (e == hipSuccess) e = hipEventRecord(ev[1], s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
        if (e == hipSuccess) e = hipMemcpy(gp.data(), dp.ptr, 12u * total, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(gv.data(), dv.ptr, 36u * total, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(gvel.data(), dvel.ptr, 12u * total, hipMemcpyDeviceToHost);
        return e;
    };
    const hipError_t e = run();
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    if (s) (void)hipStreamDestroy(s);
    d.release();
    for (DeviceBuffer* b : { &dp, &dv, &dvel, &dprev }) b->release();
    if (e != hipSuccess) return ARK_DDGI_E_DEVICE;

    // by bits; a NaN equals any NaN
    auto compare = [&](const std::vector<uint32_t>& got, const std::vector<float>& want, size_t fpv, uint64_t& differ, uint64_t& marksLost) {
        for (size_t w = 0; w < got.size(); ++w) {
            if (w < first * fpv || w >= (first + n) * fpv) {
                marksLost += got[w] != kMark;
                continue;
            }
            const float x = want[w - first * fpv];
            const float g = u2f(got[w]);
            differ += !(f2u(x) == got[w] || (x != x && g != g));
        }
    };
    out[0] = out[1] = out[2] = out[3] = 0;
    compare(gp, hp, 3, out[0], out[3]);
    compare(gv, hv, 9, out[1], out[3]);
    compare(gvel, hvel, 3, out[2], out[3]);
    out[4] = static_cast<uint64_t>(static_cast<double>(ms) * 1e6);
    return ARK_DDGI_OK;
}
