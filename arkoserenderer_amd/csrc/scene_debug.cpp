// scene_debug.cpp — the debug downloads of the front copy (scene_store.h: the digest, the
// installed-BVH checks, the last refit's reach).
#include "../../include/ark_ddgi_debug.h"
#include "bvh8_check.h"
#include "path_tracer_host.h"
#include "scene_store_internal.h"

namespace ark {

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

int sceneRecordsAndClasses(const SceneStore& st, ErrorSink* err, std::vector<uint32_t>& records, std::vector<int32_t>& classOf)
{
    static_assert(sizeof(GpuTriangle) == 48, "12 words per record");
    records.assign(static_cast<size_t>(st.world.records) * 12u, 0u);
    if (!records.empty()) ARK_HIP(hipMemcpy(records.data(), st.args.tris, records.size() * 4u, hipMemcpyDeviceToHost));
    const std::vector<int> cls = instanceClasses(st);
    classOf.assign(cls.begin(), cls.end());
    return ARK_DDGI_OK;
}

int sceneHostCopy(const SceneStore& st, ErrorSink* err, pt::HostScene& out)
{
    auto fetch = [&](auto& vec, const void* dev, size_t count) -> hipError_t {
        vec.resize(count);
        return count ? hipMemcpy(vec.data(), dev, count * sizeof(vec[0]), hipMemcpyDeviceToHost) : hipSuccess;
    };
    static_assert(sizeof(pt::F4) == 16, "a texel");
    ARK_HIP(fetch(out.tris, st.args.tris, st.world.records));
    ARK_HIP(fetch(out.indices, st.args.indices, st.indices.bytes / sizeof(uint32_t)));
    ARK_HIP(fetch(out.vertices, st.args.vertices, st.vertices.bytes / sizeof(float)));
    ARK_HIP(fetch(out.meshes, st.args.meshes, st.meshes.bytes / sizeof(ArkRTTriangleMesh)));
    ARK_HIP(fetch(out.materials, st.args.materials, st.materials.bytes / sizeof(ArkShaderMaterial)));
    ARK_HIP(fetch(out.instances, st.args.instances, st.instHost.size()));
    ARK_HIP(fetch(out.texInfos, st.args.tex_infos, st.texInfos.bytes / sizeof(GpuTextureInfo)));
    ARK_HIP(fetch(out.texels, st.args.texels, st.texels.bytes / sizeof(pt::F4)));
    out.textureCount = st.args.texture_count;
    out.whiteTexture = st.args.white_texture;
    out.envTexture = st.args.env_texture;
    return ARK_DDGI_OK;
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
