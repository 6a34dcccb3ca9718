// scene_build.cpp — ark_ddgi_set_scene's host preprocessing and build (scene_store.h:
// buildScene), its steps in the order they run.
#include <chrono>
#include <cmath>
#include <mutex>

#include "scene_store_internal.h"

#include "ark_fmath.h"
#include "bvh8_check.h"
#include "shading_math.h"
#include "sun_bvh.h"

namespace ark {

// (GpuScene.cpp:844-858: the fields of LightData.h:19-40 the DDGI path uses)
GpuSpotLight gpuSpotLight(const ArkSpotLight& sl)
{
    GpuSpotLight g;
    std::memset(&g, 0, sizeof(g));
    for (int k = 0; k < 3; ++k) {
        g.color[k] = sl.color[k];
        g.direction[k] = sl.world_space_direction[k];
        g.right[k] = sl.world_space_right[k];
        g.up[k] = sl.world_space_up[k];
        g.position[k] = sl.world_space_position[k];
    }
    g.position[3] = sl.outer_cone_half_angle;
    g.ies_texture = sl.ies_profile_index;
    return g;
}

// An instance in the shading kernels' table: the rows of its transform, its facing flip
// (det(ObjectToWorld) < 0), hit mask and material
GpuInstance gpuInstance(const ArkRTInstance& inst, const ArkRTTriangleMesh& mesh)
{
    const float* M = inst.object_to_world;
    const float det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
    GpuInstance g;
    std::memset(&g, 0, sizeof(g));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) g.normal_matrix[r * 4 + c] = M[r * 4 + c];
    g.rt_mesh_index = static_cast<int32_t>(inst.rt_mesh_index);
    g.flip_facing = det < 0.0f ? 1 : 0;
    g.hit_mask = static_cast<int32_t>(inst.hit_mask);
    g.material_index = mesh.material_index;
    return g;
}

namespace {

// f(begin, end) over [0, n) in `threads` contiguous chunks (one when n is small)
template<class F>
void parallelFor(size_t n, int threads, F f)
{
    const int T = std::max(1, std::min<int>(threads, static_cast<int>(n >> 16) + 1));
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back([&, t] { f(n * t / T, n * (t + 1) / T); });
    f(0, n / T);
    for (std::thread& th : pool) th.join();
}

int validateScene(ErrorSink* err,const ArkDdgiScene* s)
{
    for (uint32_t i = 0; i < s->instance_count; ++i) {
        const ArkRTInstance& inst = s->instances[i];
        if (inst.rt_mesh_index >= s->mesh_count) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u: rt_mesh_index out of range", i);
        const ArkRTTriangleMesh& m = s->meshes[inst.rt_mesh_index];
        if (m.material_index < 0 || static_cast<uint32_t>(m.material_index) >= s->material_count)
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "mesh %u: material_index out of range", inst.rt_mesh_index);
        if (static_cast<uint64_t>(m.first_index) + 3ull * inst.triangle_count > s->index_count)
            return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u: indices out of range", i);
    }
    if (s->spot_light_count > ARK_DDGI_MAX_SPOT_LIGHTS || (s->spot_light_count && !s->spot_lights))
        return err->fail(ARK_DDGI_E_UNSUPPORTED, "at most %d spot lights (GpuScene.cpp:430)", ARK_DDGI_MAX_SPOT_LIGHTS);
    return ARK_DDGI_OK;
}

// World-space triangles per hit-mask class (GpuScene.cpp:883-929: one TLAS instance per
// mesh segment; flattened here into one BVH per class) and the instance table.
int flattenInstances(ErrorSink* err,const ArkDdgiScene* s, std::vector<BuildTriangle> cls[3], std::vector<GpuInstance>& ginst)
{
    ginst.resize(s->instance_count);
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) {
        const ArkRTInstance& inst = s->instances[ii];
        const ArkRTTriangleMesh& m = s->meshes[inst.rt_mesh_index];
        const float* M = inst.object_to_world;
        const GpuInstance& g = ginst[ii] = gpuInstance(inst, m);
        const int c = hit_mask_class(inst.hit_mask);
        for (uint32_t p = 0; p < inst.triangle_count; ++p) {
            BuildTriangle t;
            float* w[3] = { t.v0, t.v1, t.v2 };
            for (int k = 0; k < 3; ++k) {
                const uint32_t idx = s->indices[static_cast<size_t>(m.first_index) + 3u * p + k];
                const uint64_t vi = static_cast<uint64_t>(m.first_vertex) + idx;
                if (vi >= s->vertex_count) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "instance %u prim %u: vertex out of range", ii, p);
                const float* P = &s->positions[vi * 3];
                w[k][0] = M[0] * P[0] + M[1] * P[1] + M[2] * P[2] + M[3];
                w[k][1] = M[4] * P[0] + M[5] * P[1] + M[6] * P[2] + M[7];
                w[k][2] = M[8] * P[0] + M[9] * P[1] + M[10] * P[2] + M[11];
            }
            t.instance = ii;
            t.primitive = p;
            t.flip_facing = static_cast<uint32_t>(g.flip_facing);
            cls[c].push_back(t);
        }
    }
    return ARK_DDGI_OK;
}

// textures: decoded to float4 texels (sRGB EOTF per texel), + trailing 1x1 white
int decodeTextures(ErrorSink* err,const ArkDdgiScene* s, std::vector<GpuTextureInfo>& infos, std::vector<float>& texels)
{
    for (uint32_t i = 0; i <= s->texture_count; ++i) {
        GpuTextureInfo ti {};
        ti.texel_offset = texels.size() / 4;
        if (i == s->texture_count) {
            ti.width = ti.height = 1;
            ti.wrap = ARK_WRAP_REPEAT;
            texels.insert(texels.end(), { 1.0f, 1.0f, 1.0f, 1.0f });
        } else {
            const ArkTexture& t = s->textures[i];
            if (t.width <= 0 || t.height <= 0 || !t.data) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u invalid", i);
            ti.width = t.width;
            ti.height = t.height;
            // per-axis wrap, s in bits 0-3 and t in 4-7 (ARK_WRAP_AXES)
            const int ws = (t.wrap & ARK_WRAP_PER_AXIS) ? (t.wrap & 0xf) : t.wrap, wt = (t.wrap & ARK_WRAP_PER_AXIS) ? ((t.wrap >> 4) & 0xf) : t.wrap;
            if (ws < ARK_WRAP_REPEAT || ws > ARK_WRAP_MIRRORED_REPEAT || wt < ARK_WRAP_REPEAT || wt > ARK_WRAP_MIRRORED_REPEAT ||
                ((t.wrap & ARK_WRAP_PER_AXIS) && (t.wrap & ~0x1ff)))
                return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u: unknown wrap mode 0x%x", i, t.wrap);
            ti.wrap = ws | (wt << 4);
            const size_t n = static_cast<size_t>(t.width) * t.height;
            for (size_t p = 0; p < n; ++p)
                for (int c = 0; c < 4; ++c) {
                    float v = 0.0f;
                    if (!dev::decodeTexel(t.format, t.data, p, c, &v)) return err->fail(ARK_DDGI_E_INVALID_ARGUMENT, "texture %u: unknown format", i);
                    texels.push_back(v);
                }
        }
        infos.push_back(ti);
    }
    return ARK_DDGI_OK;
}

// every instance's object-space box (refitInflations) and every RT mesh's vertex span: the
// largest index any instance of it draws (which instances a vertex update touches)
void instanceObjectBoxes(const ArkDdgiScene* s, int threads, std::vector<std::array<float, 6>>& boxes, std::vector<MeshSpan>& spans)
{
    boxes.assign(s->instance_count, { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY });
    spans.assign(s->mesh_count, MeshSpan {});
    for (uint32_t ii = 0; ii < s->instance_count; ++ii) {
        const ArkRTInstance& in = s->instances[ii];
        const ArkRTTriangleMesh& mesh = s->meshes[in.rt_mesh_index];
        std::array<float, 6>& box = boxes[ii];
        MeshSpan& span = spans[in.rt_mesh_index];
        span.first = mesh.first_vertex;
        std::mutex mu;
        parallelFor(static_cast<size_t>(in.triangle_count) * 3u, threads, [&](size_t b, size_t e) {
            float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
            uint32_t most = 0;
            for (size_t k = b; k < e; ++k) {
                most = std::max(most, s->indices[static_cast<size_t>(mesh.first_index) + k]);
                const float* P = s->positions + (static_cast<int64_t>(mesh.first_vertex) + s->indices[static_cast<size_t>(mesh.first_index) + k]) * 3;
                for (int a = 0; a < 3; ++a) {
                    lo[a] = std::min(lo[a], P[a]);
                    hi[a] = std::max(hi[a], P[a]);
                }
            }
            std::lock_guard<std::mutex> g(mu);
            for (int a = 0; a < 3; ++a) {
                box[a] = std::min(box[a], lo[a]);
                box[3 + a] = std::max(box[3 + a], hi[a]);
            }
            if (e > b) {
                span.maxIndex = std::max(span.maxIndex, most);
                span.used = true;
            }
        });
    }
}

// per-triangle shading records (GpuTriangle order, 64 B): the three vertex normals, the
// instance and the three UVs, copied from the vertex pool, so the shading and shadow-ray
// kernels reach a hit's surface in one fetch instead of instance -> mesh -> indices ->
// vertices
void shadingRecords(const ArkDdgiScene* s, const std::vector<GpuTriangle>& tris, int threads, std::vector<float>& tn)
{
    tn.assign(tris.size() * 16, 0.0f);
    parallelFor(tris.size(), threads, [&](size_t b, size_t e) {
        for (size_t t = b; t < e; ++t) {
            if (isHoleTriangle(tris[t])) continue; // never hit: no record
            uint32_t inst, prim;
            std::memcpy(&inst, &tris[t].t2[1], 4);
            std::memcpy(&prim, &tris[t].t2[2], 4);
            const ArkRTTriangleMesh& mesh = s->meshes[s->instances[inst].rt_mesh_index];
            float* o = tn.data() + t * 16;
            for (int q = 0; q < 3; ++q) {
                const uint32_t idx = s->indices[static_cast<size_t>(mesh.first_index) + 3u * prim + q];
                const float* v = reinterpret_cast<const float*>(s->vertices) + (static_cast<size_t>(mesh.first_vertex) + idx) * 9;
                for (int k = 0; k < 3; ++k) o[q * 3 + k] = v[2 + k];
                o[10 + 2 * q] = v[0];
                o[11 + 2 * q] = v[1];
            }
            std::memcpy(o + 9, &inst, 4);
        }
    });
    if (tn.empty()) tn.assign(16, 0.0f);
}

// the store's refit stream and the events that order its copies (scene_store.h)
hipError_t createOrdering(SceneStore& st)
{
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&st.refitStream, hipStreamNonBlocking, hi);
    for (hipEvent_t* ev : { &st.frontFree, &st.spare[0].free, &st.spare[1].free, &st.evInstalled, &st.evGeometry })
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    return e;
}

} // namespace

int buildScene(ErrorSink* err, const ArkDdgiScene* s, int device, int buildThreads, int sunBvh, bool coverMap, std::shared_ptr<SceneStore>& out)
{
    auto st = std::make_shared<SceneStore>();
    st->device = device;
    ARK_HIP(createOrdering(*st));
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    if ((rc = validateScene(err, s)) != 0) return rc;
    std::vector<BuildTriangle> cls[3];
    std::vector<GpuInstance> ginst;
    if ((rc = flattenInstances(err, s, cls, ginst)) != 0) return rc;
    // host threads for the build (ArkDdgiDesc.build_threads; 0: the box's CPU share per
    // GPU, 16 cores)
    BvhBuildOptions opt;
    opt.threads = buildThreads > 0 ? buildThreads : 16;
    // BVH2 -> BVH8 child selection: SAH-optimal (Ylitie et al. 2017 DP) with the default
    // node / triangle costs (a lower triangle cost and the greedy collapse measured no
    // better)
    Bvh8CollapseOptions copt;
    copt.threads = opt.threads;
    // the sun's light-space BVH input, before the class builds free their triangles; the
    // build itself on its own thread beside the class builds (each build's top levels
    // leave cores idle: C4 setup 13.5 -> s)
    const bool sunInput = s->has_directional_light && sunBvh != 0;
    SunBvhInput sunIn;
    Bvh8BuildResult r; // the sun's
    bool sunBuilt = false, sunOk = true;
    float sunBuildMs = 0.0f;
    struct Joiner {
        std::thread t;
        ~Joiner()
        {
            if (t.joinable()) t.join();
        }
    } sunThread;
    if (sunInput) {
        const auto ts0 = std::chrono::steady_clock::now();
        sun_frame(s->directional_light.world_space_direction, sunIn.frame);
        for (int c = 0; c < 3; ++c) sun_add_triangles(sunIn, cls[c], opt.threads);
        sunBuilt = !sunIn.tris.empty();
        if (sunBuilt)
            sunThread.t = std::thread([&sunIn, &opt, &copt, &r, &sunOk, &sunBuildMs, ts0] {
                sunOk = build_sun_bvh(sunIn, opt, copt, r);
                sunBuildMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - ts0).count();
            });
    }
    WorldBvh8 w;
    std::string why;
    if (!build_world_bvh8(cls, opt, copt, w, why)) return err->fail(w.tooLarge ? ARK_DDGI_E_UNSUPPORTED : ARK_DDGI_E_DEVICE, "%s", why.c_str());
    std::vector<GpuTextureInfo> infos;
    std::vector<float> texels;
    if ((rc = decodeTextures(err, s, infos, texels)) != 0) return rc;
    std::vector<GpuSpotLight> gspots(s->spot_light_count);
    for (uint32_t i = 0; i < s->spot_light_count; ++i) gspots[i] = gpuSpotLight(s->spot_lights[i]);
    // (the traversal's 32-bit byte offset: nodes and records must stay below 4 GiB)
    if (DeviceBvh::bytesFor(w.nodes.size(), w.tris.size()) >= (1ull << 32)) return err->fail(ARK_DDGI_E_UNSUPPORTED, "BVH nodes + triangles exceed 4 GiB");
    ARK_HIP(uploadBvh(w.nodes, w.tris, nullptr, st->world));
    st->world.depth = w.depth;
    st->world.inflateAbs = w.inflateAbs;
    if (sunThread.t.joinable()) sunThread.t.join();
    const auto ts0 = std::chrono::steady_clock::now();
    const int32_t sroot = 0;
    if (sunBuilt) {
        if (!sunOk) return err->fail(ARK_DDGI_E_DEVICE, "sun BVH2 leaf over %d triangles", kBvh8MaxLeafSize);
        if (!checkBvh8Structure(r.nodes, r.tris, &sroot, 1, why)) return err->fail(ARK_DDGI_E_DEVICE, "%s", why.c_str());
        // by cost unless forced: sample sun shadow rays through both structures on the host
        const float* sd = s->directional_light.world_space_direction;
        const float dd = sd[0] * sd[0] + sd[1] * sd[1] + sd[2] * sd[2];
        const float isc = 1.0f / std::sqrt(dd);
        const float L[3] = { -(sd[0] * isc), -(sd[1] * isc), -(sd[2] * isc) };
        std::vector<float> origins;
        sun_sample_origins(w.tris, L, 4096u, origins);
        st->sunCostWorld = static_cast<float>(sun_shadow_cost(w.nodes, w.tris, w.roots, 3, nullptr, L, origins));
        st->sunCostLight = static_cast<float>(sun_shadow_cost(r.nodes, r.tris, &sroot, 1, sunIn.frame, L, origins));
    }
    st->sunArgs.sun_root = -1;
    if (sunBuilt && (sunBvh == 1 ||sun_bvh_pays(st->sunCostWorld, st->sunCostLight))) {
        DeviceBvh sb;
        std::vector<uint32_t> order;
        if (!bvhLevelOrder(r.nodes.data(), r.nodes.size(), &sroot, 1, order, sb.levelOffsets)) return err->fail(ARK_DDGI_E_DEVICE, "sun BVH: a node outside it");
        sb.depth = r.max_depth;
        sb.inflateAbs = sunIn.inflateAbs;
        sb.nodeCount = r.nodes.size(); // (the install sizes the refit's boxes scratch from it, ahead of its upload)
        rc = upload(err, sb.order, order.data(), order.size());
        if (rc == 0) rc = installSunBvh(err, *st, sb, &r, &sunIn.frame[0][0], s->directional_light.world_space_direction, nullptr);
        sb.order.release(); // (a failure before the install took it)
        if (rc != 0) return rc;
    }
    sunBuildMs += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - ts0).count();
    std::vector<GpuTriangle>().swap(sunIn.world);
    if ((rc = upload(err, st->indices, s->indices, s->index_count)) != 0) return rc;
    if ((rc = upload(err, st->vertices, reinterpret_cast<const float*>(s->vertices), s->vertex_count * 9)) != 0) return rc;
    if ((rc = upload(err, st->positions, s->positions, s->vertex_count * 3)) != 0) return rc;
    st->instHost.assign(s->instances, s->instances + s->instance_count);
    // the transforms every geometry copy holds (the spares are made at their first refits)
    st->book.newScene(s->instances, s->instance_count);
    st->meshHost.assign(s->meshes, s->meshes + s->mesh_count);
    instanceObjectBoxes(s, opt.threads, st->instObjBox, st->meshSpans);
    st->vertexCount = s->vertex_count;
    if ((rc = upload(err, st->meshes, s->meshes, s->mesh_count)) != 0) return rc;
    if ((rc = upload(err, st->materials, s->materials, s->material_count)) != 0) return rc;
    if ((rc = upload(err, st->instances, ginst.data(), ginst.size())) != 0) return rc;
    if ((rc = upload(err, st->texInfos, infos.data(), infos.size())) != 0) return rc;
    if ((rc = upload(err, st->texels, texels.data(), texels.size())) != 0) return rc;
    {
        std::vector<float> tn;
        shadingRecords(s, w.tris, opt.threads, tn);
        if ((rc = upload(err, st->triNormals, tn.data(), tn.size())) != 0) return rc;
    }
    SceneArgs& sc = st->args;
    setGeometryArgs(*st);
    setWorldRoots(*st, w.roots, w.opaqueNodes, w.opaqueRecords);
    sc.tri_normals = st->triNormals.as<float4>();
    sc.texture_count = static_cast<int32_t>(s->texture_count);
    sc.indices = st->indices.as<uint32_t>();
    sc.vertices = st->vertices.as<float>();
    sc.meshes = st->meshes.as<ArkRTTriangleMesh>();
    sc.materials = st->materials.as<ArkShaderMaterial>();
    sc.tex_infos = st->texInfos.as<GpuTextureInfo>();
    sc.texels = st->texels.as<float4>();
    sc.white_texture = static_cast<int32_t>(s->texture_count);
    sc.env_texture = (s->environment_texture >= 0 && static_cast<uint32_t>(s->environment_texture) < s->texture_count) ? s->environment_texture : sc.white_texture;
    sc.sun_root = -1;
    // lights: the scene's are each context's until ark_ddgi_set_lights (deriveSceneArgs)
    st->hasSunScene = s->has_directional_light ? 1 : 0;
    st->sunScene = s->directional_light;
    st->spotsScene = std::move(gspots);
    st->sunWanted = st->sun.nodeCount > 0;
    st->buildThreads = opt.threads;
    // the sun's cover map, on the device from the records just uploaded (no map: a scene
    // it does not take, sun_cover_map.h; every sun ray is then traced)
    st->coverWanted = coverMap;
    if (coverMap && s->has_directional_light && st->world.records > 0) {
        const auto tc = std::chrono::steady_clock::now();
        double frame[3][3];
        sun_frame(s->directional_light.world_space_direction, frame);
        float L[3];
        sunRayDirection(s->directional_light.world_space_direction, L);
        cover::Grid grid {};
        DeviceBuffer buf;
        bool ok = false;
        ARK_HIP(deviceBuildCoverMap(st->world.tris(st->world.buf), st->world.records, &frame[0][0], L, cover::kDefaultBudget, nullptr, grid, buf, ok));
        if (ok) setCoverMap(*st, buf, grid, s->directional_light.world_space_direction, &frame[0][0], std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tc).count());
    }
    // the sun's traversal pushes onto the same spill area (its depth counts)
    st->bvhMaxDepth = std::max(st->world.depth, st->sun.depth);
    const auto t1 = std::chrono::steady_clock::now();
    st->bvhStats.node_count = w.nodes.size();
    st->bvhStats.triangle_count = w.triangles;
    st->bvhStats.max_depth = st->bvhMaxDepth;
    st->bvhStats.max_leaf_size = w.maxLeaf;
    st->bvhStats.sah_cost = w.sah;
    st->bvhStats.build_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
    st->bvhStats.node_bytes = w.nodes.size() * sizeof(GpuBvh8Node);
    st->bvhStats.triangle_bytes = w.tris.size() * sizeof(GpuTriangle);
    st->bvhStats.sun_node_count = st->sun.nodeCount;
    st->bvhStats.sun_max_depth = st->sun.depth;
    st->bvhStats.sun_cost_world = st->sunCostWorld;
    st->bvhStats.sun_cost_light = st->sunCostLight;
    st->bvhStats.sun_build_ms = sunBuildMs;
    out = std::move(st);
    return ARK_DDGI_OK;
}

} // namespace ark
