// path_tracer_host.cpp — see path_tracer_host.h; at the end the host-only
// ark_ddgi_debug_path_tracer_* entries (include/ark_ddgi_debug.h), which need nothing else of
// the library.
#include "path_tracer_host.h"

#include <cmath>
#include <cstddef>
#include <cstring>

#include "../../include/ark_ddgi_debug.h"
#include "refl_denoise.h"

namespace ark {
namespace pt {

HostView HostScene::view() const
{
    HostView v {};
    v.tris = tris.data();
    v.indices = indices.data();
    v.vertices = vertices.data();
    v.meshes = meshes.data();
    v.materials = materials.data();
    v.instances = instances.data();
    v.tex_infos = texInfos.data();
    v.texels = texels.data();
    v.texture_count = textureCount;
    v.white_texture = whiteTexture;
    v.env_texture = envTexture;
    v.has_sun = hasSun;
    v.spot_count = static_cast<int32_t>(spots.size());
    for (int k = 0; k < 3; ++k) {
        v.sun_color[k] = sunColor[k];
        v.sun_dir[k] = sunDir[k];
    }
    v.spots = spots.data();
    return v;
}

// ark_ddgi_set_scene's host preprocessing without a device (scene_build.cpp: flattenInstances,
// gpuInstance, gpuSpotLight, decodeTextures; bvh_builder.cpp: the record of a triangle), the
// records in (instance, primitive) order. The texel decode is shading_math.h's.
int hostSceneFrom(const ArkDdgiScene& s, HostScene& out)
{
    out = HostScene {};
    for (uint32_t ii = 0; ii < s.instance_count; ++ii) {
        const ArkRTInstance& inst = s.instances[ii];
        if (inst.rt_mesh_index >= s.mesh_count) return -1;
        const ArkRTTriangleMesh& m = s.meshes[inst.rt_mesh_index];
        if (m.material_index < 0 || static_cast<uint32_t>(m.material_index) >= s.material_count) return -1;
        if (static_cast<uint64_t>(m.first_index) + 3ull * inst.triangle_count > s.index_count) return -1;
        const float* M = inst.object_to_world;
        const float det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
        GpuInstance g;
        std::memset(&g, 0, sizeof(g));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) g.normal_matrix[r * 4 + c] = M[r * 4 + c];
        g.rt_mesh_index = static_cast<int32_t>(inst.rt_mesh_index);
        g.flip_facing = det < 0.0f ? 1 : 0;
        g.hit_mask = static_cast<int32_t>(inst.hit_mask);
        g.material_index = m.material_index;
        out.instances.push_back(g);
        for (uint32_t p = 0; p < inst.triangle_count; ++p) {
            float w[3][3];
            for (int k = 0; k < 3; ++k) {
                const uint32_t idx = s.indices[static_cast<size_t>(m.first_index) + 3u * p + k];
                const uint64_t vi = static_cast<uint64_t>(m.first_vertex) + idx;
                if (vi >= s.vertex_count) return -1;
                const float* P = &s.positions[vi * 3];
                w[k][0] = M[0] * P[0] + M[1] * P[1] + M[2] * P[2] + M[3];
                w[k][1] = M[4] * P[0] + M[5] * P[1] + M[6] * P[2] + M[7];
                w[k][2] = M[8] * P[0] + M[9] * P[1] + M[10] * P[2] + M[11];
            }
            GpuTriangle t;
            float e1[3], e2[3];
            for (int a = 0; a < 3; ++a) {
                e1[a] = w[1][a] - w[0][a];
                e2[a] = w[2][a] - w[0][a];
            }
            t.t0[0] = w[0][0]; t.t0[1] = w[0][1]; t.t0[2] = w[0][2]; t.t0[3] = e1[0];
            t.t1[0] = e1[1]; t.t1[1] = e1[2]; t.t1[2] = e2[0]; t.t1[3] = e2[1];
            t.t2[0] = e2[2];
            t.t2[1] = u2f(ii);
            t.t2[2] = u2f(p);
            t.t2[3] = u2f(static_cast<uint32_t>(g.flip_facing));
            out.tris.push_back(t);
        }
    }
    out.indices.assign(s.indices, s.indices + s.index_count);
    const float* vtx = reinterpret_cast<const float*>(s.vertices);
    out.vertices.assign(vtx, vtx + s.vertex_count * 9);
    out.meshes.assign(s.meshes, s.meshes + s.mesh_count);
    out.materials.assign(s.materials, s.materials + s.material_count);
    for (uint32_t i = 0; i <= s.texture_count; ++i) {
        GpuTextureInfo ti {};
        ti.texel_offset = out.texels.size();
        if (i == s.texture_count) {
            ti.width = ti.height = 1;
            ti.wrap = ARK_WRAP_REPEAT;
            out.texels.push_back(F4 { 1.0f, 1.0f, 1.0f, 1.0f });
        } else {
            const ArkTexture& t = s.textures[i];
            if (t.width <= 0 || t.height <= 0 || !t.data) return -1;
            ti.width = t.width;
            ti.height = t.height;
            const int ws = (t.wrap & ARK_WRAP_PER_AXIS) ? (t.wrap & 0xf) : t.wrap, wt = (t.wrap & ARK_WRAP_PER_AXIS) ? ((t.wrap >> 4) & 0xf) : t.wrap;
            if (ws < ARK_WRAP_REPEAT || ws > ARK_WRAP_MIRRORED_REPEAT || wt < ARK_WRAP_REPEAT || wt > ARK_WRAP_MIRRORED_REPEAT) return -1;
            ti.wrap = ws | (wt << 4);
            const size_t n = static_cast<size_t>(t.width) * t.height;
            for (size_t p = 0; p < n; ++p) {
                float c[4];
                for (int k = 0; k < 4; ++k)
                    if (!dev::decodeTexel(t.format, t.data, p, k, &c[k])) return -1;
                out.texels.push_back(F4 { c[0], c[1], c[2], c[3] });
            }
        }
        out.texInfos.push_back(ti);
    }
    out.textureCount = static_cast<int32_t>(s.texture_count);
    out.whiteTexture = out.textureCount;
    out.envTexture = (s.environment_texture >= 0 && static_cast<uint32_t>(s.environment_texture) < s.texture_count) ? s.environment_texture : out.whiteTexture;
    out.hasSun = s.has_directional_light ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
        out.sunColor[k] = s.directional_light.color[k];
        out.sunDir[k] = s.directional_light.world_space_direction[k];
    }
    if (s.spot_light_count > ARK_DDGI_MAX_SPOT_LIGHTS || (s.spot_light_count && !s.spot_lights)) return -1;
    for (uint32_t i = 0; i < s.spot_light_count; ++i) {
        const ArkSpotLight& sl = s.spot_lights[i];
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
        out.spots.push_back(g);
    }
    return 0;
}

const char* descProblem(const ArkPathTracerDesc& d)
{
    if (d.flags & ~(ARK_PATH_TRACER_RESET | ARK_PATH_TRACER_ACCUMULATE)) return "unknown flag";
    if ((d.flags & ARK_PATH_TRACER_RESET) && (d.flags & ARK_PATH_TRACER_ACCUMULATE)) return "reset and accumulate in one call";
    if (d.flags && !d.accumulation) return "a flag without an accumulation plane";
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(d.world_from_view[k]) || !std::isfinite(d.view_from_projection[k])) return "non-finite camera matrix";
    if (!std::isfinite(d.environment_multiplier) || !std::isfinite(d.z_near) || !std::isfinite(d.z_far)) return "non-finite scalar";
    const uint64_t pixels = static_cast<uint64_t>(d.width) * d.height;
    if (pixels >= (1ull << 28)) return "target too large: a shadow ray's owner word is (path << 4) | light";
    if (pixels == 0) return nullptr;
    if (!d.image) return "no image";
    const uintptr_t img = reinterpret_cast<uintptr_t>(d.image), acc = reinterpret_cast<uintptr_t>(d.accumulation);
    if (img % 8u) return "image not aligned to its texel";
    if (d.flags) {
        if (acc % 16u) return "accumulation not aligned to its texel";
        if (img < acc + pixels * 16u && acc < img + pixels * 8u) return "image and accumulation overlap";
    }
    return nullptr;
}

namespace {

struct Hit {
    float t, u, v;
    uint32_t tri, inst, prim;
    bool backface;
};

int classOf(const HostView& sc, uint32_t inst)
{
    switch (static_cast<uint32_t>(sc.instances[inst].hit_mask)) {
    case ARK_RT_HIT_MASK_OPAQUE: return 0;
    case ARK_RT_HIT_MASK_MASKED: return 1;
    case ARK_RT_HIT_MASK_BLEND: return 2;
    default: return -1;
    }
}

// travStepDual's acceptance over every record: closest hit in [tmin, tmax] of the three
// classes, ties to the smaller (instance, primitive), the alpha test on class 1
Hit closestHit(const HostView& sc, uint64_t nRecords, V3 o, V3 d, float tmin, float tmax, uint32_t* alphaRejected)
{
    Hit h { tmax, 0.0f, 0.0f, 0xffffffffu, 0u, 0u, false };
    for (uint64_t i = 0; i < nRecords; ++i) {
        const GpuTriangle& g = sc.tris[i];
        const uint32_t inst = f2u(g.t2[1]), prim = f2u(g.t2[2]);
        if (inst == kHoleInstance) continue;
        const int c = classOf(sc, inst);
        if (c < 0) continue;
        float tt, uu, vv;
        bool bf;
        if (!dev::intersectTri(o, d, tmin, h.t, g, &tt, &uu, &vv, &bf)) continue;
        if (h.tri != 0xffffffffu && tt == h.t && (inst > h.inst || (inst == h.inst && prim > h.prim))) continue;
        if (c == 1 && !alphaAccept(sc, inst, prim, uu, vv)) {
            ++*alphaRejected;
            continue;
        }
        h = Hit { tt, uu, vv, static_cast<uint32_t>(i), inst, prim, bf != (f2u(g.t2[3]) != 0u) };
    }
    return h;
}

// k_trace_shadow<kShadowPath>: any hit of the opaque and masked classes in [0.025, tmax]
bool occluded(const HostView& sc, uint64_t nRecords, V3 o, V3 d, float tmax)
{
    if (!(tmax >= kShadowTmin)) return false;
    for (uint64_t i = 0; i < nRecords; ++i) {
        const GpuTriangle& g = sc.tris[i];
        const uint32_t inst = f2u(g.t2[1]);
        if (inst == kHoleInstance) continue;
        const int c = classOf(sc, inst);
        if (c != 0 && c != 1) continue;
        float tt, uu, vv;
        bool bf;
        if (dev::intersectTri(o, d, kShadowTmin, tmax, g, &tt, &uu, &vv, &bf)) return true;
    }
    return false;
}

void put3(float* dst, V3 v)
{
    dst[0] = v.x;
    dst[1] = v.y;
    dst[2] = v.z;
}

} // namespace

void hostAccumulate(const ArkPathTracerDesc& d)
{
    const uint64_t pixels = static_cast<uint64_t>(d.width) * d.height;
    for (uint64_t p = 0; p < pixels; ++p) {
        const uint16_t* texel = d.image + 4 * p;
        float* acc = d.accumulation + 4 * p;
        if (d.flags & ARK_PATH_TRACER_RESET) {
            for (int c = 0; c < 4; ++c) acc[c] = refl::h2f(texel[c]);
        } else {
            for (int c = 0; c < 3; ++c) acc[c] = accumulate(acc[c], refl::h2f(texel[c]), d.accumulated_frames);
            acc[3] = 1.0f;
        }
    }
}

int hostPathTrace(const HostView& sc, uint64_t nRecords, const ArkPathTracerDesc& d, Vertex* vertices, uint64_t* counts)
{
    if (descProblem(d)) return -1;
    uint64_t cnt[kCounts] = {};
    const uint64_t pixels = static_cast<uint64_t>(d.width) * d.height;
    if (vertices && pixels) std::memset(vertices, 0, sizeof(Vertex) * pixels * kMaxSegments);
    const uint32_t lightCount = static_cast<uint32_t>(sc.has_sun ? 1 : 0) + static_cast<uint32_t>(sc.spot_count);
    for (uint32_t py = 0; py < d.height; ++py)
        for (uint32_t px = 0; px < d.width; ++px) {
            const uint64_t p = static_cast<uint64_t>(py) * d.width + px;
            V3 origin, direction;
            PathState s = cameraRay(px, py, d.width, d.height, d.frame_index, d.world_from_view, d.view_from_projection, &origin, &direction);
            float tmin = d.z_near;
            // k_pt_setup, then per segment k_trace / k_pt_hit / k_trace_shadow / k_pt_shade
            for (uint32_t seg = 0; seg < kMaxSegments; ++seg) {
                Vertex scratch;
                Vertex& vx = vertices ? vertices[p * kMaxSegments + seg] : scratch;
                std::memset(&vx, 0, sizeof(Vertex));
                vx.rngBefore = s.rng;
                put3(vx.origin, origin);
                put3(vx.direction, direction);
                vx.tmin = tmin;
                put3(vx.attenuationBefore, s.attenuation);
                put3(vx.radianceBefore, s.radiance);
                cnt[7]++;
                if (seg == 8) cnt[3]++;
                uint32_t rejected = 0;
                const Hit h = closestHit(sc, nRecords, origin, direction, tmin, d.z_far, &rejected);
                vx.alphaRejected = rejected;
                cnt[1] += rejected;
                vx.tri = h.tri;
                bool ends = true;
                if (h.tri == 0xffffffffu) {
                    s.radiance = missRadiance(sc, direction, d.environment_multiplier, s.attenuation, s.radiance);
                    vx.status = kVertexMiss;
                    cnt[6]++;
                } else {
                    vx.t = h.t;
                    vx.u = h.u;
                    vx.v = h.v;
                    vx.backface = h.backface ? 1u : 0u;
                    const Surface sf = surfaceOf(sc, h.tri, h.u, h.v, h.backface);
                    vx.glass = sf.glass;
                    cnt[0] += sf.glass;
                    const V3 X = origin + h.t * direction;
                    uint32_t bits = litLights(sc, sf.N);
                    for (uint32_t l = 0; l < lightCount; ++l) {
                        if (!((bits >> l) & 1u)) continue;
                        V3 dir;
                        float tmax;
                        shadowRay(sc, d.z_far, l, X, &dir, &tmax);
                        const bool occ = occluded(sc, nRecords, X, dir, tmax);
                        if (occ) bits |= 1u << (16u + l);
                        cnt[occ ? 4 : 5]++;
                    }
                    vx.shadowBits = bits;
                    s.radiance = s.radiance + s.attenuation * directRadiance(sc, sf, direction, X, bits);
                    const Scatter sct = scatter(sf, direction, s.rng, s.attenuation);
                    s.rng = sct.rng;
                    s.attenuation = sct.attenuation;
                    const V3 scattered = sct.direction;
                    if (!sct.alive) {
                        s.radiance = missRadiance(sc, direction, d.environment_multiplier, s.attenuation, s.radiance);
                        vx.status = kVertexKilled;
                        cnt[2]++;
                    } else if (goesOn(seg, s.attenuation)) {
                        vx.status = kVertexScattered;
                        origin = X;
                        direction = scattered;
                        tmin = kNextTmin;
                        ends = false;
                    } else {
                        vx.status = kVertexLast;
                    }
                    put3(vx.scattered, scattered);
                }
                put3(vx.attenuationAfter, s.attenuation);
                put3(vx.radianceAfter, s.radiance);
                vx.rngAfter = s.rng;
                if (ends) break;
            }
            uint16_t* texel = d.image + 4 * p;
            texel[0] = refl::f2h(s.radiance.x);
            texel[1] = refl::f2h(s.radiance.y);
            texel[2] = refl::f2h(s.radiance.z);
            texel[3] = 0;
        }
    if (d.flags) hostAccumulate(d); // k_pt_accumulate
    if (counts) std::memcpy(counts, cnt, sizeof(cnt));
    return 0;
}

} // namespace pt
} // namespace ark

// ark_ddgi_debug.h: the host-only entries of the restatement, no GPU
extern "C" int ark_ddgi_debug_path_tracer_check_desc(const ArkPathTracerDesc* desc)
{
    if (!desc || desc->struct_size != sizeof(ArkPathTracerDesc)) return ARK_DDGI_E_INVALID_ARGUMENT;
    return ark::pt::descProblem(*desc) ? ARK_DDGI_E_INVALID_ARGUMENT : ARK_DDGI_OK;
}

extern "C" int ark_ddgi_debug_path_tracer_host(const ArkDdgiScene* scene, const ArkPathTracerDesc* desc, void* vertices, uint64_t* counts)
{
    if (!scene || scene->struct_size != sizeof(ArkDdgiScene) || ark_ddgi_debug_path_tracer_check_desc(desc) != ARK_DDGI_OK) return ARK_DDGI_E_INVALID_ARGUMENT;
    ark::pt::HostScene hs;
    if (ark::pt::hostSceneFrom(*scene, hs) != 0) return ARK_DDGI_E_INVALID_ARGUMENT;
    return ark::pt::hostPathTrace(hs.view(), hs.tris.size(), *desc, static_cast<ark::pt::Vertex*>(vertices), counts) == 0 ? ARK_DDGI_OK : ARK_DDGI_E_INVALID_ARGUMENT;
}

extern "C" int ark_ddgi_debug_path_tracer_layout(uint32_t* out, int n)
{
    const uint32_t offsets[] = { offsetof(ArkPathTracerDesc, width), offsetof(ArkPathTracerDesc, height), offsetof(ArkPathTracerDesc, flags),
                                 offsetof(ArkPathTracerDesc, frame_index), offsetof(ArkPathTracerDesc, accumulated_frames), offsetof(ArkPathTracerDesc, max_paths_per_batch),
                                 offsetof(ArkPathTracerDesc, environment_multiplier), offsetof(ArkPathTracerDesc, z_near), offsetof(ArkPathTracerDesc, z_far),
                                 offsetof(ArkPathTracerDesc, world_from_view), offsetof(ArkPathTracerDesc, view_from_projection), offsetof(ArkPathTracerDesc, image),
                                 offsetof(ArkPathTracerDesc, accumulation), offsetof(ArkPathTracerDesc, reserved), sizeof(ArkPathTracerDesc),
                                 static_cast<uint32_t>(sizeof(ark::pt::Vertex)) };
    const int m = static_cast<int>(sizeof(offsets) / sizeof(offsets[0]));
    if (!out) return 0;
    for (int i = 0; i < n && i < m; ++i) out[i] = offsets[i];
    return m < n ? m : n;
}

extern "C" int ark_ddgi_debug_path_tracer_accumulate_host(const ArkPathTracerDesc* desc)
{
    if (ark_ddgi_debug_path_tracer_check_desc(desc) != ARK_DDGI_OK || !desc->flags) return ARK_DDGI_E_INVALID_ARGUMENT;
    ark::pt::hostAccumulate(*desc);
    return ARK_DDGI_OK;
}

// pt_randomFloat alone: out_value the float it returns for `state`, out_next the state after
extern "C" int ark_ddgi_debug_path_tracer_random(uint32_t state, float* out_value, uint32_t* out_next)
{
    if (!out_value || !out_next) return ARK_DDGI_E_INVALID_ARGUMENT;
    *out_value = ark::pt::randomFloat(state);
    *out_next = state;
    return ARK_DDGI_OK;
}

extern "C" int ark_ddgi_debug_path_tracer_sample(uint32_t px, uint32_t py, uint32_t width, uint32_t height, uint32_t frame_index, const float* world_from_view,
                                                 const float* view_from_projection, uint32_t* out_state, float* out_ray)
{
    if (!world_from_view || !view_from_projection || !out_state || !out_ray) return ARK_DDGI_E_INVALID_ARGUMENT;
    ark::pt::V3 o, d;
    out_state[0] = ark::pt::pixelSeed(px, py, width, height, frame_index);
    const ark::pt::PathState s = ark::pt::cameraRay(px, py, width, height, frame_index, world_from_view, view_from_projection, &o, &d);
    out_state[1] = s.rng;
    out_ray[0] = o.x;
    out_ray[1] = o.y;
    out_ray[2] = o.z;
    out_ray[3] = d.x;
    out_ray[4] = d.y;
    out_ray[5] = d.z;
    return ARK_DDGI_OK;
}
