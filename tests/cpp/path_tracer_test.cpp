// path_tracer_test.cpp — csrc/path_tracer_host.cpp on its own (tests/test_path_tracer_sanitizers.py
// builds both with -fsanitize=address,undefined): the host restatement of the path tracer
// over a small scene (a floor, a wall, a checker-alpha masked quad, a glass pane, a sun, a
// spot) at 1 x 1 and 1 x 97, with hole records among the triangle records, a spot light
// placed exactly on a shading point (the NaN length: not traced, lit), zero lights, the
// accumulate step and the reset copy, and the refusals. Every texel is written, inside its
// plane only.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_tracer_host.h"

using namespace ark;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
            ++failures;                                      \
        }                                                    \
    } while (0)

struct World {
    std::vector<float> positions;
    std::vector<ArkRTVertex> vertices;
    std::vector<uint32_t> indices;
    std::vector<ArkRTTriangleMesh> meshes;
    std::vector<ArkShaderMaterial> materials;
    std::vector<ArkRTInstance> instances;
    std::vector<uint8_t> checker;
    ArkTexture textures[1];
    ArkSpotLight spot;
    ArkDdgiScene scene;

    void quad(const float c[3], const float a[3], const float b[3], const float n[3], int material, uint32_t mask)
    {
        const int32_t fv = static_cast<int32_t>(vertices.size()), fi = static_cast<int32_t>(indices.size());
        const float s[4][2] = { { -1, -1 }, { 1, -1 }, { 1, 1 }, { -1, 1 } };
        const float len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        for (int k = 0; k < 4; ++k) {
            ArkRTVertex v {};
            for (int i = 0; i < 3; ++i) {
                positions.push_back(c[i] + s[k][0] * a[i] + s[k][1] * b[i]);
                v.normal[i] = n[i];
                v.tangent[i] = a[i] / len;
            }
            v.tangent[3] = 1.0f;
            v.tex_coord[0] = 0.5f * (s[k][0] + 1.0f);
            v.tex_coord[1] = 0.5f * (s[k][1] + 1.0f);
            vertices.push_back(v);
        }
        for (uint32_t i : { 0u, 1u, 2u, 0u, 2u, 3u }) indices.push_back(i);
        meshes.push_back({ fv, fi, material });
        ArkRTInstance inst {};
        inst.object_to_world[0] = inst.object_to_world[5] = inst.object_to_world[10] = 1.0f;
        inst.rt_mesh_index = static_cast<uint32_t>(meshes.size() - 1);
        inst.triangle_count = 2;
        inst.hit_mask = mask;
        instances.push_back(inst);
    }

    World()
    {
        auto material = [](int baseColor, int blend, float metallic, float alphaTint) {
            ArkShaderMaterial m {};
            m.base_color = baseColor;
            m.normal_map = m.metallic_roughness = m.emissive = m.occlusion = m.bent_normal_map = -1;
            m.blend_mode = blend;
            m.mask_cutoff = 0.5f;
            m.metallic_factor = metallic;
            m.roughness_factor = 0.5f;
            m.color_tint[0] = m.color_tint[1] = m.color_tint[2] = 0.8f;
            m.color_tint[3] = alphaTint;
            return m;
        };
        materials = { material(-1, ARK_BLEND_MODE_OPAQUE, 0.0f, 1.0f), material(0, ARK_BLEND_MODE_MASKED, 0.0f, 1.0f), material(0, ARK_BLEND_MODE_TRANSLUCENT, 0.0f, 0.5f),
                      material(-1, ARK_BLEND_MODE_OPAQUE, 1.0f, 1.0f) };
        const float up[3] = { 0, 1, 0 }, front[3] = { 0, 0, 1 };
        const float c0[3] = { 0, 0, 0 }, a0[3] = { 6, 0, 0 }, b0[3] = { 0, 0, -6 };
        quad(c0, a0, b0, up, 0, ARK_RT_HIT_MASK_OPAQUE);
        const float c1[3] = { 0, 1.5f, -3 }, a1[3] = { 3, 0, 0 }, b1[3] = { 0, 1.5f, 0 };
        quad(c1, a1, b1, front, 3, ARK_RT_HIT_MASK_OPAQUE);
        const float c2[3] = { -0.5f, 1, -1 }, a2[3] = { 0.6f, 0, 0 }, b2[3] = { 0, 0.6f, 0 };
        quad(c2, a2, b2, front, 1, ARK_RT_HIT_MASK_MASKED);
        const float c3[3] = { 0.6f, 1, -0.5f };
        quad(c3, a2, b2, front, 2, ARK_RT_HIT_MASK_BLEND);
        checker.resize(8 * 8 * 4);
        for (int y = 0; y < 8; ++y)
            for (int x = 0; x < 8; ++x) {
                uint8_t* t = &checker[(y * 8 + x) * 4];
                t[0] = 200, t[1] = 180, t[2] = 90;
                t[3] = ((x / 2 + y / 2) & 1) ? 255 : 30;
            }
        textures[0] = { 8, 8, ARK_TEX_RGBA8_SRGB, ARK_WRAP_REPEAT, checker.data() };
        std::memset(&spot, 0, sizeof(spot));
        const float col[3] = { 20, 18, 15 }, dir[3] = { 0, -1, 0 }, right[3] = { 1, 0, 0 }, upv[3] = { 0, 0, 1 }, pos[3] = { 0.2f, 2.5f, -1 };
        for (int k = 0; k < 3; ++k) {
            spot.color[k] = col[k];
            spot.world_space_direction[k] = dir[k];
            spot.world_space_right[k] = right[k];
            spot.world_space_up[k] = upv[k];
            spot.world_space_position[k] = pos[k];
        }
        spot.outer_cone_half_angle = 0.9f;
        spot.ies_profile_index = -1;
        std::memset(&scene, 0, sizeof(scene));
        scene.struct_size = sizeof(scene);
        scene.indices = indices.data();
        scene.index_count = indices.size();
        scene.positions = positions.data();
        scene.vertex_count = vertices.size();
        scene.vertices = vertices.data();
        scene.meshes = meshes.data();
        scene.mesh_count = static_cast<uint32_t>(meshes.size());
        scene.materials = materials.data();
        scene.material_count = static_cast<uint32_t>(materials.size());
        scene.textures = textures;
        scene.texture_count = 1;
        scene.instances = instances.data();
        scene.instance_count = static_cast<uint32_t>(instances.size());
        scene.has_directional_light = 1;
        const float sunCol[3] = { 2, 2, 1.8f }, sunDir[3] = { 0.3f, -0.9f, -0.3f };
        for (int k = 0; k < 3; ++k) {
            scene.directional_light.color[k] = sunCol[k];
            scene.directional_light.world_space_direction[k] = sunDir[k];
        }
        scene.spot_lights = &spot;
        scene.spot_light_count = 1;
        scene.environment_texture = -1;
    }
};

// a camera at (0, 1.2, 2.5) looking down -z: worldFromView a translation, a 90-degree projection inverted by hand
static void camera(ArkPathTracerDesc& d, uint32_t w, uint32_t h)
{
    std::memset(&d, 0, sizeof(d));
    d.struct_size = sizeof(d);
    d.width = w;
    d.height = h;
    d.environment_multiplier = 0.5f;
    d.z_near = 0.1f;
    d.z_far = 50.0f;
    const float wv[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 1.2f, 2.5f, 1 };
    // viewFromProjection * (x, y, 1, 1) = (x, y, -1, 1): a 90-degree view down -z
    const float pv[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, -1, 1 };
    std::memcpy(d.world_from_view, wv, sizeof(wv));
    std::memcpy(d.view_from_projection, pv, sizeof(pv));
}

struct Planes {
    std::vector<uint16_t> image;
    std::vector<float> acc;
    std::vector<pt::Vertex> vtx;
    void attach(ArkPathTracerDesc& d, bool withAcc)
    {
        const size_t px = static_cast<size_t>(d.width) * d.height;
        image.assign(px * 4 + 8, 0x5a5a); // 4 guard words on each side
        acc.assign(px * 4 + 8, -7.0f);
        vtx.assign(px * pt::kMaxSegments, pt::Vertex {});
        d.image = image.data() + 4;
        d.accumulation = withAcc ? acc.data() + 4 : nullptr;
    }
    void check(const ArkPathTracerDesc& d, const char* what)
    {
        const size_t px = static_cast<size_t>(d.width) * d.height;
        for (int g = 0; g < 4; ++g) CHECK(image[g] == 0x5a5a && image[4 + px * 4 + g] == 0x5a5a, "%s: image guard", what);
        for (int g = 0; g < 4; ++g) CHECK(acc[g] == -7.0f && acc[4 + px * 4 + g] == -7.0f, "%s: accumulation guard", what);
        for (size_t p = 0; p < px; ++p) CHECK(image[4 + p * 4 + 3] == 0, "%s: alpha of texel %zu", what, p);
        for (size_t p = 0; p < px; ++p) CHECK(vtx[p * pt::kMaxSegments].status != pt::kVertexNone, "%s: pixel %zu has no first segment", what, p);
    }
};

int main()
{
    World world;
    pt::HostScene hs;
    CHECK(pt::hostSceneFrom(world.scene, hs) == 0, "hostSceneFrom");
    CHECK(hs.tris.size() == 8 && hs.texels.size() == 65, "records %zu texels %zu", hs.tris.size(), hs.texels.size());
    // hole records between the live ones (a BVH8's leaf rows have them)
    {
        std::vector<GpuTriangle> withHoles;
        for (const GpuTriangle& t : hs.tris) {
            GpuTriangle hole {};
            hole.t2[1] = u2f(kHoleInstance);
            withHoles.push_back(hole);
            withHoles.push_back(t);
        }
        withHoles.push_back(GpuTriangle {}); // the zero padding record: instance 0, degenerate
        hs.tris = withHoles;
    }
    uint64_t counts[pt::kCounts];
    const uint32_t sizes[3][2] = { { 1, 1 }, { 1, 97 }, { 13, 9 } };
    uint64_t glass = 0, rejected = 0, killed = 0, shadows = 0;
    for (const auto& wh : sizes)
        for (uint32_t frame : { 0u, 3u }) {
            ArkPathTracerDesc d;
            camera(d, wh[0], wh[1]);
            d.frame_index = frame;
            d.flags = frame ? ARK_PATH_TRACER_ACCUMULATE : ARK_PATH_TRACER_RESET;
            d.accumulated_frames = frame;
            Planes pl;
            pl.attach(d, true);
            CHECK(pt::hostPathTrace(hs.view(), hs.tris.size(), d, pl.vtx.data(), counts) == 0, "%ux%u", wh[0], wh[1]);
            pl.check(d, "frame");
            for (size_t p = 0; p < static_cast<size_t>(wh[0]) * wh[1]; ++p) CHECK(pl.acc[4 + p * 4 + 3] == (frame ? 1.0f : 0.0f), "accumulation alpha");
            for (const pt::Vertex& v : pl.vtx) CHECK(v.status == pt::kVertexNone || v.tri == 0xffffffffu || (v.tri < hs.tris.size() && f2u(hs.tris[v.tri].t2[1]) != kHoleInstance), "a hole was hit");
            glass += counts[0], rejected += counts[1], killed += counts[2], shadows += counts[4] + counts[5];
        }
    CHECK(glass > 0 && rejected > 0 && killed > 0 && shadows > 0, "ground: glass %llu rejected %llu killed %llu shadow rays %llu", (unsigned long long)glass,
          (unsigned long long)rejected, (unsigned long long)killed, (unsigned long long)shadows);
    // the spot exactly on the first shading point of a 1 x 1 frame: a zero-length toLight
    {
        ArkPathTracerDesc d;
        camera(d, 1, 1);
        d.world_from_view[13] = 2.0f; // higher up: the pixel's ray meets the floor
        d.view_from_projection[12] = -1.0f; // (the jittered sample lies in [0, 2] of NDC: centre it)
        d.view_from_projection[13] = -2.5f; // and looks down
        Planes pl;
        pl.attach(d, false);
        CHECK(pt::hostPathTrace(hs.view(), hs.tris.size(), d, pl.vtx.data(), counts) == 0, "1x1");
        const pt::Vertex v = pl.vtx[0];
        CHECK(v.status != pt::kVertexMiss && v.status != pt::kVertexNone, "the 1x1 ray misses (status %u)", v.status);
        pt::HostScene moved = hs;
        for (int k = 0; k < 3; ++k) moved.spots[0].position[k] = v.origin[k] + v.t * v.direction[k];
        pl.attach(d, false);
        CHECK(pt::hostPathTrace(moved.view(), moved.tris.size(), d, pl.vtx.data(), counts) == 0, "spot at the shading point");
        pl.check(d, "spot at the shading point");
        CHECK(((pl.vtx[0].shadowBits) & 2u) != 0 && !((pl.vtx[0].shadowBits >> 17) & 1u), "the NaN-length ray must be cast and lit (bits %#x)",
              pl.vtx[0].shadowBits);
    }
    // zero lights
    {
        pt::HostScene dark = hs;
        dark.hasSun = 0;
        dark.spots.clear();
        ArkPathTracerDesc d;
        camera(d, 5, 7);
        Planes pl;
        pl.attach(d, false);
        CHECK(pt::hostPathTrace(dark.view(), dark.tris.size(), d, pl.vtx.data(), counts) == 0, "zero lights");
        pl.check(d, "zero lights");
        CHECK(counts[4] + counts[5] == 0, "shadow rays without lights");
    }
    // the refusals: nothing is written
    {
        ArkPathTracerDesc d;
        camera(d, 4, 4);
        Planes pl;
        pl.attach(d, true);
        auto refused = [&](ArkPathTracerDesc bad, const char* what) {
            CHECK(pt::descProblem(bad) != nullptr, "%s accepted", what);
            CHECK(pt::hostPathTrace(hs.view(), hs.tris.size(), bad, nullptr, nullptr) == -1, "%s ran", what);
        };
        ArkPathTracerDesc b = d;
        b.flags = 8;
        refused(b, "unknown flag");
        b = d;
        b.flags = 3;
        refused(b, "both flags");
        b = d;
        b.flags = 1;
        b.accumulation = nullptr;
        refused(b, "flag without accumulation");
        b = d;
        b.image = nullptr;
        refused(b, "null image");
        b = d;
        b.image = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(d.image) + 2);
        refused(b, "misaligned image");
        b = d;
        b.flags = 2;
        b.accumulation = reinterpret_cast<float*>(reinterpret_cast<char*>(d.accumulation) + 4);
        refused(b, "misaligned accumulation");
        b = d;
        b.flags = 1;
        b.accumulation = reinterpret_cast<float*>(d.image);
        refused(b, "overlap");
        b = d;
        b.z_far = INFINITY;
        refused(b, "infinite z_far");
        b = d;
        b.view_from_projection[3] = NAN;
        refused(b, "NaN matrix");
        b = d;
        b.width = b.height = 1u << 14;
        refused(b, "2^28 pixels");
        for (uint16_t w : pl.image) CHECK(w == 0x5a5a, "a refused call wrote the image");
        for (float w : pl.acc) CHECK(w == -7.0f, "a refused call wrote the accumulation");
        ArkPathTracerDesc empty = d;
        empty.width = 0;
        empty.image = nullptr;
        CHECK(pt::descProblem(empty) == nullptr && pt::hostPathTrace(hs.view(), hs.tris.size(), empty, nullptr, counts) == 0 && counts[7] == 0, "an empty image");
    }
    std::printf(failures ? "%d FAILURES\n" : "OK\n", failures);
    return failures ? 1 : 0;
}
