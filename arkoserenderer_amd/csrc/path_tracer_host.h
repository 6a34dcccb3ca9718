// path_tracer_host.h — the host side of the path tracer (ark_ddgi_path_trace): the entry's
// argument checks and a serial restatement of the frame that walks every path through
// path_tracer.h, the functions the kernels call, in the kernels' order. Hits are found by
// brute force over the triangle records with the kernels' intersectTri (shading_math.h) and tie rule
// (equal t: the smaller (instance, primitive)), so they do not depend on a BVH. Host only,
// no HIP (also built on its own, tests/cpp).
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/ark_ddgi.h"
#include "path_tracer.h"

namespace ark {
namespace pt {

struct F4 {
    float x, y, z, w;
};
using HostView = SceneView<F4>;

// A scene held on the host in the device's layouts (a context's buffers downloaded, or made
// by a caller), and its view.
struct HostScene {
    std::vector<GpuTriangle> tris; // the world BVHs' records, holes included
    std::vector<uint32_t> indices;
    std::vector<float> vertices;
    std::vector<ArkRTTriangleMesh> meshes;
    std::vector<ArkShaderMaterial> materials;
    std::vector<GpuInstance> instances;
    std::vector<GpuTextureInfo> texInfos;
    std::vector<F4> texels;
    std::vector<GpuSpotLight> spots;
    int32_t textureCount = 0, whiteTexture = 0, envTexture = 0, hasSun = 0;
    float sunColor[3] { 0, 0, 0 }, sunDir[3] { 0, 0, 0 };
    HostView view() const;
};

// ark_ddgi_set_scene's host preprocessing of `s` without a device: the records in (instance,
// primitive) order, the instance table, the decoded texels, the scene's lights. Returns 0, or
// -1 for a scene ark_ddgi_set_scene refuses.
int hostSceneFrom(const ArkDdgiScene& s, HostScene& out);

// What ark_ddgi_path_trace refuses about a descriptor of the right struct_size (null:
// nothing): an unknown flag, both flags, a flag without `accumulation`, a non-finite matrix or
// scalar, width * height >= 2^28 and, unless the image is empty, a null image, a plane not
// aligned to its texel (8 bytes RGBA16F, 16 bytes RGBA32F) and planes whose byte ranges
// overlap. The pointers are compared, never followed.
const char* descProblem(const ArkPathTracerDesc& d);

// One segment of one path as the restatement walked it (33 words; ark_ddgi_debug.h).
struct Vertex {
    uint32_t status;     // kVertex*; 0: the path had ended before this segment
    uint32_t rngBefore;
    float origin[3], direction[3], tmin;
    uint32_t tri;        // record index, 0xffffffff: no hit
    float t, u, v;
    uint32_t backface;
    uint32_t shadowBits; // bit l: light l cast a ray; bit 16 + l: it was occluded
    float attenuationBefore[3], radianceBefore[3], attenuationAfter[3], radianceAfter[3];
    float scattered[3];
    uint32_t rngAfter;
    uint32_t alphaRejected; // candidates the alpha test refused while this segment's hit was searched
    uint32_t glass;         // the hit ran the glass program
};
static_assert(sizeof(Vertex) == 33 * 4, "33 words");
enum : uint32_t { kVertexNone = 0, kVertexScattered = 1, kVertexMiss = 2, kVertexKilled = 3, kVertexLast = 4 };
// counts[8]: glass vertices, alpha-rejected candidates, killed paths, paths with a segment 8,
// occluded shadow rays, lit shadow rays, missed segments, vertices
constexpr int kCounts = 8;

// The accumulate step or the reset copy of `d` (a flag is set) over host planes.
void hostAccumulate(const ArkPathTracerDesc& d);

// The frame of `d` (image and accumulation are host pointers here) over the scene. vertices:
// null, or width * height * 16 records (pixel-major). Returns 0, or -1 for what descProblem
// refuses.
int hostPathTrace(const HostView& sc, uint64_t nRecords, const ArkPathTracerDesc& d, Vertex* vertices, uint64_t* counts);

} // namespace pt
} // namespace ark
