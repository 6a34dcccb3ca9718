// refl_denoise_host.cpp — see refl_denoise_host.h; at the end the host-only
// ark_ddgi_debug_refl_denoise_* entries (include/ark_ddgi_debug.h), which need nothing else
// of the library.
#include "refl_denoise_host.h"

#include <cmath>
#include <cstddef>
#include <cstring>

#include "../../include/ark_ddgi_debug.h"

namespace ark {
namespace refl {

const char* descProblem(const ArkReflDenoiseDesc& d)
{
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(d.world_from_view[k]) || !std::isfinite(d.view_from_projection[k]) || !std::isfinite(d.previous_frame_view_from_world[k]) ||
            !std::isfinite(d.previous_frame_projection_from_view[k]))
            return "non-finite camera matrix";
    if (!std::isfinite(d.no_tracing_roughness) || !std::isfinite(d.temporal_stability) || !std::isfinite(d.z_near) || !std::isfinite(d.z_far)) return "non-finite scalar";
    if (d.z_near == d.z_far) return "z_near == z_far";
    if (d.flags & ~(ARK_REFL_DENOISE_FIRST_FRAME | ARK_REFL_DENOISE_DISABLED)) return "unknown flag";
    const uint64_t pixels = static_cast<uint64_t>(d.width) * d.height;
    if (pixels >= (1ull << 28)) return "target too large";
    if (pixels == 0) return nullptr;
    const uint64_t tiles = static_cast<uint64_t>((d.width + 7u) / 8u) * ((d.height + 7u) / 8u);
    struct Plane {
        const void* p;
        uint64_t bytes, align;
    };
    const Plane planes[13] = { { d.radiance, pixels * 8, 8 },         { d.depth, pixels * 4, 4 },           { d.material, pixels * 4, 4 },
                               { d.normal_velocity, pixels * 8, 8 },  { d.radiance_history, pixels * 8, 8 }, { d.normal_history, pixels * 8, 8 },
                               { d.depth_history, pixels * 8, 8 },    { d.reprojected, pixels * 8, 8 },      { d.average_radiance, tiles * 8, 8 },
                               { d.variance, pixels * 4, 4 },         { d.num_samples, pixels * 4, 4 },      { d.resolved, pixels * 8, 8 },
                               { d.temporal_accumulation, pixels * 8, 8 } };
    for (const Plane& q : planes) {
        if (!q.p) return "null plane";
        if (reinterpret_cast<uintptr_t>(q.p) % q.align) return "misaligned plane";
    }
    for (int i = 0; i < 13; ++i)
        for (int j = 0; j < i; ++j) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(planes[i].p), b = reinterpret_cast<uintptr_t>(planes[j].p);
            if (a < b + planes[j].bytes && b < a + planes[i].bytes) return "two planes alias";
        }
    return nullptr;
}

Args argsOf(const ArkReflDenoiseDesc& d)
{
    Args a {};
    a.width = d.width;
    a.height = d.height;
    a.noTracingRoughness = d.no_tracing_roughness;
    a.temporalStability = d.temporal_stability;
    std::memcpy(a.worldFromView, d.world_from_view, 64);
    std::memcpy(a.viewFromProjection, d.view_from_projection, 64);
    std::memcpy(a.prevViewFromWorld, d.previous_frame_view_from_world, 64);
    std::memcpy(a.prevProjectionFromView, d.previous_frame_projection_from_view, 64);
    a.zNear = d.z_near;
    a.zFar = d.z_far;
    a.radiance = d.radiance;
    a.depth = d.depth;
    a.material = d.material;
    a.normalVelocity = d.normal_velocity;
    a.radianceHistory = d.radiance_history;
    a.normalHistory = d.normal_history;
    a.depthHistory = d.depth_history;
    a.reprojected = d.reprojected;
    a.averageRadiance = d.average_radiance;
    a.variance = d.variance;
    a.numSamples = d.num_samples;
    a.resolved = d.resolved;
    a.temporalAccumulation = d.temporal_accumulation;
    return a;
}

namespace {

// every 8 x 8 group of the image; lanes in the order (gx, gy) = (lane & 7, lane >> 3)
template<class F>
void forTiles(const Args& a, F&& tile)
{
    const uint32_t tilesX = (a.width + 7u) / 8u, tilesY = (a.height + 7u) / 8u;
    for (uint32_t ty = 0; ty < tilesY; ++ty)
        for (uint32_t tx = 0; tx < tilesX; ++tx) tile(tx, ty);
}

} // namespace

void hostHistoryCopy(const Args& a, bool firstCopy)
{
    for (uint32_t y = 0; y < a.height; ++y)
        for (uint32_t x = 0; x < a.width; ++x) historyCopyPixel(a, static_cast<int>(x), static_cast<int>(y), firstCopy);
}

void hostReproject(const Args& a)
{
    uint32_t s0[kTileWords], s1[kTileWords];
    forTiles(a, [&](uint32_t tx, uint32_t ty) {
        const int bx = static_cast<int>(tx * 8u), by = static_cast<int>(ty * 8u);
        for (int l = 0; l < 64; ++l) fillRadianceTile(a, s0, s1, bx + (l & 7), by + (l >> 3), l & 7, l >> 3);
        F4 part[64];
        for (int l = 0; l < 64; ++l) part[l] = reprojectPixel(a, s0, s1, bx + (l & 7), by + (l >> 3), (l & 7) + 4, (l >> 3) + 4);
        for (int l = 0; l < 64; ++l) tileStore4(s0, s1, l & 7, l >> 3, part[l]);
        for (int i = 2; i <= 8; i *= 2)
            for (int l = 0; l < 64; ++l) reduceStep(s0, s1, l & 7, l >> 3, i);
        storeAverage(a, s0, s1, tx, ty);
    });
}

void hostPrefilter(const Args& a)
{
    uint32_t s0[kTileWords], s1[kTileWords], s2[kTileWords], s3[kTileWords];
    float sd[kTileWords];
    forTiles(a, [&](uint32_t tx, uint32_t ty) {
        const int bx = static_cast<int>(tx * 8u), by = static_cast<int>(ty * 8u);
        for (int l = 0; l < 64; ++l) fillPrefilterTile(a, s0, s1, s2, s3, sd, bx + (l & 7), by + (l >> 3), l & 7, l >> 3);
        for (int l = 0; l < 64; ++l) {
            const int px = bx + (l & 7), py = by + (l >> 3);
            if (inside(px, py, a.width, a.height)) prefilterPixel(a, s0, s1, s2, s3, sd, px, py, (l & 7) + 4, (l >> 3) + 4);
        }
    });
}

void hostResolveTemporal(const Args& a)
{
    uint32_t s0[kTileWords], s1[kTileWords];
    forTiles(a, [&](uint32_t tx, uint32_t ty) {
        const int bx = static_cast<int>(tx * 8u), by = static_cast<int>(ty * 8u);
        for (int l = 0; l < 64; ++l) fillRadianceTile(a, s0, s1, bx + (l & 7), by + (l >> 3), l & 7, l >> 3);
        for (int l = 0; l < 64; ++l) {
            const int px = bx + (l & 7), py = by + (l >> 3);
            if (inside(px, py, a.width, a.height)) resolveTemporalPixel(a, s0, s1, px, py, (l & 7) + 4, (l >> 3) + 4);
        }
    });
}

int hostDenoise(const ArkReflDenoiseDesc& d)
{
    if (descProblem(d)) return -1;
    const uint64_t pixels = static_cast<uint64_t>(d.width) * d.height;
    if (pixels == 0) return 0;
    if (d.flags & ARK_REFL_DENOISE_DISABLED) { // RTReflectionsNode.cpp:134-138
        std::memcpy(d.resolved, d.radiance, pixels * 8);
        return 0;
    }
    const Args a = argsOf(d);
    if (d.flags & ARK_REFL_DENOISE_FIRST_FRAME) hostHistoryCopy(a, true);
    hostReproject(a);
    hostPrefilter(a);
    hostResolveTemporal(a);
    hostHistoryCopy(a, false);
    return 0;
}

} // namespace refl
} // namespace ark

// ark_ddgi_debug.h: the host-only entries of the restatement, no GPU
extern "C" int ark_ddgi_debug_refl_denoise_check_desc(const ArkReflDenoiseDesc* desc)
{
    if (!desc || desc->struct_size != sizeof(ArkReflDenoiseDesc)) return ARK_DDGI_E_INVALID_ARGUMENT;
    return ark::refl::descProblem(*desc) ? ARK_DDGI_E_INVALID_ARGUMENT : ARK_DDGI_OK;
}

extern "C" int ark_ddgi_debug_refl_denoise_host(const ArkReflDenoiseDesc* desc)
{
    if (ark_ddgi_debug_refl_denoise_check_desc(desc) != ARK_DDGI_OK) return ARK_DDGI_E_INVALID_ARGUMENT;
    return ark::refl::hostDenoise(*desc) == 0 ? ARK_DDGI_OK : ARK_DDGI_E_INVALID_ARGUMENT;
}

extern "C" int ark_ddgi_debug_refl_denoise_layout(uint32_t* out, int n)
{
    typedef ArkReflDenoiseDesc D;
    const uint32_t offsets[] = { offsetof(D, width),          offsetof(D, height),        offsetof(D, flags),
                                 offsetof(D, no_tracing_roughness), offsetof(D, temporal_stability), offsetof(D, world_from_view),
                                 offsetof(D, view_from_projection), offsetof(D, previous_frame_view_from_world), offsetof(D, previous_frame_projection_from_view),
                                 offsetof(D, z_near),         offsetof(D, z_far),         offsetof(D, radiance),
                                 offsetof(D, depth),          offsetof(D, material),      offsetof(D, normal_velocity),
                                 offsetof(D, radiance_history), offsetof(D, normal_history), offsetof(D, depth_history),
                                 offsetof(D, reprojected),    offsetof(D, average_radiance), offsetof(D, variance),
                                 offsetof(D, num_samples),    offsetof(D, resolved),      offsetof(D, temporal_accumulation),
                                 static_cast<uint32_t>(sizeof(D)) };
    const int m = static_cast<int>(sizeof(offsets) / sizeof(offsets[0]));
    if (!out) return 0;
    for (int i = 0; i < n && i < m; ++i) out[i] = offsets[i];
    return m < n ? m : n;
}

extern "C" int ark_ddgi_debug_refl_denoise_kat(int which, const float* in, int n_in, float* out, int n_out)
{
    using namespace ark::refl;
    if (!in || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    auto need = [&](int i, int o) { return n_in == i && n_out == o; };
    switch (which) {
    case ARK_REFL_KAT_ROUND_UP8:
        if (!need(1, 1)) break;
        out[0] = static_cast<float>(roundUp8(static_cast<uint32_t>(in[0])));
        return ARK_DDGI_OK;
    case ARK_REFL_KAT_CLIP_AABB: {
        if (!need(9, 3)) break;
        const F3 r = clipAABB(f3(in[0], in[1], in[2]), f3(in[3], in[4], in[5]), f3(in[6], in[7], in[8]));
        out[0] = r.x, out[1] = r.y, out[2] = r.z;
        return ARK_DDGI_OK;
    }
    case ARK_REFL_KAT_KERNEL_WEIGHT:
        if (!need(1, 1)) break;
        out[0] = kernelWeight(in[0]);
        return ARK_DDGI_OK;
    case ARK_REFL_KAT_TILE_REDUCTION: { // in: 64 lanes x 4, lane = gy * 8 + gx
        if (!need(256, 4)) break;
        uint32_t s0[kTileWords] = {}, s1[kTileWords] = {};
        for (int l = 0; l < 64; ++l) tileStore4(s0, s1, l & 7, l >> 3, { in[4 * l], in[4 * l + 1], in[4 * l + 2], in[4 * l + 3] });
        for (int i = 2; i <= 8; i *= 2)
            for (int l = 0; l < 64; ++l) reduceStep(s0, s1, l & 7, l >> 3, i);
        const F4 s = tileRaw(s0, s1, 0, 0);
        out[0] = s.x, out[1] = s.y, out[2] = s.z, out[3] = s.w;
        return ARK_DDGI_OK;
    }
    case ARK_REFL_KAT_EXP:
        if (n_in != n_out) break;
        for (int i = 0; i < n_in; ++i) out[i] = expf_(in[i]);
        return ARK_DDGI_OK;
    case ARK_REFL_KAT_POW512:
        if (n_in != n_out) break;
        for (int i = 0; i < n_in; ++i) out[i] = ark::powf_(in[i], kPrefilterNormalSigma);
        return ARK_DDGI_OK;
    case ARK_REFL_KAT_HALF:
        if (n_in != n_out) break;
        for (int i = 0; i < n_in; ++i) out[i] = h2f(f2h(in[i]));
        return ARK_DDGI_OK;
    default: break;
    }
    return ARK_DDGI_E_INVALID_ARGUMENT;
}
