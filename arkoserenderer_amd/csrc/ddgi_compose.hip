// ddgi_compose.hip — the DDGI consumers that only read the atlases (ddgi_sampling.h):
// lighting compose and the probe debug visualisation.
//
// Lighting compose (lightingCompose.comp:22-135, WITH_DDGI = 1, driven by
// LightingComposeNode.cpp:60-110).
//
// One thread per pixel, 64 x 4 tiles: a wave reads one row of 64 pixels, so a 4-B plane
// is two whole 128-B lines per wave and an 8-B plane four (16 x 16 tiles read half lines
// of the 4-B planes: 230.6 -> 211.3 MB of counter fetch per 1080p launch, the time
// unchanged at 0.204 ms, profiles/r06_c_compose; 32 x 8: 213.6 MB). The G-buffer planes
// are read once (52 B in, 8 B out per pixel with every flag on); the 8-probe atlas
// gather mostly hits L2 (neighbouring pixels share probes): the ~79 MB of counter fetch
// beyond the plane bytes is atlas texels missing the XCDs' L2s. Matrix products are summed column by column,
// left to right, without contraction (the same order as the oracle); GLSL leaves
// that order to the driver.

#include <hip/hip_runtime.h>

#include "../../include/ark_ddgi.h"
#include "ddgi_device.h"
#include "ddgi_kernels.h"
#include "ddgi_sampling.h"

namespace ark {
namespace dev {

__device__ __forceinline__ float4 ldHalf4(const uint16_t* p, uint32_t i)
{
    if (!p) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint2 w = reinterpret_cast<const uint2*>(p)[i];
    return make_float4(f16_to_f32(static_cast<uint16_t>(w.x & 0xffffu)), f16_to_f32(static_cast<uint16_t>(w.x >> 16)),
                       f16_to_f32(static_cast<uint16_t>(w.y & 0xffffu)), f16_to_f32(static_cast<uint16_t>(w.y >> 16)));
}

__device__ __forceinline__ float4 ldUnorm4(const uint8_t* p, uint32_t i)
{
    if (!p) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t w = reinterpret_cast<const uint32_t*>(p)[i];
    return make_float4(static_cast<float>(w & 0xffu) / 255.0f, static_cast<float>((w >> 8) & 0xffu) / 255.0f,
                       static_cast<float>((w >> 16) & 0xffu) / 255.0f, static_cast<float>(w >> 24) / 255.0f);
}

// mat3(M) * v and M * vec4(x, y, z, w) for a column-major mat4
__device__ __forceinline__ V3 mulDir(const float* M, V3 v)
{
    return { M[0] * v.x + M[4] * v.y + M[8] * v.z, M[1] * v.x + M[5] * v.y + M[9] * v.z, M[2] * v.x + M[6] * v.y + M[10] * v.z };
}

__device__ __forceinline__ float4 mulPoint(const float* M, float x, float y, float z, float w)
{
    return make_float4(M[0] * x + M[4] * y + M[8] * z + M[12] * w, M[1] * x + M[5] * y + M[9] * z + M[13] * w,
                       M[2] * x + M[6] * y + M[10] * z + M[14] * w, M[3] * x + M[7] * y + M[11] * z + M[15] * w);
}

// The 8-probe gather two probes at a time (both probes' taps in flight before their
// weights): 0.189 -> 0.178 ms per 1080p launch, bit-identical; 4 and 8 at a time 0.197 /
// 0.246 (registers), and 6 or 8 waves per SIMD (113 VGPRs today: 4) 0.20 / 0.35 ms
// (profiles/r06_l_compose_ab.txt). k_shade keeps kGatherBatch = 1.
constexpr int kComposeGatherBatch = 2;

// XCD-aware tile order: workgroup L is dispatched to XCD L % 8, so XCD x gets the
// contiguous run of 64 x 4 tiles [x * per, (x + 1) * per) (a horizontal band of the
// image): neighbouring pixels gather the same probes' atlas texels from one L2
// instead of all eight.
__global__ void __launch_bounds__(256) k_lighting_compose(FrameArgs f, ArkComposeDesc c)
{
    const uint32_t tilesX = (c.width + 63u) / 64u, tiles = tilesX * ((c.height + 3u) / 4u);
    const uint32_t per = (tiles + 7u) / 8u;
    const uint32_t tile = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if (tile >= tiles) return;
    const uint32_t x = (tile % tilesX) * 64u + (threadIdx.x & 63u);
    const uint32_t y = (tile / tilesX) * 4u + (threadIdx.x >> 6);
    if (x >= c.width || y >= c.height) return;
    const uint32_t p = y * c.width + x;
    const uint32_t flags = c.flags;

    V3 materialBaseColor = splat(1.0f);
    if (flags & ARK_COMPOSE_MATERIAL_COLOR) {
        const float4 b = ldUnorm4(c.base_color, p);
        materialBaseColor = v3(b.x, b.y, b.z);
    }
    float4 sceneColor = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (flags & ARK_COMPOSE_DIRECT_LIGHT) {
        const float4 d = ldHalf4(c.direct_light, p);
        sceneColor = make_float4(sceneColor.x + d.x, sceneColor.y + d.y, sceneColor.z + d.z, sceneColor.w + d.w);
    }
    V3 rgb = v3(sceneColor.x, sceneColor.y, sceneColor.z);
    if (flags & ARK_COMPOSE_SKIN_DIFFUSE_LIGHT) {
        const float4 di = ldHalf4(c.diffuse_irradiance, p);
        rgb = rgb + v3(di.x, di.y, di.z) * materialBaseColor * splat(1.0f / kPi);
    }
    float ambientOcclusion = 1.0f;
    if ((flags & ARK_COMPOSE_SCREEN_SPACE_OCCLUSION) && c.screen_space_occlusion) ambientOcclusion = c.screen_space_occlusion[p];

    const float nonLinearDepth = c.depth ? c.depth[p] : 0.0f;
    if (nonLinearDepth < 1.0f - 1e-6f) {
        const float4 materialProps = ldUnorm4(c.material, p);
        // .x = roughness only feeds specularBRDF's D and V terms, which the output does not use
        const float metallic = materialProps.y;
        const float occlusion = materialProps.z;
        if (flags & ARK_COMPOSE_BAKED_OCCLUSION) ambientOcclusion = fminf_(ambientOcclusion, occlusion);
        const float4 rr = ldHalf4(c.reflections, p);
        const float4 rd = ldHalf4(c.reflection_direction, p);
        const V3 reflectionRadiance = v3(rr.x, rr.y, rr.z);
        const V3 reflectionWorldDirection = v3(rd.x, rd.y, rd.z);
        const bool hasReflections = dot(reflectionWorldDirection, reflectionWorldDirection) > 1e-4f;
        // camera.glsl:101-106
        const float4 vp = mulPoint(c.view_from_pixel, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, nonLinearDepth, 1.0f);
        const V3 pixelViewSpacePosition = v3(vp.x / vp.w, vp.y / vp.w, vp.z / vp.w);
        const V3 V = -normalize(pixelViewSpacePosition);
        const float4 nv = ldHalf4(c.normal_velocity, p);
        const V3 N = octahedralDecode(nv.x, nv.y);
        const V3 L = mulDir(c.view_from_world, reflectionWorldDirection);
        // specularBRDF's F (brdf.glsl:70-89)
        const V3 H = normalize(L + V);
        const float LdotH = clampf(dot(L, H), 0.0f, 1.0f);
        const V3 F = F_Schlick3(LdotH, mix3(splat(kDielectricReflectance), materialBaseColor, metallic));
        if (hasReflections && (flags & ARK_COMPOSE_GLOSSY_GI)) rgb = rgb + materialBaseColor * reflectionRadiance * 0.25f;
        if (flags & ARK_COMPOSE_DIFFUSE_GI) {
            const float4 bn = ldHalf4(c.bent_normal, p);
            V3 worldSpaceSampleDir;
            if ((flags & ARK_COMPOSE_USE_BENT_NORMAL) && bn.w >= 0.0f) {
                const V3 worldSpaceBentNormal = v3(bn.x, bn.y, bn.z);
                const float bentNormalLength = length(worldSpaceBentNormal);
                worldSpaceSampleDir = worldSpaceBentNormal / bentNormalLength;
                if (flags & ARK_COMPOSE_BENT_NORMAL_OCCLUSION) ambientOcclusion = fminf_(ambientOcclusion, bentNormalLength);
            } else {
                worldSpaceSampleDir = normalize(mulDir(c.world_from_view, N));
            }
            const float4 wp = mulPoint(c.world_from_view, pixelViewSpacePosition.x, pixelViewSpacePosition.y, pixelViewSpacePosition.z, 1.0f);
            const V3 worldSpaceView = normalize(mulDir(c.world_from_view, V));
            const V3 indirectIrradiance = sampleDDGI<kComposeGatherBatch>(f, v3(wp.x, wp.y, wp.z), worldSpaceSampleDir, worldSpaceView);
            const float fudgeFactor = hasReflections ? 1.0f : 0.0f;
            const V3 colorForDiffuse = materialBaseColor * splat(1.0f - metallic * fudgeFactor) * (splat(1.0f) - F * fudgeFactor);
            rgb = rgb + colorForDiffuse * indirectIrradiance * ambientOcclusion;
        }
    }
    uint2 o;
    o.x = static_cast<uint32_t>(f32_to_f16(rgb.x)) | (static_cast<uint32_t>(f32_to_f16(rgb.y)) << 16);
    o.y = static_cast<uint32_t>(f32_to_f16(rgb.z)) | (static_cast<uint32_t>(f32_to_f16(sceneColor.w)) << 16);
    reinterpret_cast<uint2*>(c.out)[p] = o;
}

// DDGI probe debug visualisation (DDGIProbeDebug.cpp:34-71, probeDebug.vert/.frag):
// the reference rasterises a 48x48 sphere per probe and shades each fragment from its
// own probe's tile; here the fragment stage runs on a caller-given batch of (probe
// index, sphere normal) samples, one thread each, and writes the RGBA16F colour the
// fragment would store. Rasterising the spheres is the caller's (out of scope).
__global__ void __launch_bounds__(256) k_probe_debug(FrameArgs f, ArkProbeDebugDesc d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.count) return;
    const uint32_t probe = d.probe_indices[i];
    const V3 dir = normalize(v3(d.directions[3 * i], d.directions[3 * i + 1], d.directions[3 * i + 2]));
    // calculateProbePosition (ddgi/common.glsl:69-77) + 1e-4, then baseGridCoord (probeSampling.glsl:52-57)
    const uint32_t sheet = static_cast<uint32_t>(f.X * f.Z);
    const uint32_t inSheet = probe % sheet;
    const float cx = static_cast<float>(inSheet % static_cast<uint32_t>(f.X));
    const float cy = static_cast<float>(probe / sheet);
    const float cz = static_cast<float>(inSheet / static_cast<uint32_t>(f.X));
    const V3 spacing = v3(f.spacing[0], f.spacing[1], f.spacing[2]), origin = v3(f.origin[0], f.origin[1], f.origin[2]);
    const V3 pos = origin + v3(cx, cy, cz) * spacing + splat(1e-4f);
    const V3 rel = (pos - origin) / spacing;
    const int gx = min(max(static_cast<int>(rel.x), 0), f.X - 1);
    const int gy = min(max(static_cast<int>(rel.y), 0), f.Y - 1);
    const int gz = min(max(static_cast<int>(rel.z), 0), f.Z - 1);
    float u, v, irr[3], vis[2];
    atlasSampleUV(f, gx, gy, gz, dir, ARK_DDGI_IRRADIANCE_RES, 1.0f / static_cast<float>(f.Wi), 1.0f / static_cast<float>(f.Hi), &u, &v);
    atlasFilter<4, 3>(atlasTap<4>(f.irr, f.Wi, f.Hi, u, v), irr);
    atlasSampleUV(f, gx, gy, gz, dir, ARK_DDGI_VISIBILITY_RES, 1.0f / static_cast<float>(f.Wv), 1.0f / static_cast<float>(f.Hv), &u, &v);
    atlasFilter<2, 2>(atlasTap<2>(f.vis, f.Wv, f.Hv, u, v), vis);
    V3 c = v3(1.0f, 0.0f, 1.0f);
    if (d.visualisation == ARK_PROBE_DEBUG_IRRADIANCE) {
        c = pow3(v3(irr[0], irr[1], irr[2]), 5.0f); // sampleIrradianceProbe: pow(raw, DDGI_IRRADIANCE_GAMMA)
    } else if (d.visualisation == ARK_PROBE_DEBUG_DISTANCE) {
        c = splat(d.distance_scale * vis[0]);
        if (vis[0] < 0.0f) c = v3(1.0f, 0.0f, 1.0f);
    } else if (d.visualisation == ARK_PROBE_DEBUG_DISTANCE2) {
        c = splat(d.distance_scale * vis[1]);
    }
    uint2 o;
    o.x = static_cast<uint32_t>(f32_to_f16(c.x)) | (static_cast<uint32_t>(f32_to_f16(c.y)) << 16);
    o.y = static_cast<uint32_t>(f32_to_f16(c.z)) | (0x3c00u << 16);
    reinterpret_cast<uint2*>(d.out)[i] = o;
}

} // namespace dev

hipError_t launch_lighting_compose(const FrameArgs& f, const ArkComposeDesc& c, hipStream_t s)
{
    if (c.width == 0 || c.height == 0) return hipSuccess;
    const uint64_t tiles = static_cast<uint64_t>((c.width + 63u) / 64u) * ((c.height + 3u) / 4u); // 64 x 4 tiles (k_lighting_compose)
    if (tiles > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_lighting_compose, dim3(static_cast<uint32_t>((tiles + 7u) / 8u * 8u)), dim3(256), 0, s, f, c);
    return hipGetLastError();
}

hipError_t launch_probe_debug(const FrameArgs& f, const ArkProbeDebugDesc& d, hipStream_t s)
{
    if (d.count == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_probe_debug, dim3((d.count + 255u) / 256u), dim3(256), 0, s, f, d);
    return hipGetLastError();
}

} // namespace ark
