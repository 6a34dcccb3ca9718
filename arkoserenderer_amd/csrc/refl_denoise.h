// refl_denoise.h — the arithmetic of the reference's reflection denoiser passes, written once:
// historyCopy.comp:24-41, reproject.comp + ffx_denoiser_reflections_reproject.h
// (maxNumSamples = 32), prefilter.comp + ffx_denoiser_reflections_prefilter.h,
// resolveTemporal.comp + ffx_denoiser_reflections_resolve_temporal.h, the common and config
// headers and common/camera.glsl:108-118. The kernels (ddgi_refl_denoise.hip) and the serial
// host restatement (refl_denoise_host.cpp) call these functions in the same order on the same
// 16 x 16 tile words, and both sides are compiled with -ffp-contract=off, so every output byte
// is the same. Pure C++ without a HIP dependency (the host side is also built on its own,
// tests/cpp).
//
// hlsl-on-glsl.glsl:21-24 maps min16float* to float/vec*: the arithmetic is fp32. fp16 appears
// where the shaders pack (the tiles) and at the RGBA16F stores.
//
// Adopted semantics:
//  - texelFetch outside the image (tile aprons, the 2 x 2 slow path) reads 0 in every channel.
//  - textureLod on the history and average planes is bilinear at LOD 0 with repeat wrap in
//    sampleTexture's fp32 formulation (ddgi_device.h) over fp16 texels decoded exactly. A
//    texel coordinate that is NaN or at least 2^30 in magnitude samples as coordinate 0; the
//    slow path's integer texel coordinate of such a value is outside the image.
//  - exp(x) = exp2f_(x * log2(e)), pow(x, 512) = powf_; length, normalize, dot as ddgi_device.h
//    (dot left to right, normalize = v * (1 / sqrt(dot))), mix(x, y, a) = x * (1 - a) + y * a.
//  - fp16 conversion rounds to nearest even; a NaN becomes 0x7e00, and 0x7fc00000 in an R32F store
//    (the sign and payload of a NaN differ between the host's and the device's operations).
//  - PickReprojection's early return (surface history rejected) leaves reprojection_uv
//    undefined; either outcome of the range test that follows stores (0, 1, 1) and skips the
//    lerp into the tile average: the store branch is taken.
//  - reproject's tile reduction writes its first level into words that other lanes' 9 x 9
//    neighbourhoods read, with no barrier between in the shader; all neighbourhood reads come
//    first here.
//  - RoundUp8(v) is v + 8 when v is no multiple of 8 (29 -> 37), as the shader has it.
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ARK_UNROLL _Pragma("unroll")
#define ARK_NO_UNROLL _Pragma("unroll 1")
#else
#define ARK_UNROLL
#define ARK_NO_UNROLL
#endif

#include "ark_fmath.h"

namespace ark {
namespace refl {

// ffx_denoiser_reflections_config.h
constexpr float kGaussianK = 3.0f;
constexpr float kRadianceWeightBias = 0.6f;
constexpr float kRadianceWeightVarianceK = 0.1f;
constexpr float kAvgRadianceLuminanceWeight = 0.3f;
constexpr float kPrefilterVarianceWeight = 4.4f;
constexpr float kSurfaceDiscardVarianceWeight = 1.5f;
constexpr float kPrefilterVarianceBias = 0.1f;
constexpr float kPrefilterNormalSigma = 512.0f;
constexpr float kPrefilterDepthSigma = 4.0f;
constexpr float kDisocclusionNormalWeight = 1.4f;
constexpr float kDisocclusionDepthWeight = 1.0f;
constexpr float kDisocclusionThreshold = 0.9f;
constexpr float kNormalSimilarityThreshold = 0.9999f;
constexpr float kMaxNumSamples = 32.0f; // reproject.comp:187
constexpr float kMirrorRoughness = 0.001f; // prefilter.comp:75
constexpr float kLog2e = 0x1.715476p+0f;
constexpr int kTile = 16, kTileWords = kTile * kTile; // the 8 x 8 group plus its apron of 4

// Everything the four passes read and write: ArkReflDenoiseDesc's planes and scalars.
struct Args {
    uint32_t width, height;
    float noTracingRoughness, temporalStability;
    float worldFromView[16], viewFromProjection[16], prevViewFromWorld[16], prevProjectionFromView[16];
    float zNear, zFar;
    const uint16_t* radiance;       // RGBA16F: rgb radiance, a signed ray length
    const float* depth;             // non-linear depth
    const uint8_t* material;        // RGBA8: byte 0 roughness
    const uint16_t* normalVelocity; // RGBA16F: rg octahedral view-space normal, ba motion vector
    uint16_t *radianceHistory, *normalHistory, *depthHistory; // RGBA16F; depthHistory = depth, roughness, variance, numSamples
    uint16_t *reprojected, *averageRadiance;                  // RGBA16F; averageRadiance is ceil(w/8) x ceil(h/8)
    float *variance, *numSamples;                             // R32F
    uint16_t *resolved, *temporalAccumulation;                // RGBA16F
};

struct F3 {
    float x, y, z;
};
struct F4 {
    float x, y, z, w;
};

ARK_HD F3 f3(float x, float y, float z) { return { x, y, z }; }
ARK_HD F3 add(F3 a, F3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
ARK_HD F3 sub(F3 a, F3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
ARK_HD F3 mul(F3 a, F3 b) { return { a.x * b.x, a.y * b.y, a.z * b.z }; }
ARK_HD F3 mul(F3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
ARK_HD F3 div(F3 a, float s) { return { a.x / s, a.y / s, a.z / s }; }
ARK_HD float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ARK_HD float length(F3 a) { return sqrtf_(dot(a, a)); }
ARK_HD F3 normalize(F3 a) { const float s = 1.0f / sqrtf_(dot(a, a)); return mul(a, s); }
ARK_HD float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
ARK_HD F3 mix3(F3 x, F3 y, float a) { return { mixf(x.x, y.x, a), mixf(x.y, y.y, a), mixf(x.z, y.z, a) }; }
ARK_HD float lerpf(float a, float b, float t) { return a + (b - a) * t; }
ARK_HD bool isinf_(float x) { return fabsf_(x) == inf_(); }
ARK_HD bool bad(float x) { return isinf_(x) || isnan_(x); }
ARK_HD float expf_(float x) { return exp2f_(x * kLog2e); }
ARK_HD float fracf_(float x) { return x - floorf_(x); }

// fp16 storage: round to nearest even, NaN -> 0x7e00 (ddgi_device.h's f32_to_f16)
ARK_HD uint16_t f2h(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(f)); // no fusion of the producing multiply with the conversion
    if (f != f) return 0x7e00u;
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
#else
    const uint32_t u = f2u(f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return 0x7e00u;
    if (a >= 0x477ff000u) return static_cast<uint16_t>(sign | 0x7c00u); // >= 65520 rounds to inf
    if (a < 0x33000001u) return static_cast<uint16_t>(sign);            // <= 2^-25 rounds to 0
    const int e = static_cast<int>(a >> 23) - 127;
    uint32_t m = (a & 0x007fffffu) | 0x00800000u;
    int shift = 13;
    uint32_t base;
    if (e < -14) { // subnormal half
        shift = 13 + (-14 - e);
        base = 0;
    } else {
        base = static_cast<uint32_t>(e + 15) << 10;
        m &= 0x007fffffu;
    }
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
    uint32_t h = base + q;
    if (rem > halfway || (rem == halfway && (h & 1u))) ++h; // a carry walks into the exponent
    return static_cast<uint16_t>(sign | h);
#endif
}
ARK_HD float h2f(uint16_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<float>(__builtin_bit_cast(_Float16, h));
#else
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    if (e == 0x1fu) return u2f(sign | 0x7f800000u | (m << 13));
    if (e) return u2f(sign | ((e + 112u) << 23) | (m << 13));
    const float v = static_cast<float>(m) * 0x1p-24f;
    return sign ? -v : v;
#endif
}
ARK_HD uint32_t pack2(float a, float b) { return static_cast<uint32_t>(f2h(a)) | (static_cast<uint32_t>(f2h(b)) << 16); }
ARK_HD float lo16(uint32_t w) { return h2f(static_cast<uint16_t>(w & 0xffffu)); }
ARK_HD float hi16(uint32_t w) { return h2f(static_cast<uint16_t>(w >> 16)); }

// One RGBA16F texel, a single 8-byte access (planes are 8-byte aligned).
ARK_HD F4 loadTexel(const uint16_t* plane, uint64_t p)
{
    const uint64_t v = reinterpret_cast<const uint64_t*>(plane)[p];
    const uint32_t a = static_cast<uint32_t>(v), b = static_cast<uint32_t>(v >> 32);
    return { lo16(a), hi16(a), lo16(b), hi16(b) };
}
ARK_HD void storeTexel(uint16_t* plane, uint64_t p, float x, float y, float z, float w)
{
    reinterpret_cast<uint64_t*>(plane)[p] = static_cast<uint64_t>(pack2(x, y)) | (static_cast<uint64_t>(pack2(z, w)) << 32);
}
// an R32F store: a NaN is stored as 0x7fc00000, whatever sign and payload the operation gave it
ARK_HD void storeFloat(float* plane, uint64_t p, float v) { plane[p] = isnan_(v) ? nan_() : v; }
ARK_HD bool inside(int x, int y, uint32_t w, uint32_t h) { return x >= 0 && y >= 0 && static_cast<uint32_t>(x) < w && static_cast<uint32_t>(y) < h; }
// texelFetch: 0 outside the image
ARK_HD F4 fetchTexel(const uint16_t* plane, int x, int y, uint32_t w, uint32_t h)
{
    if (!inside(x, y, w, h)) return { 0.0f, 0.0f, 0.0f, 0.0f };
    return loadTexel(plane, static_cast<uint64_t>(y) * w + static_cast<uint32_t>(x));
}
ARK_HD float fetchFloat(const float* plane, int x, int y, uint32_t w, uint32_t h) { return inside(x, y, w, h) ? plane[static_cast<uint64_t>(y) * w + static_cast<uint32_t>(x)] : 0.0f; }
ARK_HD float fetchRoughness(const uint8_t* material, int x, int y, uint32_t w, uint32_t h)
{
    return inside(x, y, w, h) ? static_cast<float>(material[4u * (static_cast<uint64_t>(y) * w + static_cast<uint32_t>(x))]) / 255.0f : 0.0f;
}

ARK_HD int wrapRepeat(int i, int n)
{
    const int m = i % n;
    return m < 0 ? m + n : m;
}
ARK_HD float tameCoord(float x) { return fabsf_(x) < 0x1p30f ? x : 0.0f; }
// textureLod(plane, uv, 0): bilinear, repeat
ARK_HD F4 sampleBilinear(const uint16_t* plane, uint32_t w, uint32_t h, float u, float v)
{
    const float x = tameCoord(u * static_cast<float>(w) - 0.5f), y = tameCoord(v * static_cast<float>(h) - 0.5f);
    const float x0f = floorf_(x), y0f = floorf_(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
    const int W = static_cast<int>(w), H = static_cast<int>(h);
    const uint64_t xa = static_cast<uint64_t>(wrapRepeat(x0, W)), xb = static_cast<uint64_t>(wrapRepeat(x0 + 1, W));
    const uint64_t ya = static_cast<uint64_t>(wrapRepeat(y0, H)), yb = static_cast<uint64_t>(wrapRepeat(y0 + 1, H));
    const F4 t00 = loadTexel(plane, ya * w + xa), t10 = loadTexel(plane, ya * w + xb);
    const F4 t01 = loadTexel(plane, yb * w + xa), t11 = loadTexel(plane, yb * w + xb);
    F4 r;
    r.x = lerpf(lerpf(t00.x, t10.x, fx), lerpf(t01.x, t11.x, fx), fy);
    r.y = lerpf(lerpf(t00.y, t10.y, fx), lerpf(t01.y, t11.y, fx), fy);
    r.z = lerpf(lerpf(t00.z, t10.z, fx), lerpf(t01.z, t11.z, fx), fy);
    r.w = lerpf(lerpf(t00.w, t10.w, fx), lerpf(t01.w, t11.w, fx), fy);
    return r;
}

// octahedral.glsl:26-41 through encoding.glsl decodeNormal
ARK_HD float signNotZero(float f) { return f >= 0.0f ? 1.0f : -1.0f; }
ARK_HD F3 decodeNormal(float ox, float oy)
{
    F3 v = { ox, oy, 1.0f - fabsf_(ox) - fabsf_(oy) };
    if (v.z < 0.0f) {
        const float nx = (1.0f - fabsf_(v.y)) * signNotZero(v.x);
        const float ny = (1.0f - fabsf_(v.x)) * signNotZero(v.y);
        v.x = nx;
        v.y = ny;
    }
    return normalize(v);
}
// column-major GLSL mat3(M) * v and M * vec4
ARK_HD F3 mat3Mul(const float* M, F3 v) { return { M[0] * v.x + M[4] * v.y + M[8] * v.z, M[1] * v.x + M[5] * v.y + M[9] * v.z, M[2] * v.x + M[6] * v.y + M[10] * v.z }; }
ARK_HD F4 mat4Mul(const float* M, float x, float y, float z, float w)
{
    return { M[0] * x + M[4] * y + M[8] * z + M[12] * w, M[1] * x + M[5] * y + M[9] * z + M[13] * w, M[2] * x + M[6] * y + M[10] * z + M[14] * w,
             M[3] * x + M[7] * y + M[11] * z + M[15] * w };
}
// camera.glsl:108-118
ARK_HD F3 unprojectUvDepth(const float* viewFromProjection, float u, float v, float depth)
{
    const F4 p = mat4Mul(viewFromProjection, u * 2.0f - 1.0f, v * 2.0f - 1.0f, depth, 1.0f);
    return { p.x / p.w, p.y / p.w, p.z / p.w };
}
ARK_HD float linearDepth(float nonlinearDepth, float zNear, float zFar) { return zNear * zFar / ((nonlinearDepth * (zFar - zNear)) - zFar); }

// ffx_denoiser_reflections_common.h
ARK_HD uint32_t roundUp8(uint32_t v) { return (v & ~7u) == v ? v : v + 8u; }
ARK_HD float luminance(F3 c) { return fmaxf_(dot(c, f3(0.299f, 0.587f, 0.114f)), 0.001f); }
ARK_HD float temporalVariance(F3 historyRadiance, F3 radiance)
{
    const float hl = luminance(historyRadiance), l = luminance(radiance);
    const float diff = fabsf_(hl - l) / fmaxf_(fmaxf_(hl, l), 0.5f);
    return diff * diff;
}
ARK_HD F3 clipAABB(F3 aabbMin, F3 aabbMax, F3 prevSample)
{
    const F3 center = mul(add(aabbMax, aabbMin), 0.5f);
    const F3 h = mul(sub(aabbMax, aabbMin), 0.5f);
    const F3 extent = { h.x + 0.001f, h.y + 0.001f, h.z + 0.001f };
    const F3 cv = sub(prevSample, center);
    const float maxAbsUnit = fmaxf_(fmaxf_(fabsf_(cv.x / extent.x), fabsf_(cv.y / extent.y)), fabsf_(cv.z / extent.z));
    if (maxAbsUnit > 1.0f) return add(center, div(cv, maxAbsUnit));
    return prevSample;
}
ARK_HD float kernelWeight(float i)
{
    const float radius = 4.0f + 1.0f;
    return expf_(-kGaussianK * (i * i) / (radius * radius));
}
ARK_HD bool isGlossy(const Args& a, float roughness) { return roughness < a.noTracingRoughness; }

// ---- tiles: kTileWords words per array, index y * 16 + x ------------------------------

ARK_HD F3 tileRadiance(const uint32_t* s0, const uint32_t* s1, int x, int y)
{
    const uint32_t a = s0[y * kTile + x], b = s1[y * kTile + x];
    return { lo16(a), hi16(a), lo16(b) };
}
ARK_HD F4 tileRaw(const uint32_t* s0, const uint32_t* s1, int x, int y)
{
    const uint32_t a = s0[y * kTile + x], b = s1[y * kTile + x];
    return { lo16(a), hi16(a), lo16(b), hi16(b) };
}
ARK_HD void tileStore4(uint32_t* s0, uint32_t* s1, int x, int y, F4 v)
{
    s0[y * kTile + x] = pack2(v.x, v.y);
    s1[y * kTile + x] = pack2(v.z, v.w);
}
// reproject's and resolve's InitializeGroupSharedMemory, one lane's four texels
ARK_HD void fillRadianceTile(const Args& a, uint32_t* s0, uint32_t* s1, int px, int py, int gx, int gy)
{
    F4 r[4];
    ARK_UNROLL
    for (int k = 0; k < 4; ++k) r[k] = fetchTexel(a.radiance, px - 4 + (k & 1) * 8, py - 4 + (k >> 1) * 8, a.width, a.height);
    ARK_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int i = (gy + (k >> 1) * 8) * kTile + gx + (k & 1) * 8;
        s0[i] = pack2(r[k].x, r[k].y);
        s1[i] = pack2(r[k].z, r[k].z);
    }
}

struct Moments {
    F3 mean, variance;
};
// EstimateLocalNeighborhoodInGroup: 9 x 9 around (cx, cy), 4 <= cx, cy < 12
ARK_HD Moments localNeighborhood(const uint32_t* s0, const uint32_t* s1, int cx, int cy)
{
    Moments e = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
    float acc = 0.0f;
    ARK_NO_UNROLL // a row at a time: unrolled whole, the 162 tile words are all loaded before the first is used
    for (int j = -4; j <= 4; ++j) {
        const float wj = kernelWeight(static_cast<float>(j));
        ARK_UNROLL
        for (int i = -4; i <= 4; ++i) {
            const F3 r = tileRadiance(s0, s1, cx + i, cy + j);
            const float w = kernelWeight(static_cast<float>(i)) * wj;
            acc += w;
            e.mean = add(e.mean, mul(r, w));
            e.variance = add(e.variance, mul(mul(r, r), w));
        }
    }
    e.mean = div(e.mean, acc);
    e.variance = div(e.variance, acc);
    const F3 d = sub(e.variance, mul(e.mean, e.mean));
    e.variance = { fabsf_(d.x), fabsf_(d.y), fabsf_(d.z) };
    return e;
}

// ---- historyCopy.comp:24-41 -----------------------------------------------------------

ARK_HD F3 worldNormalAt(const Args& a, int px, int py)
{
    const F4 nv = fetchTexel(a.normalVelocity, px, py, a.width, a.height);
    return mat3Mul(a.worldFromView, decodeNormal(nv.x, nv.y));
}
ARK_HD void historyCopyPixel(const Args& a, int px, int py, bool firstCopy)
{
    const uint64_t p = static_cast<uint64_t>(py) * a.width + static_cast<uint32_t>(px);
    const F4 r = loadTexel(a.radiance, p);
    storeTexel(a.radianceHistory, p, r.x, r.y, r.z, 0.0f);
    const F3 n = worldNormalAt(a, px, py);
    storeTexel(a.normalHistory, p, n.x, n.y, n.z, 0.0f);
    const float roughness = static_cast<float>(a.material[4u * p]) / 255.0f;
    const float variance = firstCopy ? 0.0f : a.variance[p];
    const float numSamples = firstCopy ? 0.0f : a.numSamples[p];
    storeTexel(a.depthHistory, p, a.depth[p], roughness, variance, numSamples);
}

// ---- reproject ------------------------------------------------------------------------

ARK_HD float disocclusionFactor(F3 normal, F3 historyNormal, float linDepth, float historyLinDepth)
{
    return expf_(-fabsf_(1.0f - fmaxf_(0.0f, dot(normal, historyNormal))) * kDisocclusionNormalWeight) *
           expf_(-fabsf_(historyLinDepth - linDepth) / linDepth * kDisocclusionDepthWeight);
}
ARK_HD F3 xyz(F4 v) { return { v.x, v.y, v.z }; }
ARK_HD int texelCoord(float v) { return fabsf_(v) < 0x1p30f ? static_cast<int>(v) : -(1 << 30); }

// PickReprojection. False: the surface history was rejected (the early return).
ARK_HD bool pickReprojection(const Args& a, const uint32_t* s0, const uint32_t* s1, int px, int py, int cx, int cy, float roughness, float rayLength, float* factorOut,
                             float uvOut[2], F3* reprojectionOut)
{
    const float W = static_cast<float>(a.width), H = static_cast<float>(a.height);
    const Moments local = localNeighborhood(s0, s1, cx, cy);
    const float u = (static_cast<float>(px) + 0.5f) / W, v = (static_cast<float>(py) + 0.5f) / H;
    const F4 nvTexel = fetchTexel(a.normalVelocity, px, py, a.width, a.height);
    const F3 normal = mat3Mul(a.worldFromView, decodeNormal(nvTexel.x, nvTexel.y));
    const float depth = fetchFloat(a.depth, px, py, a.width, a.height);
    F3 historyNormal, reprojection;
    float historyLinDepth, ru, rv;
    {
        const float su = u - nvTexel.z, sv = v - nvTexel.w; // GetSurfaceReprojection
        // GetHitPositionReprojection
        F3 ray = unprojectUvDepth(a.viewFromProjection, u, v, depth);
        const float surfaceDepth = length(ray);
        const float len = surfaceDepth + rayLength;
        ray = div(ray, surfaceDepth);
        ray = mul(ray, len);
        const F4 world = mat4Mul(a.worldFromView, ray.x, ray.y, ray.z, 1.0f);
        const F4 pv = mat4Mul(a.prevViewFromWorld, world.x, world.y, world.z, 1.0f);
        const F4 pp = mat4Mul(a.prevProjectionFromView, pv.x, pv.y, pv.z, pv.w);
        const float hu = pp.x / pp.w * 0.5f + 0.5f, hv = pp.y / pp.w * 0.5f + 0.5f;

        const F3 surfaceNormal = xyz(sampleBilinear(a.normalHistory, a.width, a.height, su, sv));
        const F3 hitNormal = xyz(sampleBilinear(a.normalHistory, a.width, a.height, hu, hv));
        const F3 surfaceHistory = xyz(sampleBilinear(a.radianceHistory, a.width, a.height, su, sv));
        const F3 hitHistory = xyz(sampleBilinear(a.radianceHistory, a.width, a.height, hu, hv));
        const F3 nn = normalize(normal);
        const float hitSimilarity = dot(normalize(hitNormal), nn);
        const float surfaceSimilarity = dot(normalize(surfaceNormal), nn);
        const F4 hitDrvn = sampleBilinear(a.depthHistory, a.width, a.height, hu, hv);
        const F4 surfaceDrvn = sampleBilinear(a.depthHistory, a.width, a.height, su, sv);
        if (hitSimilarity > kNormalSimilarityThreshold && hitSimilarity + 1.0e-3f > surfaceSimilarity &&
            fabsf_(hitDrvn.y - roughness) < fabsf_(surfaceDrvn.y - roughness) + 1.0e-3f) {
            historyNormal = hitNormal;
            historyLinDepth = linearDepth(hitDrvn.x, a.zNear, a.zFar);
            ru = hu, rv = hv;
            reprojection = hitHistory;
        } else {
            const F3 d = sub(surfaceHistory, local.mean);
            if (dot(d, d) < kSurfaceDiscardVarianceWeight * length(local.variance)) {
                historyNormal = surfaceNormal;
                historyLinDepth = linearDepth(surfaceDrvn.x, a.zNear, a.zFar);
                ru = su, rv = sv;
                reprojection = surfaceHistory;
            } else {
                *factorOut = 0.0f;
                return false;
            }
        }
    }
    const float linDepth = linearDepth(depth, a.zNear, a.zFar);
    float factor = disocclusionFactor(normal, historyNormal, linDepth, historyLinDepth);
    if (!(factor > kDisocclusionThreshold)) {
        if (factor < kDisocclusionThreshold) { // the closest sample in the vicinity; the centre moves with every improvement
            const float du = 1.0f / W, dv = 1.0f / H;
            for (int y = -1; y <= 1; ++y)
                for (int x = -1; x <= 1; ++x) {
                    const float qu = ru + static_cast<float>(x) * du, qv = rv + static_cast<float>(y) * dv;
                    const F3 hn = xyz(sampleBilinear(a.normalHistory, a.width, a.height, qu, qv));
                    const float hd = sampleBilinear(a.depthHistory, a.width, a.height, qu, qv).x;
                    const float w = disocclusionFactor(normal, hn, linDepth, linearDepth(hd, a.zNear, a.zFar));
                    if (w > factor) {
                        factor = w;
                        ru = qu, rv = qv;
                    }
                }
            reprojection = xyz(sampleBilinear(a.radianceHistory, a.width, a.height, ru, rv));
        }
        if (factor < kDisocclusionThreshold) { // the slow path: the 2 x 2 bilinear footprint, texel by texel
            const float uvx = fracf_(W * ru + 0.5f), uvy = fracf_(H * rv + 0.5f);
            const int tx = texelCoord(W * ru - 0.5f), ty = texelCoord(H * rv - 0.5f);
            F3 rad[4], nrm[4];
            float dep[4], w[4];
            for (int k = 0; k < 4; ++k) { // 00, 10, 01, 11
                const int x = tx + (k & 1), y = ty + (k >> 1);
                rad[k] = xyz(fetchTexel(a.radianceHistory, x, y, a.width, a.height));
                nrm[k] = xyz(fetchTexel(a.normalHistory, x, y, a.width, a.height));
                dep[k] = linearDepth(fetchTexel(a.depthHistory, x, y, a.width, a.height).x, a.zNear, a.zFar);
                w[k] = disocclusionFactor(normal, nrm[k], linDepth, dep[k]) > kDisocclusionThreshold / 2.0f ? 1.0f : 0.0f;
            }
            w[0] = w[0] * (1.0f - uvx) * (1.0f - uvy);
            w[1] = w[1] * uvx * (1.0f - uvy);
            w[2] = w[2] * (1.0f - uvx) * uvy;
            w[3] = w[3] * uvx * uvy;
            const float ws = fmaxf_(w[0] + w[1] + w[2] + w[3], 1.0e-3f);
            for (int k = 0; k < 4; ++k) w[k] = w[k] / ws;
            reprojection = add(add(add(mul(rad[0], w[0]), mul(rad[1], w[1])), mul(rad[2], w[2])), mul(rad[3], w[3]));
            const float hld = dep[0] * w[0] + dep[1] * w[1] + dep[2] * w[2] + dep[3] * w[3];
            const F3 hn = add(add(add(mul(nrm[0], w[0]), mul(nrm[1], w[1])), mul(nrm[2], w[2])), mul(nrm[3], w[3]));
            factor = disocclusionFactor(normal, hn, linDepth, hld);
        }
        factor = factor < kDisocclusionThreshold ? 0.0f : factor;
    }
    *factorOut = factor;
    uvOut[0] = ru, uvOut[1] = rv;
    *reprojectionOut = reprojection;
    return true;
}

// FFX_DNSR_Reflections_Reproject up to the reduction: one lane of the tile at (cx, cy) =
// group thread id + 4. Stores reprojected / variance / numSamples of a glossy pixel in the
// image; returns the lane's (radiance * weight, weight) for the 8 x 8 -> 1 reduction.
ARK_HD F4 reprojectPixel(const Args& a, const uint32_t* s0, const uint32_t* s1, int px, int py, int cx, int cy)
{
    // a lane outside the image stores nothing and enters the reduction as 0 (reproject.h:341)
    if (!inside(px, py, a.width, a.height)) return { 0.0f, 0.0f, 0.0f, 0.0f };
    const uint64_t p = static_cast<uint64_t>(py) * a.width + static_cast<uint32_t>(px);
    const float roughness = static_cast<float>(a.material[4u * p]) / 255.0f;
    const F4 texel = loadTexel(a.radiance, p);
    F3 radiance = xyz(texel);
    const float rayLength = texel.w;
    if (isGlossy(a, roughness)) {
        float factor, uv[2] = { 0.0f, 0.0f };
        F3 reprojection = { 0.0f, 0.0f, 0.0f };
        const bool picked = pickReprojection(a, s0, s1, px, py, cx, cy, roughness, rayLength, &factor, uv, &reprojection);
        bool keep = false;
        if (picked && uv[0] > 0.0f && uv[1] > 0.0f && uv[0] < 1.0f && uv[1] < 1.0f) {
            const F4 drvn = sampleBilinear(a.depthHistory, a.width, a.height, uv[0], uv[1]);
            const float prevVariance = drvn.z;
            float numSamples = drvn.w * factor;
            const float maxSamples = fmaxf_(8.0f, kMaxNumSamples * (1.0f - expf_(-roughness * 100.0f)));
            numSamples = fminf_(maxSamples, numSamples + 1.0f);
            const float newVariance = temporalVariance(radiance, reprojection);
            if (!(factor < kDisocclusionThreshold)) {
                keep = true;
                storeTexel(a.reprojected, p, reprojection.x, reprojection.y, reprojection.z, 0.0f);
                storeFloat(a.variance, p, mixf(newVariance, prevVariance, 1.0f / numSamples));
                storeFloat(a.numSamples, p, numSamples);
                radiance = mix3(radiance, reprojection, 0.3f);
            }
        }
        if (!keep) {
            storeTexel(a.reprojected, p, 0.0f, 0.0f, 0.0f, 0.0f);
            a.variance[p] = 1.0f;
            a.numSamples[p] = 1.0f;
        }
    }
    float weight = fmaxf_(expf_(-luminance(radiance) * kAvgRadianceLuminanceWeight), 1.0e-2f);
    radiance = mul(radiance, weight);
    if (bad(radiance.x) || bad(radiance.y) || bad(radiance.z) || weight > 1.0e3f) {
        radiance = { 0.0f, 0.0f, 0.0f };
        weight = 0.0f;
    }
    return { radiance.x, radiance.y, radiance.z, weight };
}
// One lane's part of reduction level i = 2, 4, 8: 00 + 01 + 10 + 11 with 01 = (ix, oy) and
// 10 = (ox, iy), stored back as fp16.
ARK_HD void reduceStep(uint32_t* s0, uint32_t* s1, int gx, int gy, int i)
{
    const int ox = gx * i, oy = gy * i, ix = ox + i / 2, iy = oy + i / 2;
    if (ix < 8 && iy < 8) {
        const F4 w00 = tileRaw(s0, s1, ox, oy), w10 = tileRaw(s0, s1, ox, iy), w01 = tileRaw(s0, s1, ix, oy), w11 = tileRaw(s0, s1, ix, iy);
        tileStore4(s0, s1, ox, oy, { w00.x + w01.x + w10.x + w11.x, w00.y + w01.y + w10.y + w11.y, w00.z + w01.z + w10.z + w11.z, w00.w + w01.w + w10.w + w11.w });
    }
}
ARK_HD void storeAverage(const Args& a, const uint32_t* s0, const uint32_t* s1, uint32_t tileX, uint32_t tileY)
{
    const F4 sum = tileRaw(s0, s1, 0, 0);
    const float acc = fmaxf_(sum.w, 1.0e-3f);
    storeTexel(a.averageRadiance, static_cast<uint64_t>(tileY) * ((a.width + 7u) / 8u) + tileX, sum.x / acc, sum.y / acc, sum.z / acc, 0.0f);
}

// uv8 lookup of prefilter and resolve: the average plane's own extent, divided by RoundUp8
ARK_HD F3 sampleAverage(const Args& a, int px, int py)
{
    const float u = (static_cast<float>(px) + 0.5f) / static_cast<float>(roundUp8(a.width));
    const float v = (static_cast<float>(py) + 0.5f) / static_cast<float>(roundUp8(a.height));
    return xyz(sampleBilinear(a.averageRadiance, (a.width + 7u) / 8u, (a.height + 7u) / 8u, u, v));
}

// ---- prefilter: tile words s0..s3 (radiance xy, zz, normal xy, normal z + variance), fp32 depth

ARK_HD void fillPrefilterTile(const Args& a, uint32_t* s0, uint32_t* s1, uint32_t* s2, uint32_t* s3, float* sd, int px, int py, int gx, int gy)
{
    F3 rad[4], nrm[4];
    float var[4], dep[4];
    ARK_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int x = px - 4 + (k & 1) * 8, y = py - 4 + (k >> 1) * 8;
        rad[k] = xyz(fetchTexel(a.radiance, x, y, a.width, a.height));
        var[k] = fetchFloat(a.variance, x, y, a.width, a.height);
        const F4 nv = fetchTexel(a.normalVelocity, x, y, a.width, a.height);
        nrm[k] = decodeNormal(nv.x, nv.y); // view space
        dep[k] = fabsf_(linearDepth(fetchFloat(a.depth, x, y, a.width, a.height), a.zNear, a.zFar));
    }
    ARK_UNROLL
    for (int k = 0; k < 4; ++k) {
        const int i = (gy + (k >> 1) * 8) * kTile + gx + (k & 1) * 8;
        s0[i] = pack2(rad[k].x, rad[k].y);
        s1[i] = pack2(rad[k].z, rad[k].z);
        s2[i] = pack2(nrm[k].x, nrm[k].y);
        s3[i] = pack2(nrm[k].z, var[k]);
        sd[i] = dep[k];
    }
}
ARK_HD float radianceWeight(F3 center, F3 neighbor, float variance)
{
    return fmaxf_(expf_(-(kRadianceWeightBias + variance * kRadianceWeightVarianceK) * length(sub(center, neighbor))), 1.0e-2f);
}
// FFX_DNSR_Reflections_Prefilter after the tile is filled; the lane is inside the image
ARK_HD void prefilterPixel(const Args& a, const uint32_t* s0, const uint32_t* s1, const uint32_t* s2, const uint32_t* s3, const float* sd, int px, int py, int cx, int cy)
{
    const uint64_t p = static_cast<uint64_t>(py) * a.width + static_cast<uint32_t>(px);
    const float roughness = static_cast<float>(a.material[4u * p]) / 255.0f;
    const int c = cy * kTile + cx;
    const F3 cRad = tileRadiance(s0, s1, cx, cy);
    const F3 cNrm = { lo16(s2[c]), hi16(s2[c]), lo16(s3[c]) };
    const float cVar = hi16(s3[c]), cDepth = sd[c];
    F3 outRad = cRad;
    float outVar = cVar;
    if (cVar > 0.0f && isGlossy(a, roughness) && !(roughness < kMirrorRoughness)) {
        const F3 avg = sampleAverage(a, px, py);
        // First 15 of Halton(2, 3) stretched to [-3, 3] (prefilter.h:112-113)
        const int offs[15][2] = { { 0, 1 }, { -2, 1 }, { 2, -3 }, { -3, 0 }, { 1, 2 }, { -1, -2 }, { 3, 0 }, { -3, 3 }, { 0, -3 }, { -1, -1 }, { 2, 1 }, { -2, -2 }, { 1, 0 }, { 0, 2 }, { 3, -1 } };
        float accW = radianceWeight(avg, cRad, cVar);
        F3 accRad = mul(cRad, accW);
        float accVar = cVar * accW * accW;
        const float varianceWeight = fmaxf_(kPrefilterVarianceBias, 1.0f - expf_(-(cVar * kPrefilterVarianceWeight)));
        ARK_UNROLL
        for (int k = 0; k < 15; ++k) {
            const int x = cx + offs[k][0], y = cy + offs[k][1], n = y * kTile + x;
            const F3 nRad = tileRadiance(s0, s1, x, y);
            const F3 nNrm = { lo16(s2[n]), hi16(s2[n]), lo16(s3[n]) };
            const float nVar = hi16(s3[n]), nDepth = sd[n];
            float w = powf_(fmaxf_(dot(cNrm, nNrm), 0.0f), kPrefilterNormalSigma);
            w *= expf_(-fabsf_(cDepth - nDepth) * cDepth * kPrefilterDepthSigma);
            w *= radianceWeight(avg, nRad, cVar);
            w *= varianceWeight;
            accW += w;
            accRad = add(accRad, mul(nRad, w));
            accVar += w * w * nVar;
        }
        outRad = div(accRad, accW);
        outVar = accVar / (accW * accW);
    }
    storeTexel(a.resolved, p, outRad.x, outRad.y, outRad.z, outVar);
}

// ---- resolve temporal: the radiance tile of fillRadianceTile; the lane is inside the image

ARK_HD void resolveTemporalPixel(const Args& a, const uint32_t* s0, const uint32_t* s1, int px, int py, int cx, int cy)
{
    const uint64_t p = static_cast<uint64_t>(py) * a.width + static_cast<uint32_t>(px);
    F3 newSignal = tileRadiance(s0, s1, cx, cy);
    const float roughness = static_cast<float>(a.material[4u * p]) / 255.0f;
    float newVariance = a.variance[p];
    if (isGlossy(a, roughness)) {
        const float numSamples = a.numSamples[p];
        F3 avg = sampleAverage(a, px, py);
        const F3 oldSignal = xyz(loadTexel(a.reprojected, p));
        Moments local = localNeighborhood(s0, s1, cx, cy);
        const float spread = length(sub(local.mean, avg));
        const F3 sd = { sqrtf_(local.variance.x) + spread, sqrtf_(local.variance.y) + spread, sqrtf_(local.variance.z) + spread };
        const F3 colorStd = mul(mul(sd, a.temporalStability), 1.4f);
        local.mean = mix3(local.mean, avg, 0.2f);
        const F3 clippedOld = clipAABB(sub(local.mean, colorStd), add(local.mean, colorStd), oldSignal);
        const float accumulationSpeed = 1.0f / fmaxf_(numSamples, 1.0f);
        const float weight = 1.0f - accumulationSpeed;
        newSignal = mix3(newSignal, avg, 1.0f / fmaxf_(numSamples + 1.0f, 1.0f));
        const F3 cs1 = mul(colorStd, 1.0f);
        newSignal = clipAABB(sub(avg, cs1), add(avg, cs1), newSignal);
        newSignal = mix3(newSignal, clippedOld, weight);
        newVariance = mixf(temporalVariance(newSignal, clippedOld), newVariance, weight);
        if (bad(newSignal.x) || bad(newSignal.y) || bad(newSignal.z) || bad(newVariance)) {
            newSignal = { 0.0f, 0.0f, 0.0f };
            newVariance = 0.0f;
        }
    }
    storeTexel(a.temporalAccumulation, p, newSignal.x, newSignal.y, newSignal.z, newVariance);
}

} // namespace refl
} // namespace ark
