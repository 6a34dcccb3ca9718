// rt_shadows.h — the arithmetic of the reference's local-light shadow raygen
// (arkose/shaders/rt-shadow/raygen.rgen:33-80), written once: k_rtshadow_gen
// (ddgi_rt_shadows.hip) and the serial host restatement (rt_shadows_host.cpp) call these
// functions in the same order, and both sides are compiled with -ffp-contract=off, so their
// rays are the same bits. Pure C++ without a HIP dependency (the host side is also built on
// its own, tests/cpp).
//
// Adopted semantics:
//  - normalize is the kernels' own (ddgi_device.h): v * (1 / sqrt(dot(v, v))), dot left to right.
//  - camera.worldFromView * camera.viewFromProjection is formed first (column-major mat4
//    product, sums in index order), then applied to vec4(uv * 2 - 1, depth, 1); the three
//    divisions by w are separate fp32 divisions.
//  - sign(x) is 1, -1 or 0; sign(+-0) = sign(NaN) = 0. With n.z == 0 createOrthonormalBasis
//    divides by zero, 0 * inf makes b1 NaN, the light sample and the ray length are NaN, the
//    cone test (a comparison with NaN) is false and the ray falls under the traversal's
//    rule: !(tmax >= tmin) is not traced and counts as lit.
//  - Every light of one frame restarts the generator from the pixel's seed (the reference
//    runs one traceRays per light with the same frameIndex), so the disc point is the same
//    for all lights of a pixel.
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "ark_fmath.h"

namespace ark {
namespace rtshadow {

constexpr float kTmin = 0.025f;           // raygen.rgen:61 (k_trace_shadow's tmin)
constexpr float kSkyDepth = 1.0f - 1e-6f; // raygen.rgen:38, the fp32 difference
constexpr uint32_t kMaxLights = 16;       // ARK_RT_SHADOWS_MAX_LIGHTS: the owner word's light bits

// random.glsl:17-53
ARK_HD uint32_t wangHash(uint32_t seed)
{
    seed = (seed ^ 61u) ^ (seed >> 16);
    seed *= 9u;
    seed = seed ^ (seed >> 4);
    seed *= 0x27d4eb2du;
    seed = seed ^ (seed >> 15);
    return seed;
}
ARK_HD uint32_t randXorshift(uint32_t state)
{
    state ^= (state << 13);
    state ^= (state >> 17);
    state ^= (state << 5);
    return state;
}
ARK_HD float randomFloat(uint32_t& state)
{
    state = randXorshift(state);
    return static_cast<float>(state) * (1.0f / 4294967296.0f);
}

// raygen.rgen:49 seedRandom((frameIndex() + 1) * (pixelCoord.x + pixelCoord.y * 4000)), uint32 wrap-around
ARK_HD uint32_t pixelSeed(uint32_t frameIndex, uint32_t px, uint32_t py) { return wangHash((frameIndex + 1u) * (px + py * 4000u)); }

// random.glsl:68-76 randomPointInDisk(): theta first, then r
ARK_HD void pointInDisk(uint32_t& state, float* x, float* y)
{
    const float theta = kTwoPi * randomFloat(state);
    const float r = sqrtf_(randomFloat(state));
    float s, c;
    sincosf_(theta, &s, &c);
    *x = r * c;
    *y = r * s;
}

// column-major GLSL mat4 product, sums in index order (k_refl_setup's reflMat4Mul)
ARK_HD void mat4Mul(const float* A, const float* B, float* C)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            C[c * 4 + r] = A[r] * B[c * 4] + A[4 + r] * B[c * 4 + 1] + A[8 + r] * B[c * 4 + 2] + A[12 + r] * B[c * 4 + 3];
}

// raygen.rgen:42-45: PW = worldFromView * viewFromProjection
ARK_HD void shadingPoint(const float* PW, uint32_t px, uint32_t py, uint32_t width, uint32_t height, float depth, float P[3])
{
    const float u = (static_cast<float>(px) + 0.5f) / static_cast<float>(width);
    const float v = (static_cast<float>(py) + 0.5f) / static_cast<float>(height);
    const float x = u * 2.0f - 1.0f, y = v * 2.0f - 1.0f;
    float h[4];
    for (int i = 0; i < 4; ++i) h[i] = PW[i] * x + PW[4 + i] * y + PW[8 + i] * depth + PW[12 + i] * 1.0f;
    P[0] = h[0] / h[3];
    P[1] = h[1] / h[3];
    P[2] = h[2] / h[3];
}

ARK_HD float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ARK_HD float signf(float x) { return x > 0.0f ? 1.0f : x < 0.0f ? -1.0f : 0.0f; }

// common.glsl:91-98 createOrthonormalBasis
ARK_HD void orthonormalBasis(const float n[3], float b1[3], float b2[3])
{
    const float zSign = signf(n[2]);
    const float a = -1.0f / (zSign + n[2]);
    const float b = n[0] * n[1] * a;
    b1[0] = 1.0f + zSign * n[0] * n[0] * a;
    b1[1] = zSign * b;
    b1[2] = -zSign * n[0];
    b2[0] = b;
    b2[1] = zSign + n[1] * n[1] * a;
    b2[2] = -n[1];
}

// One light of one pixel, raygen.rgen:22-31 and :50-59: the ray from P towards the disc
// point (diskX, diskY are pointInDisk's, not yet scaled by the radius). light = position[3],
// direction[3], outer cone angle cosine, source radius (ArkRtShadowLight's floats). False:
// outside the cone (mask 0, no ray). True: trace origin P, direction L, [kTmin, *tmax].
ARK_HD bool lightRay(const float P[3], const float* light, float diskX, float diskY, float L[3], float* tmax)
{
    const float toCenter[3] = { light[0] - P[0], light[1] - P[1], light[2] - P[2] };
    const float inv = 1.0f / sqrtf_(dot3(toCenter, toCenter));
    const float n[3] = { toCenter[0] * inv, toCenter[1] * inv, toCenter[2] * inv };
    float b1[3], b2[3];
    orthonormalBasis(n, b1, b2);
    const float dx = diskX * light[7], dy = diskY * light[7];
    float toLight[3];
    for (int i = 0; i < 3; ++i) toLight[i] = (light[i] + dx * b1[i] + dy * b2[i]) - P[i];
    const float dist = sqrtf_(dot3(toLight, toLight));
    for (int i = 0; i < 3; ++i) L[i] = toLight[i] / dist;
    *tmax = dist;
    const float mL[3] = { -L[0], -L[1], -L[2] };
    return !(dot3(mL, light + 3) < light[6]);
}

} // namespace rtshadow
} // namespace ark
