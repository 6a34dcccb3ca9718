// shading_math.h — the shading arithmetic of the kernels without a HIP dependency: vectors,
// the reference's random numbers, octahedral and spherical mappings, the bilinear texture
// fetch and the Filament BRDF. ddgi_device.h includes it for the kernels; the host
// restatements that need the same bits (path_tracer_host.cpp) include it directly, so there is
// one copy of each function. The texel type of sampleTexture is a template parameter (float4
// in the kernels, a plain struct of four floats on the host).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "ark_fmath.h"
#include "../../include/ark_ddgi.h"
#include "ddgi_types.h"

namespace ark {
namespace dev {

struct V3 {
    float x, y, z;
};
ARK_HD V3 v3(float x, float y, float z) { return { x, y, z }; }
ARK_HD V3 operator+(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
ARK_HD V3 operator-(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
ARK_HD V3 operator-(V3 a) { return { -a.x, -a.y, -a.z }; }
ARK_HD V3 operator*(V3 a, V3 b) { return { a.x * b.x, a.y * b.y, a.z * b.z }; }
ARK_HD V3 operator*(V3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
ARK_HD V3 operator*(float s, V3 a) { return { s * a.x, s * a.y, s * a.z }; }
ARK_HD V3 operator/(V3 a, float s) { return { a.x / s, a.y / s, a.z / s }; }
ARK_HD V3 operator/(V3 a, V3 b) { return { a.x / b.x, a.y / b.y, a.z / b.z }; }
ARK_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ARK_HD V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
ARK_HD float length(V3 a) { return sqrtf_(dot(a, a)); }
ARK_HD V3 normalize(V3 a) { float s = 1.0f / sqrtf_(dot(a, a)); return a * s; }
ARK_HD float saturate(float x) { return fminf_(fmaxf_(x, 0.0f), 1.0f); }
ARK_HD float clampf(float x, float lo, float hi) { return fminf_(fmaxf_(x, lo), hi); }
ARK_HD float square(float x) { return x * x; }
ARK_HD float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }
ARK_HD V3 mix3(V3 x, V3 y, float a) { return { mixf(x.x, y.x, a), mixf(x.y, y.y, a), mixf(x.z, y.z, a) }; }
ARK_HD V3 pow3(V3 v, float e) { return { powf_(v.x, e), powf_(v.y, e), powf_(v.z, e) }; }
ARK_HD V3 splat(float s) { return { s, s, s }; }
ARK_HD float lerpf(float a, float b, float t) { return a + (b - a) * t; }

// random.glsl:25-48
ARK_HD uint32_t wang_hash(uint32_t seed)
{
    seed = (seed ^ 61u) ^ (seed >> 16);
    seed *= 9u;
    seed = seed ^ (seed >> 4);
    seed *= 0x27d4eb2du;
    seed = seed ^ (seed >> 15);
    return seed;
}
ARK_HD uint32_t rand_xorshift(uint32_t state)
{
    state ^= (state << 13);
    state ^= (state >> 17);
    state ^= (state << 5);
    return state;
}
ARK_HD float randomFloat(uint32_t& state)
{
    state = rand_xorshift(state);
    return static_cast<float>(state) * (1.0f / 4294967296.0f);
}

// axisAngleRotate (common.glsl:133-142) with sin/cos of the per-probe angle hoisted.
ARK_HD V3 rotate(V3 v, V3 k, float s, float c)
{
    return v * c + cross(k, v) * s + k * dot(k, v) * (1.0f - c);
}

// octahedral.glsl:10-41
ARK_HD float signNotZero(float f) { return (f >= 0.0f) ? 1.0f : -1.0f; }
ARK_HD void octahedralEncode(V3 v, float* ox, float* oy)
{
    float l1norm = fabsf_(v.x) + fabsf_(v.y) + fabsf_(v.z);
    float inv = 1.0f / l1norm;
    float rx = v.x * inv, ry = v.y * inv;
    if (v.z < 0.0f) {
        float nx = (1.0f - fabsf_(ry)) * signNotZero(rx);
        float ny = (1.0f - fabsf_(rx)) * signNotZero(ry);
        rx = nx;
        ry = ny;
    }
    *ox = rx;
    *oy = ry;
}
ARK_HD V3 octahedralDecode(float ox, float oy)
{
    V3 v = { ox, oy, 1.0f - fabsf_(ox) - fabsf_(oy) };
    if (v.z < 0.0f) {
        float nx = (1.0f - fabsf_(v.y)) * signNotZero(v.x);
        float ny = (1.0f - fabsf_(v.x)) * signNotZero(v.y);
        v.x = nx;
        v.y = ny;
    }
    return normalize(v);
}

// spherical.glsl:6-13
ARK_HD void sphericalUvFromDirection(V3 d, float* u, float* v)
{
    float phi = atan2f_(d.z, d.x);
    float theta = acosf_(clampf(d.y, -1.0f, 1.0f));
    if (phi < 0.0f) phi += kTwoPi;
    *u = phi / kTwoPi;
    *v = theta / kPi;
}

// Texel wrap of one axis (GpuTextureInfo.wrap: s in bits 0-3, t in 4-7, normalised
// by ark_ddgi_set_scene): clamp to edge, mirrored repeat (period 2n, the second
// half reversed) or repeat.
ARK_HD int wrapCoord(int i, int n, int wrap)
{
#if defined(__HIPCC__)
    if (wrap == ARK_WRAP_CLAMP_TO_EDGE) return min(max(i, 0), n - 1);
#else
    if (wrap == ARK_WRAP_CLAMP_TO_EDGE) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
#endif
    if (wrap == ARK_WRAP_MIRRORED_REPEAT) {
        int m = i % (2 * n);
        m = m < 0 ? m + 2 * n : m;
        return m < n ? m : 2 * n - 1 - m;
    }
    int m = i % n;
    return m < 0 ? m + n : m;
}

// sRGB EOTF applied per texel before filtering (Vulkan sRGB formats).
ARK_HD float srgbToLinear(float c) { return c <= 0.04045f ? c / 12.92f : powf_((c + 0.055f) / 1.055f, 2.4f); }

// Channel c of texel p of an ArkTexture's data as the texel pool holds it (ark_ddgi_set_scene's
// decode); false: an unknown format.
ARK_HD bool decodeTexel(int format, const void* data, size_t p, int c, float* out)
{
    float v = 0.0f;
    switch (format) {
    case ARK_TEX_RGBA8_UNORM: v = static_cast<float>(static_cast<const uint8_t*>(data)[p * 4 + c]) / 255.0f; break;
    case ARK_TEX_RGBA8_SRGB:
        v = static_cast<float>(static_cast<const uint8_t*>(data)[p * 4 + c]) / 255.0f;
        if (c < 3) v = srgbToLinear(v);
        break;
    case ARK_TEX_R32F: v = c == 0 ? static_cast<const float*>(data)[p] : (c == 3 ? 1.0f : 0.0f); break;
    case ARK_TEX_RGBA32F: v = static_cast<const float*>(data)[p * 4 + c]; break;
    default: return false;
    }
    *out = v;
    return true;
}

// Bilinear LOD-0 fetch from a decoded float4 texture (see oracle sampleBilinear).
template<class T4>
ARK_HD T4 sampleTexture(const GpuTextureInfo* __restrict__ infos, const T4* __restrict__ texels, int idx, float u, float v)
{
    const GpuTextureInfo ti = infos[idx];
    float x = u * static_cast<float>(ti.width) - 0.5f;
    float y = v * static_cast<float>(ti.height) - 0.5f;
    float x0f = floorf_(x), y0f = floorf_(y);
    float fx = x - x0f, fy = y - y0f;
    int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
    const int ws = ti.wrap & 0xf, wt = (ti.wrap >> 4) & 0xf;
    int xa = wrapCoord(x0, ti.width, ws), xb = wrapCoord(x0 + 1, ti.width, ws);
    int ya = wrapCoord(y0, ti.height, wt), yb = wrapCoord(y0 + 1, ti.height, wt);
    const T4* base = texels + ti.texel_offset;
    T4 t00 = base[static_cast<size_t>(ya) * ti.width + xa];
    T4 t10 = base[static_cast<size_t>(ya) * ti.width + xb];
    T4 t01 = base[static_cast<size_t>(yb) * ti.width + xa];
    T4 t11 = base[static_cast<size_t>(yb) * ti.width + xb];
    T4 r;
    r.x = lerpf(lerpf(t00.x, t10.x, fx), lerpf(t01.x, t11.x, fx), fy);
    r.y = lerpf(lerpf(t00.y, t10.y, fx), lerpf(t01.y, t11.y, fx), fy);
    r.z = lerpf(lerpf(t00.z, t10.z, fx), lerpf(t01.z, t11.z, fx), fy);
    r.w = lerpf(lerpf(t00.w, t10.w, fx), lerpf(t01.w, t11.w, fx), fy);
    return r;
}

// brdf.glsl:17-148 (Filament BRDF) -------------------------------------------
constexpr float kDielectricReflectance = 0.04f;

ARK_HD float D_GGX(float NdotH, float a)
{
    float a2 = a * a;
    float f = (NdotH * a2 - NdotH) * NdotH + 1.0f;
    return a2 / (kPi * f * f + 1e-20f);
}
ARK_HD float F_Schlick1(float VdotH, float f0) { return f0 + (1.0f - f0) * powf_(1.0f - VdotH, 5.0f); }
ARK_HD V3 F_Schlick3(float VdotH, V3 f0)
{
    float p = powf_(1.0f - VdotH, 5.0f);
    return f0 + (splat(1.0f) - f0) * p;
}
ARK_HD float V_SmithGGXCorrelated(float NdotV, float NdotL, float a)
{
    float a2 = a * a;
    float GGXL = NdotV * sqrtf_((-NdotL * a2 + NdotL) * NdotL + a2);
    float GGXV = NdotL * sqrtf_((-NdotV * a2 + NdotV) * NdotV + a2);
    return 0.5f / (GGXV + GGXL + 1e-20f);
}
ARK_HD V3 evaluateDefaultBRDF(V3 L, V3 V, V3 N, V3 baseColor, float roughness, float metallic, float clearcoat, float ccRough)
{
    // clearcoatBRDF (brdf.glsl:55-68)
    V3 H = normalize(L + V);
    float NdotHc = saturate(dot(N, H));
    float LdotHc = saturate(dot(L, H));
    float ac = square(clampf(ccRough, 0.1f, 1.0f));
    float Dc = D_GGX(NdotHc, ac);
    float Vc = 0.25f / square(LdotHc);
    float F_c = F_Schlick1(LdotHc, kDielectricReflectance) * clearcoat;
    float Fr_c = Dc * Vc * F_c;
    // specularBRDF (brdf.glsl:70-89)
    V3 Hs = normalize(L + V);
    float NdotV = fabsf_(dot(N, V)) + 1e-5f;
    float NdotL = clampf(dot(N, L), 0.0f, 1.0f);
    float NdotH = clampf(dot(N, Hs), 0.0f, 1.0f);
    float LdotH = clampf(dot(L, Hs), 0.0f, 1.0f);
    float a = square(roughness);
    V3 f0 = mix3(splat(kDielectricReflectance), baseColor, metallic);
    V3 F_s = F_Schlick3(LdotH, f0);
    float D = D_GGX(NdotH, a);
    float Vv = V_SmithGGXCorrelated(NdotV, NdotL, a);
    V3 Fr_s = F_s * D * Vv;
    V3 diffuseColor = splat(1.0f - metallic) * baseColor;
    V3 Fr_d = diffuseColor * splat(1.0f / kPi);
    return (Fr_d * (splat(1.0f) - F_s) + Fr_s) * (1.0f - F_c) + splat(Fr_c);
}

// Möller–Trumbore, identical op order to the oracle's intersectTri. The cross and dot
// products are fused explicitly (crossFma / dotFma: 6 and 3 VALU instead of 9 and 5;
// the ray-triangle test is the traversal step's second largest block), in the same
// places as the oracle, so results stay bit-exact under -ffp-contract=off.
ARK_HD V3 crossFma(V3 a, V3 b)
{
    return { fmaf_(a.y, b.z, -(a.z * b.y)), fmaf_(a.z, b.x, -(a.x * b.z)), fmaf_(a.x, b.y, -(a.y * b.x)) };
}
ARK_HD float dotFma3(V3 a, V3 b) { return fmaf_(a.x, b.x, fmaf_(a.y, b.y, a.z * b.z)); }

// Branch free: in a wave some lane passes each early-out test on almost every
// step, so the early returns saved no VALU and cost an exec-mask branch each
// (~14 SALU per traversal step). The accepted set is the oracle's: u <= 1 follows
// from v >= 0 and RN(u + v) <= 1 (rounding is monotonic), and det == 0 gives
// inv = +-inf, so u or v is NaN or infinite and one of u >= 0, v >= 0, u + v <= 1
// fails, as the oracle's early return rejects it; the values of an accepted hit
// are computed exactly as the oracle computes them.
ARK_HD bool intersectTri(V3 o, V3 d, float tmin, float tmax, const GpuTriangle& tr, float* outT, float* outU, float* outV, bool* backfaceDet)
{
    V3 v0 = { tr.t0[0], tr.t0[1], tr.t0[2] };
    V3 e1 = { tr.t0[3], tr.t1[0], tr.t1[1] };
    V3 e2 = { tr.t1[2], tr.t1[3], tr.t2[0] };
    V3 p = crossFma(d, e2);
    float det = dotFma3(e1, p);
    float inv = 1.0f / det;
    V3 s = o - v0;
    float u = dotFma3(s, p) * inv;
    V3 q = crossFma(s, e1);
    float v = dotFma3(d, q) * inv;
    float tt = dotFma3(e2, q) * inv;
    *outT = tt;
    *outU = u;
    *outV = v;
    *backfaceDet = det < 0.0f;
    return (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (tt >= tmin) & (tt <= tmax);
}

// SceneArgs::sample's rule for a texture index: an index outside the scene's textures reads
// the 1 x 1 white default, which filters to exactly (1, 1, 1, 1) for finite coordinates and is
// not fetched.
template<class T4>
ARK_HD T4 sampleOrWhite(const GpuTextureInfo* __restrict__ infos, const T4* __restrict__ texels, int textureCount, int whiteTexture, int idx, float u, float v)
{
    const int r = (idx >= 0 && idx < textureCount) ? idx : whiteTexture;
    if (r == whiteTexture && fabsf_(u) < inf_() && fabsf_(v) < inf_()) {
        T4 one;
        one.x = one.y = one.z = one.w = 1.0f;
        return one;
    }
    return sampleTexture(infos, texels, r, u, v);
}

} // namespace dev
} // namespace ark
