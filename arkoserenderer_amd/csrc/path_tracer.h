// path_tracer.h — the arithmetic of the reference's path tracer (arkose/shaders/pathtracer/
// pathtracer.rgen, closesthit.rchit, material.glsl, common.glsl, accumulate.comp), written
// once: the kernels of ddgi_path_tracer.hip and the serial host restatement
// (path_tracer_host.cpp) call these functions in the same order, and both sides are compiled
// with -ffp-contract=off, so a path is the same bits on both. Pure C++ without a HIP
// dependency (the host side is also built on its own, tests/cpp). Vectors, the BRDF and the
// texture fetch are shading_math.h's; transcendentals are ark_fmath.h's.
//
// The pinned semantics (DESIGN.md "Path tracer") are marked [1] .. [9] where they are decided.
#pragma once

#include <stdint.h>

#include "rt_shadows.h"
#include "shading_math.h"

namespace ark {
namespace pt {

using dev::V3;
using dev::v3;

constexpr uint32_t kMaxSegments = 16;        // pathtracer.rgen:61 maxRayRepth
constexpr float kAttenuationFloor = 0.00001f; // pathtracer.rgen:67
constexpr float kNextTmin = 0.0001f;         // pathtracer.rgen:71 [2]
constexpr float kShadowTmin = 0.025f;        // closesthit.rchit:45 (k_trace_shadow's tmin) [5]
constexpr float kIorAir = 1.0f, kIorGlass = 1.5f;
// [4] the reference's default normal map: a 1 x 1 RGBA8 texel of (0.5, 0.5, 1, 1) * 255.99
// truncated, i.e. (127, 127, 255, 255); its .rg as the sampler returns them
constexpr float kDefaultNormalRG = 127.0f / 255.0f;

// What the shared functions read of a scene: SceneArgs' fields by the same names (the
// kernels fill one from their SceneArgs, the host from downloaded or caller-made arrays).
// T4: the texel type (float4 on the device).
template<class T4>
struct SceneView {
    const GpuTriangle* tris;
    const uint32_t* indices;
    const float* vertices; // RTVertex, 9 floats
    const ArkRTTriangleMesh* meshes;
    const ArkShaderMaterial* materials;
    const GpuInstance* instances;
    const GpuTextureInfo* tex_infos;
    const T4* texels;
    int32_t texture_count, white_texture, env_texture;
    int32_t has_sun, spot_count;
    float sun_color[3], sun_dir[3];
    const GpuSpotLight* spots;
};

template<class T4>
ARK_HD bool validTexture(const SceneView<T4>& sc, int idx) { return idx >= 0 && idx < sc.texture_count; }
// SceneArgs::sample: the 1 x 1 white default is not fetched
template<class T4>
ARK_HD T4 sample(const SceneView<T4>& sc, int idx, float u, float v)
{
    return dev::sampleOrWhite(sc.tex_infos, sc.texels, sc.texture_count, sc.white_texture, idx, u, v);
}

// ---- [1] random numbers (pathtracer/common.glsl:31-36, random.glsl:17-40) ----------------
// the value of the state BEFORE the xorshift step; float(state) rounds to nearest, so states
// >= 2^32 - 128 return exactly 1.0
ARK_HD float randomFloat(uint32_t& state)
{
    const float value = static_cast<float>(state) / 4294967296.0f;
    state = dev::rand_xorshift(state);
    return value;
}
ARK_HD uint32_t pixelSeed(uint32_t px, uint32_t py, uint32_t width, uint32_t height, uint32_t frameIndex)
{
    return dev::wang_hash((px + py * width) + frameIndex * (width * height)); // uint wrap-around
}

ARK_HD float lengthSquared(V3 v) { return dev::dot(v, v); }
ARK_HD float luminance(V3 c) { return dev::dot(c, v3(0.2126f, 0.7152f, 0.0722f)); }
ARK_HD V3 reflect(V3 I, V3 N) { return I - 2.0f * dev::dot(N, I) * N; }
ARK_HD V3 refract(V3 I, V3 N, float eta)
{
    const float k = 1.0f - eta * eta * (1.0f - dev::dot(N, I) * dev::dot(N, I));
    if (k < 0.0f) return dev::splat(0.0f);
    return eta * I - (eta * dev::dot(N, I) + sqrtf_(k)) * N;
}

// column-major GLSL mat4 * vec4, sums in index order
ARK_HD void mulVec4(const float* M, float x, float y, float z, float w, float* out)
{
    for (int i = 0; i < 4; ++i) out[i] = M[i] * x + M[4 + i] * y + M[8 + i] * z + M[12 + i] * w;
}

struct PathState {
    V3 attenuation, radiance;
    uint32_t rng;
};

// ---- [2] camera ray (pathtracer.rgen:23-40, :54-65) ---------------------------------------
// the jitter is added to pixel + 0.5, so sample positions span [0.5, 1.5) of the pixel
ARK_HD PathState cameraRay(uint32_t px, uint32_t py, uint32_t width, uint32_t height, uint32_t frameIndex, const float* worldFromView,
                           const float* viewFromProjection, V3* origin, V3* direction)
{
    PathState s;
    s.rng = pixelSeed(px, py, width, height, frameIndex);
    const float jx = randomFloat(s.rng);
    const float jy = randomFloat(s.rng);
    const float pcx = static_cast<float>(px) + 0.5f, pcy = static_cast<float>(py) + 0.5f;
    const float inU = (pcx + jx) / static_cast<float>(width), inV = (pcy + jy) / static_cast<float>(height);
    const float dx = inU * 2.0f - 1.0f, dy = inV * 2.0f - 1.0f;
    float o[4], t[4], d[4];
    mulVec4(worldFromView, 0.0f, 0.0f, 0.0f, 1.0f, o);
    mulVec4(viewFromProjection, dx, dy, 1.0f, 1.0f, t);
    const V3 dv = dev::normalize(v3(t[0] / t[3], t[1] / t[3], t[2] / t[3]));
    mulVec4(worldFromView, dv.x, dv.y, dv.z, 0.0f, d);
    *origin = v3(o[0], o[1], o[2]);
    *direction = v3(d[0], d[1], d[2]);
    s.attenuation = dev::splat(1.0f);
    s.radiance = dev::splat(0.0f);
    return s;
}

// the miss branch (pathtracer.rgen:72-77): radiance += attenuation * multiplier * environment
template<class T4>
ARK_HD V3 missRadiance(const SceneView<T4>& sc, V3 direction, float multiplier, V3 attenuation, V3 radiance)
{
    float u, v;
    dev::sphericalUvFromDirection(direction, &u, &v);
    const T4 c = sample(sc, sc.env_texture, u, v);
    const V3 environmentRadiance = multiplier * v3(c.x, c.y, c.z);
    return radiance + attenuation * environmentRadiance;
}

// ---- [3] the any-hit program (anyhit.rahit:17-40) -----------------------------------------
// called for candidates of the masked class only (the opaque class's instances carry the
// opaque flag; the blend class's hit group has no any-hit program of its own: GpuScene.cpp:
// 901-928); a material that is not BLEND_MODE_MASKED accepts without a fetch
template<class T4>
ARK_HD bool alphaAccept(const SceneView<T4>& sc, uint32_t inst, uint32_t prim, float u, float v)
{
    const GpuInstance& gi = sc.instances[inst];
    const ArkRTTriangleMesh mesh = sc.meshes[gi.rt_mesh_index];
    const ArkShaderMaterial& mat = sc.materials[mesh.material_index];
    if (mat.blend_mode != ARK_BLEND_MODE_MASKED) return true;
    const float bx = 1.0f - u - v, by = u, bz = v;
    float uv[2][3];
    for (int k = 0; k < 3; ++k) {
        const uint32_t idx = sc.indices[static_cast<size_t>(mesh.first_index) + 3u * prim + k];
        const float* vx = sc.vertices + (static_cast<size_t>(mesh.first_vertex) + idx) * 9;
        uv[0][k] = vx[0];
        uv[1][k] = vx[1];
    }
    const float uvx = uv[0][0] * bx + uv[0][1] * by + uv[0][2] * bz;
    const float uvy = uv[1][0] * bx + uv[1][1] * by + uv[1][2] * bz;
    const T4 c = sample(sc, mat.base_color, uvx, uvy);
    return !(c.w < mat.mask_cutoff);
}

// ---- [4] the surface of a hit (closesthit.rchit:113-154) ----------------------------------
struct Surface {
    V3 N, baseColor, emissive;
    float roughness, metallic, clearcoat, clearcoatRoughness;
    float alpha;    // baseColor.a * colorTint.a: the glass program's absorptionFactor [6]
    uint32_t glass; // the hit class selects the program: blend -> glass BRDF [3]
};

template<class T4>
ARK_HD Surface surfaceOf(const SceneView<T4>& sc, uint32_t tri, float hu, float hv, bool backface)
{
    const GpuTriangle& tr = sc.tris[tri];
    const uint32_t inst = f2u(tr.t2[1]);
    const uint32_t prim = f2u(tr.t2[2]);
    const GpuInstance& gi = sc.instances[inst];
    const ArkRTTriangleMesh mesh = sc.meshes[gi.rt_mesh_index];
    const ArkShaderMaterial& mat = sc.materials[mesh.material_index];
    const float bx = 1.0f - hu - hv, by = hu, bz = hv;
    const float* vx[3];
    for (int q = 0; q < 3; ++q) {
        const uint32_t idx = sc.indices[static_cast<size_t>(mesh.first_index) + 3u * prim + q];
        vx[q] = sc.vertices + (static_cast<size_t>(mesh.first_vertex) + idx) * 9;
    }
    const float uvx = vx[0][0] * bx + vx[1][0] * by + vx[2][0] * bz;
    const float uvy = vx[0][1] * bx + vx[1][1] * by + vx[2][1] * bz;
    V3 normal = dev::normalize(v3(vx[0][2], vx[0][3], vx[0][4]) * bx + v3(vx[1][2], vx[1][3], vx[1][4]) * by + v3(vx[2][2], vx[2][3], vx[2][4]) * bz);
    normal = backface ? -normal : normal;
    // the normal map, in object space (:131-140)
    float nx = kDefaultNormalRG, ny = kDefaultNormalRG;
    if (validTexture(sc, mat.normal_map)) {
        const T4 c = sample(sc, mat.normal_map, uvx, uvy);
        nx = c.x;
        ny = c.y;
    }
    const float tnx = nx * 2.0f - 1.0f, tny = ny * 2.0f - 1.0f;
    const float tnz = sqrtf_(dev::clampf(1.0f - (tnx * tnx + tny * tny), 0.0f, 1.0f));
    const V3 tangent = dev::normalize(v3(vx[0][5], vx[0][6], vx[0][7]) * bx + v3(vx[1][5], vx[1][6], vx[1][7]) * by + v3(vx[2][5], vx[2][6], vx[2][7]) * bz);
    const V3 bitangent = vx[0][8] * dev::cross(normal, tangent);
    normal = dev::normalize(tnx * tangent + tny * bitangent + tnz * normal);
    const float* M = gi.normal_matrix;
    const V3 Nw = { M[0] * normal.x + M[1] * normal.y + M[2] * normal.z, M[4] * normal.x + M[5] * normal.y + M[6] * normal.z,
                    M[8] * normal.x + M[9] * normal.y + M[10] * normal.z };
    Surface s;
    s.N = dev::normalize(Nw);
    T4 c = sample(sc, mat.base_color, uvx, uvy);
    s.baseColor = v3(c.x, c.y, c.z) * v3(mat.color_tint[0], mat.color_tint[1], mat.color_tint[2]);
    s.alpha = c.w * mat.color_tint[3];
    c = sample(sc, mat.emissive, uvx, uvy);
    s.emissive = v3(c.x, c.y, c.z) * v3(mat.emissive_factor[0], mat.emissive_factor[1], mat.emissive_factor[2]);
    c = sample(sc, mat.metallic_roughness, uvx, uvy);
    s.metallic = c.z * mat.metallic_factor;
    s.roughness = c.y * mat.roughness_factor;
    s.clearcoat = mat.clearcoat;
    s.clearcoatRoughness = mat.clearcoat_roughness;
    s.glass = gi.hit_mask == static_cast<int32_t>(ARK_RT_HIT_MASK_BLEND) ? 1u : 0u;
    return s;
}

// ---- [5] direct light (closesthit.rchit:62-109) -------------------------------------------
// brdf.glsl:70-89
ARK_HD V3 specularBRDF(V3 L, V3 V, V3 N, V3 baseColor, float roughness, float metallic)
{
    const V3 H = dev::normalize(L + V);
    const float NdotV = fabsf_(dev::dot(N, V)) + 1e-5f;
    const float NdotL = dev::clampf(dev::dot(N, L), 0.0f, 1.0f);
    const float NdotH = dev::clampf(dev::dot(N, H), 0.0f, 1.0f);
    const float LdotH = dev::clampf(dev::dot(L, H), 0.0f, 1.0f);
    const float a = dev::square(roughness);
    const V3 f0 = dev::mix3(dev::splat(dev::kDielectricReflectance), baseColor, metallic);
    const V3 F = dev::F_Schlick3(LdotH, f0);
    const float D = dev::D_GGX(NdotH, a);
    const float V_ = dev::V_SmithGGXCorrelated(NdotV, NdotL, a);
    return F * D * V_;
}
ARK_HD V3 evaluateBRDF(const Surface& s, V3 L, V3 V)
{
    if (s.glass) return specularBRDF(L, V, s.N, dev::splat(1.0f), s.roughness, 0.0f); // evaluateGlassBRDF (brdf.glsl:173-177)
    return dev::evaluateDefaultBRDF(L, V, s.N, s.baseColor, s.roughness, s.metallic, s.clearcoat, s.clearcoatRoughness);
}

// L of light l (the light's axis for spots too); the lights in order: the sun, then the spots
template<class T4>
ARK_HD V3 lightAxis(const SceneView<T4>& sc, uint32_t l)
{
    if (sc.has_sun && l == 0) return -dev::normalize(v3(sc.sun_dir[0], sc.sun_dir[1], sc.sun_dir[2]));
    const GpuSpotLight& sl = sc.spots[l - (sc.has_sun ? 1u : 0u)];
    return -dev::normalize(v3(sl.direction[0], sl.direction[1], sl.direction[2]));
}
// bit l: LdotN > 0, i.e. light l casts a shadow ray
template<class T4>
ARK_HD uint32_t litLights(const SceneView<T4>& sc, V3 N)
{
    uint32_t mask = 0;
    const uint32_t n = static_cast<uint32_t>(sc.has_sun ? 1 : 0) + static_cast<uint32_t>(sc.spot_count);
    for (uint32_t l = 0; l < n; ++l)
        if (dev::dot(lightAxis(sc, l), N) > 0.0f) mask |= 1u << l;
    return mask;
}
// traceShadowRay's ray (:31-49, :70, :89-93): from X, tmin kShadowTmin; !(tmax >= tmin) is not
// traced and lit
template<class T4>
ARK_HD void shadowRay(const SceneView<T4>& sc, float zFar, uint32_t l, V3 X, V3* dir, float* tmax)
{
    if (sc.has_sun && l == 0) {
        *dir = lightAxis(sc, 0u);
        *tmax = 2.0f * zFar;
        return;
    }
    const GpuSpotLight& sl = sc.spots[l - (sc.has_sun ? 1u : 0u)];
    const V3 toLight = v3(sl.position[0], sl.position[1], sl.position[2]) - X;
    const float distanceToLight = dev::length(toLight);
    *dir = toLight / distanceToLight;
    *tmax = distanceToLight - 0.001f;
}

// emissive + the analytic lights; occluded: bit 16 + l set when light l's shadow ray was hit
template<class T4>
ARK_HD V3 directRadiance(const SceneView<T4>& sc, const Surface& s, V3 rayDirection, V3 hitPoint, uint32_t occluded)
{
    const V3 V = -rayDirection;
    V3 radiance = s.emissive;
    uint32_t l = 0;
    if (sc.has_sun) {
        const V3 L = lightAxis(sc, 0u);
        const float LdotN = dev::dot(L, s.N);
        if (LdotN > 0.0f) {
            const float shadowFactor = (occluded >> (16u + l)) & 1u ? 0.0f : 1.0f;
            const V3 brdf = evaluateBRDF(s, L, V);
            const V3 directLight = v3(sc.sun_color[0], sc.sun_color[1], sc.sun_color[2]) * shadowFactor;
            radiance = radiance + brdf * LdotN * directLight;
        }
        l++;
    }
    for (int li = 0; li < sc.spot_count; ++li, ++l) {
        const GpuSpotLight& sl = sc.spots[li];
        const V3 sdir = v3(sl.direction[0], sl.direction[1], sl.direction[2]);
        const V3 L = -dev::normalize(sdir);
        const float LdotN = dev::dot(L, s.N);
        if (LdotN > 0.0f) {
            const V3 toLight = v3(sl.position[0], sl.position[1], sl.position[2]) - hitPoint;
            const float distanceToLight = dev::length(toLight);
            const V3 normalizedToLight = toLight / distanceToLight;
            const float shadowFactor = (occluded >> (16u + l)) & 1u ? 0.0f : 1.0f;
            const float distanceAttenuation = 1.0f / dev::square(distanceToLight);
            // evaluateIESLookupTable (lighting.glsl:20-39)
            const V3 lrd = -normalizedToLight;
            float iesValue = 0.0f;
            const float angleV = dev::dot(lrd, sdir);
            if (!(angleV <= 0.0f)) {
                const float hx = dev::dot(lrd, v3(sl.right[0], sl.right[1], sl.right[2]));
                const float hy = dev::dot(lrd, v3(sl.up[0], sl.up[1], sl.up[2]));
                const float angleH = atan2f_(hy, hx) + kPi;
                const float lx = acosf_(angleV) / (2.0f * sl.position[3]);
                const float ly = dev::clampf(angleH / kTwoPi, 0.0f, 1.0f);
                iesValue = sample(sc, sl.ies_texture, lx, ly).x;
            }
            const V3 brdf = evaluateBRDF(s, L, V);
            const V3 directLight = v3(sl.color[0], sl.color[1], sl.color[2]) * shadowFactor * distanceAttenuation * iesValue;
            radiance = radiance + brdf * LdotN * directLight;
        }
    }
    return radiance;
}

// ---- [6] scatter (pathtracer/material.glsl), tangent space --------------------------------
// brdf.glsl:99-119 (inversesqrt as 1 / sqrt)
ARK_HD V3 sampleGGXVNDF(V3 Ve, float alpha, float U1, float U2)
{
    const V3 Vh = dev::normalize(v3(alpha * Ve.x, alpha * Ve.y, Ve.z));
    const float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
    const V3 T1 = lensq > 0.0f ? v3(-Vh.y, Vh.x, 0.0f) * (1.0f / sqrtf_(lensq)) : v3(1.0f, 0.0f, 0.0f);
    const V3 T2 = dev::cross(Vh, T1);
    const float r = sqrtf_(U1);
    const float phi = 2.0f * kPi * U2;
    // (cosf_ and sinf_ apart, as k_refl_setup has them: sincosf_ through pointers to locals
    // leaves the quadrant switch as indexed stores to scratch)
    const float t1 = r * cosf_(phi);
    float t2 = r * sinf_(phi);
    const float s = 0.5f * (1.0f + Vh.z);
    t2 = (1.0f - s) * sqrtf_(1.0f - t1 * t1) + s * t2;
    const V3 Nh = t1 * T1 + t2 * T2 + sqrtf_(fmaxf_(0.0f, 1.0f - t1 * t1 - t2 * t2)) * Vh;
    return dev::normalize(v3(alpha * Nh.x, alpha * Nh.y, fmaxf_(0.0f, Nh.z)));
}
// brdf.glsl:32-35; its second parameter is named a2
ARK_HD float G1_GGX(float NdotV, float a2) { return (2.0f * NdotV) / (NdotV + sqrtf_(a2 + (1.0f - a2) * dev::square(NdotV))); }

// material.glsl:41-64: H = (V + L) / 2 is not normalised and G1_GGX is handed `a`, not a^2;
// the divisions by V.z and L.z are the shader's
ARK_HD V3 evaluateMicrofacet(float roughness, V3 V, V3 L, V3 F, float* pdf)
{
    if (L.z <= 0.0f) {
        *pdf = 0.0f;
        return dev::splat(0.0f);
    }
    const V3 H = (V + L) * 0.5f;
    const float a = dev::square(roughness);
    const float D = dev::D_GGX(H.z, fmaxf_(a, 1e-10f));
    const float G1 = G1_GGX(V.z, a);
    const float G2 = G1 * G1_GGX(L.z, a);
    const float D_v = G1 * fmaxf_(0.0f, V.z) * D / V.z;
    *pdf = D_v / (4.0f * V.z);
    return F * D * G2 / (4.0f * L.z * V.z);
}

// material.glsl:70-106
ARK_HD V3 evaluateOpaque(const Surface& m, V3 V, V3 L, V3 F, float* pdf)
{
    float PDF = 0.0f;
    V3 f = dev::splat(0.0f);
    const float reflectance = luminance(F);
    const float metalWeight = m.metallic;
    const float dielectricWeight = 1.0f - m.metallic;
    float diffuseReflectionProb = dielectricWeight * luminance(m.baseColor);
    float microfacetReflectionProb = reflectance;
    const float invTotalWeight = 1.0f / (diffuseReflectionProb + microfacetReflectionProb);
    diffuseReflectionProb *= invTotalWeight;
    microfacetReflectionProb *= invTotalWeight;
    const bool reflected = L.z * V.z > 0.0f;
    if (diffuseReflectionProb > 0.0f && reflected) {
        float lambertianPdf = 0.0f;
        V3 lambert = dev::splat(0.0f);
        if (!(L.z <= 0.0f)) { // evaluateLambertian (:30-39)
            lambertianPdf = L.z / kPi;
            lambert = m.baseColor * dev::splat(1.0f / kPi);
        }
        f = f + lambert * dielectricWeight;
        PDF += lambertianPdf * diffuseReflectionProb;
    }
    if (microfacetReflectionProb > 0.0f && reflected) {
        float microfacetPdf;
        const float microfacetWeight = dielectricWeight + metalWeight;
        f = f + evaluateMicrofacet(m.roughness, V, L, F, &microfacetPdf) * microfacetWeight;
        PDF += microfacetPdf * microfacetReflectionProb;
    }
    *pdf = PDF;
    return f * fabsf_(L.z);
}

ARK_HD V3 sampleCosineWeightedHemisphere(float r1, float r2)
{
    const float phi = 2.0f * kPi * r1;
    const float sqrtR2 = sqrtf_(r2);
    return v3(cosf_(phi) * sqrtR2, sinf_(phi) * sqrtR2, sqrtf_(1.0f - r2));
}

// A sampled direction L with the BRDF value f and the pdf (by value: out-pointers merged
// across the two programs become indexed scratch stores on the device)
struct Sample {
    V3 f, L;
    float pdf;
};
ARK_HD Sample noSample() { return { dev::splat(0.0f), dev::splat(0.0f), 0.0f }; }

// material.glsl:108-150; the draws in the shader's order per branch [1]
ARK_HD Sample sampleOpaque(uint32_t& rng, const Surface& m, V3 V)
{
    if (V.z <= 0.0f) return noSample();
    Sample r = noSample();
    const float r0 = randomFloat(rng);
    const bool isMetal = m.metallic > r0;
    const V3 f0 = dev::mix3(dev::splat(dev::kDielectricReflectance), m.baseColor, isMetal ? 1.0f : 0.0f);
    const V3 F = dev::F_Schlick3(V.z, f0);
    const float reflectance = luminance(F);
    const float r1 = randomFloat(rng);
    if (reflectance > r1) {
        const float r2 = randomFloat(rng);
        const float r3 = randomFloat(rng);
        const V3 H = sampleGGXVNDF(V, dev::square(m.roughness), r2, r3);
        r.L = reflect(-V, H);
    } else if (isMetal) {
        return noSample(); // absorbed
    } else {
        const float r2 = randomFloat(rng);
        const float r3 = randomFloat(rng);
        r.L = sampleCosineWeightedHemisphere(r2, r3);
    }
    r.f = evaluateOpaque(m, V, r.L, F, &r.pdf);
    return r;
}

// material.glsl:181-266. `payload.insideGlass != payload.insideGlass;` is a comparison whose
// result is dropped: insideGlass stays false, so eta is air / glass, a path is absorbed when
// absorptionFactor > r0, and the refraction weight is 1 - absorptionFactor
ARK_HD Sample sampleTranslucent(uint32_t& rng, const Surface& m, V3 V)
{
    if (V.z <= 0.0f) return noSample();
    V3 L;
    const float absorptionFactor = m.alpha;
    const float r0 = randomFloat(rng);
    const bool isAbsorbed = absorptionFactor > r0;
    const V3 F = dev::F_Schlick3(V.z, dev::splat(dev::kDielectricReflectance));
    const float reflectance = luminance(F);
    const float eta = kIorAir / kIorGlass;
    const float r1 = randomFloat(rng);
    const float r2 = randomFloat(rng);
    const V3 H = sampleGGXVNDF(V, dev::square(m.roughness), r1, r2);
    const V3 refracted = refract(-V, H, eta);
    const bool cantRefract = lengthSquared(refracted) < 1e-2f;
    const float r3 = randomFloat(rng);
    if (cantRefract || reflectance > r3) {
        L = reflect(-V, H);
    } else if (isAbsorbed) {
        return noSample();
    } else {
        L = refracted;
    }
    // evaluateTranslucentMicrofacetMaterial (:181-215)
    float PDF = 0.0f;
    V3 f = dev::splat(0.0f);
    float microfacetReflectionProb = reflectance;
    float refractionProb = (1.0f - microfacetReflectionProb) * (1.0f - absorptionFactor);
    const float invTotalWeight = 1.0f / (microfacetReflectionProb + refractionProb);
    microfacetReflectionProb *= invTotalWeight;
    refractionProb *= invTotalWeight;
    const bool reflected = L.z * V.z > 0.0f;
    if (microfacetReflectionProb > 0.0f && reflected) {
        float microfacetPdf;
        f = f + evaluateMicrofacet(m.roughness, V, L, F, &microfacetPdf);
        PDF += microfacetPdf * microfacetReflectionProb;
    }
    if (refractionProb > 0.0f) {
        f = f + dev::splat(1.0f) * (1.0f - absorptionFactor);
        PDF += refractionProb;
    }
    return { f * fabsf_(L.z), L, PDF };
}

// The scatter block of the hit program (closesthit.rchit:173-211). True: the path goes on
// along *scattered with the attenuation updated. False: [7] pdf <= 0 (a NaN pdf too), the
// attenuation is zero and the hit program has returned without writing hitT.
struct Scatter {
    bool alive;
    V3 attenuation, direction;
    uint32_t rng;
};
ARK_HD Scatter scatter(const Surface& s, V3 rayDirection, uint32_t rng, V3 attenuation)
{
    const float n[3] = { s.N.x, s.N.y, s.N.z };
    float b1[3], b2[3];
    rtshadow::orthonormalBasis(n, b1, b2); // common.glsl:91-98
    const V3 B1 = v3(b1[0], b1[1], b1[2]), B2 = v3(b2[0], b2[1], b2[2]);
    const V3 mv = -rayDirection;
    const V3 V = v3(dev::dot(B1, mv), dev::dot(B2, mv), dev::dot(s.N, mv)); // transpose(mat3(B1, B2, N)) * -dir
    const Sample r = s.glass ? sampleTranslucent(rng, s, V) : sampleOpaque(rng, s, V);
    if (!(r.pdf > 0.0f)) return { false, dev::splat(0.0f), dev::splat(0.0f), rng };
    return { true, attenuation * (r.f / r.pdf), B1 * r.L.x + B2 * r.L.y + s.N * r.L.z, rng };
}

// [8] the loop's condition for another segment after `segment` (0-based) has hit and scattered
ARK_HD bool goesOn(uint32_t segment, V3 attenuation) { return segment + 1u < kMaxSegments && lengthSquared(attenuation) > kAttenuationFloor; }

// [9] accumulate.comp:21-30 on one channel; the frame comes from the fp16 image
ARK_HD float accumulate(float accumulated, float thisFrame, uint32_t n) { return (accumulated * static_cast<float>(n) + thisFrame) / static_cast<float>(n + 1u); }

} // namespace pt
} // namespace ark
