// ddgi_shading.h — what the kernels that shade a hit share: the shading normal and the
// lit-light mask of a hit, its shadow rays (the sun's by the cover map where that decides),
// the front-hit surface and its shading (k_shade), and the shadow-ray generator
// k_shadow_gen<REFL> (REFL = false: the update, ddgi_kernels.hip; true: ddgi_reflections.hip).
#pragma once

#include "ddgi_sampling.h"
#include "ddgi_traversal.h"

namespace ark {
namespace dev {

// ---------------------------------------------------------------------------
// 1. a hit's normal, lit lights and shadow rays
// ---------------------------------------------------------------------------
// queue position -> slot (identity without an order table)
__device__ __forceinline__ uint32_t slotAt(const FrameArgs& f, uint32_t q)
{
    return f.slot_order ? f.slot_order[q] : q;
}

// opaque.rchit:118-131: world-space shading normal of a front hit. The trace
// kernel's shadow phase and the shading kernel both evaluate exactly this
// expression, so they agree on N (and on which lights need a shadow ray).
// hitShadingNormal from the triangle's shading record (a, b, c: n0 n1 n2) and its
// instance's normal matrix rows (m0, m1, m2), already read
__device__ __forceinline__ V3 shadingNormalOf(float4 a, float4 b, float4 c, float4 m0, float4 m1, float4 m2, float hu, float hv)
{
    const float bx = 1.0f - hu - hv, by = hu, bz = hv;
    // same operation sequence as k_shade (opaque.rchit:118-131)
    V3 N = normalize(v3(a.x, a.y, a.z) * bx + v3(a.w, b.x, b.y) * by + v3(b.z, b.w, c.x) * bz);
    V3 Nw = { m0.x * N.x + m0.y * N.y + m0.z * N.z, m1.x * N.x + m1.y * N.y + m1.z * N.z, m2.x * N.x + m2.y * N.y + m2.z * N.z };
    return normalize(Nw);
}

__device__ __forceinline__ V3 hitShadingNormal(const SceneArgs& sc, uint32_t tri, float hu, float hv)
{
    const float4* tn = sc.tri_normals + 4u * static_cast<size_t>(tri);
    const float4 a = tn[0], b = tn[1], c = tn[2];
    const uint32_t inst = __float_as_uint(c.y);
    const float* M = sc.instances[inst].normal_matrix;
    const float bx = 1.0f - hu - hv, by = hu, bz = hv;
    // same operation sequence as k_shade (opaque.rchit:118-131) and shadingNormalOf
    V3 N = normalize(v3(a.x, a.y, a.z) * bx + v3(a.w, b.x, b.y) * by + v3(b.z, b.w, c.x) * bz);
    V3 Nw = { M[0] * N.x + M[1] * N.y + M[2] * N.z, M[4] * N.x + M[5] * N.y + M[6] * N.z, M[8] * N.x + M[9] * N.y + M[10] * N.z };
    return normalize(Nw);
}

// opaque.rchit:56-103: lights with LdotN > 0 (bit l: sun first, then spots in order)
__device__ __forceinline__ uint32_t litLightMask(const SceneArgs& sc, V3 N)
{
    uint32_t need = 0, l = 0;
    if (sc.has_sun) {
        const V3 Ld = -normalize(v3(sc.sun_dir[0], sc.sun_dir[1], sc.sun_dir[2]));
        if (dot(Ld, N) > 0.0f) need |= 1u;
        l++;
    }
    for (int li = 0; li < sc.spot_count; ++li, ++l) {
        const V3 Ld = -normalize(v3(sc.spots[li].direction[0], sc.spots[li].direction[1], sc.spots[li].direction[2]));
        if (dot(Ld, N) > 0.0f) need |= 1u << l;
    }
    return need;
}

// Shadow ray of light l from hit point X (opaque.rchit:35-54 + :56-103): sun toward
// -sunDirection with tmax 2 zFar, spot toward its position with tmax distance - 0.001.
__device__ __forceinline__ void shadowRayOf(const SceneArgs& sc, float zFar, uint32_t l, V3 X, V3* dir, float* tmax)
{
    if (sc.has_sun && l == 0) {
        *dir = -normalize(v3(sc.sun_dir[0], sc.sun_dir[1], sc.sun_dir[2]));
        *tmax = 2.0f * zFar;
        return;
    }
    const GpuSpotLight& sl = sc.spots[l - (sc.has_sun ? 1u : 0u)];
    const V3 toLight = v3(sl.position[0], sl.position[1], sl.position[2]) - X;
    const float distanceToLight = length(toLight);
    *dir = toLight / distanceToLight;
    *tmax = distanceToLight - 0.001f;
}

__device__ __forceinline__ void rayOf(const FrameArgs& f, uint32_t ray, V3* origin, V3* dir)
{
    const uint32_t slot = ray / f.R, sample = ray - slot * f.R;
    const GpuProbeSlot ps = f.slots[slot];
    const float4 fb = f.fib[sample];
    *origin = { ps.pos[0], ps.pos[1], ps.pos[2] };
    *dir = rotate(v3(fb.x, fb.y, fb.z), v3(ps.axis[0], ps.axis[1], ps.axis[2]), ps.angle_sin, ps.angle_cos);
}

// The hit point of ray `ray` (hit distance t as recorded: negative for a back face): the
// origin of its shadow rays
template<bool REFL>
__device__ __forceinline__ V3 genHitPoint(const FrameArgs& f, uint32_t ray, float t)
{
    if (REFL) {
        const float4 a = f.ray_list[2u * ray], b = f.ray_list[2u * ray + 1u];
        const V3 origin = v3(a.x, a.y, a.z), dir = v3(b.x, b.y, b.z);
        return origin + fabsf_(t) * dir; // rt_RayHitT of a front or back face
    }
    V3 origin, dir;
    rayOf(f, ray, &origin, &dir);
    return origin + t * dir;
}

// The sun's shadow ray from X by the cover map (sun_cover_map.h): occluded, lit, or
// undecided - then it is listed and traced. Exact verdicts: every output stays what the
// traversal would give.
__device__ __forceinline__ int sunMapVerdict(const SceneArgs& sc, V3 X)
{
    const V3 pl = sunCoords(sc, X);
    const int64_t c = cover::cellIndex(sc.sun_grid, pl.x, pl.y);
    if (c < 0) return cover::kUndecided;
    const float2 t = sc.sun_map[c];
    return cover::verdict(pl.z, sc.map_lift, sc.map_reach, t.x, t.y);
}

// ---------------------------------------------------------------------------
// 2. front hits (k_shade)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void storeSurfel(const FrameArgs& f, uint32_t ray, V3 color, float dist)
{
    const uint32_t slot = ray / f.R, sample = ray - slot * f.R;
    uint2 packed;
    packed.x = static_cast<uint32_t>(f32_to_f16(color.x)) | (static_cast<uint32_t>(f32_to_f16(color.y)) << 16);
    packed.y = static_cast<uint32_t>(f32_to_f16(color.z)) | (static_cast<uint32_t>(f32_to_f16(dist)) << 16);
    reinterpret_cast<uint2*>(f.surfels)[static_cast<size_t>(slot) * f.Rmax + sample] = packed;
}

// A front hit's surface (opaque.rchit:105-131) and its lit lights: what the light loop and
// the indirect term of shadeFront need.
struct FrontSurface {
    V3 origin, dir, N, baseColor, base;
    float T, metallic, roughness, clearcoat, ccRough;
    uint32_t need; // lit lights (LdotN > 0), bit l: the sun first, then the spots in order
};

// SPOTS = false: the scene has no spot light (the sun-only schedule), their loops are left out.
template<bool SPOTS>
__device__ __forceinline__ void frontSurface(const SceneArgs& sc, const FrameArgs& f, const GpuSpotLight* spotsL, uint32_t ray, FrontSurface& sf)
{
    const GpuHit hit = f.hits[ray];
    rayOf(f, ray, &sf.origin, &sf.dir);
    sf.T = hit.t;
    // the triangle's shading record: vertex normals, instance, UVs
    const float4* rec = sc.tri_normals + 4u * static_cast<size_t>(hit.tri);
    const float4 ra = rec[0], rb = rec[1], rc = rec[2], rd = rec[3];
    const GpuInstance gi = sc.instances[__float_as_uint(rc.y)];
    const ArkShaderMaterial& mat = sc.materials[gi.material_index];
    const float bx = 1.0f - hit.u - hit.v, by = hit.u, bz = hit.v;
    // opaque.rchit:118-131 (front face: no flip)
    V3 N = normalize(v3(ra.x, ra.y, ra.z) * bx + v3(ra.w, rb.x, rb.y) * by + v3(rb.z, rb.w, rc.x) * bz);
    const float* M = gi.normal_matrix;
    V3 Nw = { M[0] * N.x + M[1] * N.y + M[2] * N.z, M[4] * N.x + M[5] * N.y + M[6] * N.z, M[8] * N.x + M[9] * N.y + M[10] * N.z };
    sf.N = N = normalize(Nw);
    const float uvx = rc.z * bx + rd.x * by + rd.z * bz;
    const float uvy = rc.w * bx + rd.y * by + rd.w * bz;
    float4 c = sc.sample(mat.base_color, uvx, uvy);
    sf.baseColor = v3(c.x, c.y, c.z) * v3(mat.color_tint[0], mat.color_tint[1], mat.color_tint[2]);
    c = sc.sample(mat.emissive, uvx, uvy);
    const V3 emissive = v3(c.x, c.y, c.z) * v3(mat.emissive_factor[0], mat.emissive_factor[1], mat.emissive_factor[2]);
    c = sc.sample(mat.metallic_roughness, uvx, uvy);
    sf.metallic = c.z * mat.metallic_factor;
    sf.roughness = c.y * mat.roughness_factor;
    sf.clearcoat = mat.clearcoat;
    sf.ccRough = mat.clearcoat_roughness;
    const V3 ambient = f.ambient_amount * sf.baseColor;
    sf.base = emissive + ambient;
    // lit lights (LdotN > 0): one shadow ray each (opaque.rchit:56-103)
    uint32_t need = 0, l = 0;
    if (sc.has_sun) {
        const V3 Ld = -normalize(v3(sc.sun_dir[0], sc.sun_dir[1], sc.sun_dir[2]));
        if (dot(Ld, N) > 0.0f) need |= 1u;
        l++;
    }
    for (int li = 0; SPOTS && li < sc.spot_count; ++li, ++l) {
        const V3 Ld = -normalize(v3(spotsL[li].direction[0], spotsL[li].direction[1], spotsL[li].direction[2]));
        if (dot(Ld, N) > 0.0f) need |= 1u << l;
    }
    sf.need = need;
}

// The lit lights' terms (occ: bit l set - light l is occluded), the indirect term and the
// surfel of a front hit: phase B of k_shade and its deferred pass run this one sequence.
template<bool SPOTS>
__device__ __forceinline__ void shadeFront(const SceneArgs& sc, const FrameArgs& f, const GpuSpotLight* spotsL, uint32_t ray, const FrontSurface& sf, uint32_t occ)
{
    const V3 origin = sf.origin, dir = sf.dir, N = sf.N, baseColor = sf.baseColor;
    const float T = sf.T, metallic = sf.metallic, roughness = sf.roughness, clearcoat = sf.clearcoat, ccRough = sf.ccRough;
    const uint32_t need = sf.need;
    V3 color = sf.base;
    const V3 V = -dir;
    const V3 hitPoint = origin + T * dir;
    uint32_t l = 0;
    if (sc.has_sun) { // opaque.rchit:56-73
        if (need & 1u) {
            const V3 Ld = -normalize(v3(sc.sun_dir[0], sc.sun_dir[1], sc.sun_dir[2]));
            const float LdotN = dot(Ld, N);
            const V3 brdf = evaluateDefaultBRDF(Ld, V, N, baseColor, roughness, metallic, clearcoat, ccRough);
            const V3 lc = v3(sc.sun_color[0], sc.sun_color[1], sc.sun_color[2]);
            const V3 tT = brdf * LdotN * (lc * 1.0f);
            const V3 tZ = brdf * LdotN * (lc * 0.0f);
            color = color + ((occ >> l) & 1u ? tZ : tT);
        }
        l++;
    }
    for (int li = 0; SPOTS && li < sc.spot_count; ++li, ++l) { // opaque.rchit:75-103
        if (!((need >> l) & 1u)) continue;
        const GpuSpotLight sl = spotsL[li];
        V3 sdir = v3(sl.direction[0], sl.direction[1], sl.direction[2]);
        V3 Ld = -normalize(sdir);
        float LdotN = dot(Ld, N);
        {
                V3 toLight = v3(sl.position[0], sl.position[1], sl.position[2]) - hitPoint;
                float distanceToLight = length(toLight);
                V3 normalizedToLight = toLight / distanceToLight;
                float distanceAttenuation = 1.0f / square(distanceToLight);
                // evaluateIESLookupTable (lighting.glsl:20-39)
                V3 lrd = -normalizedToLight;
                float iesValue = 0.0f;
                float angleV = dot(lrd, sdir);
                if (!(angleV <= 0.0f)) {
                    float hx = dot(lrd, v3(sl.right[0], sl.right[1], sl.right[2]));
                    float hy = dot(lrd, v3(sl.up[0], sl.up[1], sl.up[2]));
                    float angleH = atan2f_(hy, hx) + kPi;
                    float lx = acosf_(angleV) / (2.0f * sl.position[3]);
                    float ly = clampf(angleH / kTwoPi, 0.0f, 1.0f);
                    iesValue = sc.sample(sl.ies_texture, lx, ly).x;
                }
                V3 brdf = evaluateDefaultBRDF(Ld, V, N, baseColor, roughness, metallic, clearcoat, ccRough);
                V3 lc = v3(sl.color[0], sl.color[1], sl.color[2]);
                V3 tT = brdf * LdotN * (lc * 1.0f * distanceAttenuation * iesValue);
                V3 tZ = brdf * LdotN * (lc * 0.0f * distanceAttenuation * iesValue);
            color = color + ((occ >> l) & 1u ? tZ : tT);
        }
    }
    // raygen.rgen:125-127 + evaluateIndirectLightFromPreviousFrame (:94-106)
    const V3 Vi = -dir;
    const V3 F0 = mix3(splat(kDielectricReflectance), baseColor, metallic);
    const V3 F = F_Schlick3(fmaxf_(0.0f, dot(Vi, N)), F0);
    const V3 irradiance = sampleDDGI<kGatherBatch>(f, hitPoint, N, Vi);
    const V3 indirect = splat(1.0f - metallic) * (splat(1.0f) - F) * irradiance;
    const V3 bi = baseColor * indirect;
    storeSurfel(f, ray, color + bi, T);
}

// ---------------------------------------------------------------------------
// 3. the shadow-ray generator
// ---------------------------------------------------------------------------
// Shadow-ray list (the generator schedule: spots, no valid cover map, the reflections -
// shade_schedule.h; the sun-only schedule does this work inside k_shade and does not
// launch the generator): one thread per window ray in
// slot order; a front hit (raygen.rgen:121-127) stores its lit-light mask
// (opaque.rchit:56-103, LdotN > 0 with the shading normal) in shadow_bits[ray] and
// appends one shadow ray per lit light, owner = (ray << 4) | light. k_trace_shadow
// then sets the occluded bits 16 + light, and k_shade finishes every surfel
// in one pass (no per-light records, no finishing kernel).
// Block b owns the kGenSteps x 256 consecutive queue positions from b * kGenSpan:
// pass 1 stores the light masks (LDS + shadow_bits) and counts; one global atomic
// per block reserves the block's shadow rays (a per-wave atomic on the one list
// counter serialises at L2: 1.45 ms for 131K waves on C4); pass 2 writes them in
// position order (wave scans), so a shadow-kernel grab of 64 list entries holds the
// neighbouring rays of one probe. kGenSteps = 4 (16: 0.185 ms, 4: 0.163, 2: 0.215 at
// C4). Measured and removed: the list binned by light-space cell (-15 %
// shadow HBM, +34 % shadow phase) and a straight-line staged form (179 VGPRs, 0.416 ms).
constexpr uint32_t kGenSteps = 4, kGenSpan = kGenSteps * 256u;

__device__ __forceinline__ uint32_t waveInclusiveScan(uint32_t x)
{
    const uint32_t lane = __lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= static_cast<uint32_t>(off)) x += y;
    }
    return x;
}

// (genHitPoint and sunMapVerdict: §1, shared with k_shade, which resolves the sun's ray itself
// in the sun-only schedule)
// REFL: the reflection ray list (rt-reflections/raygen.rgen:122): queue position =
// list index, and the closest hit shades back faces too, with the normal flipped
// (opaque.rchit:121-125): N = -(shading normal), as negation commutes exactly with
// the normal matrix product and the normalisation.
template<bool REFL = false>
__global__ void __launch_bounds__(256) k_shadow_gen(SceneArgs sc, FrameArgs f)
{
    if (frameAborted(f.abort_word)) return;
    __shared__ uint32_t bitsL[kGenSpan];
    __shared__ uint32_t waveOff[kGenSteps][4];
    __shared__ uint32_t blockBase, sunBlockBase;
    // the sun's rays (light 0) to their own list when the scene has a light-space BVH
    const bool splitSun = !REFL && f.sun_rays != nullptr;
    const uint32_t total = REFL ? *f.list_count : f.window_rays;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t first = blockIdx.x * kGenSpan;
    if (REFL && first >= total) return; // launched for the largest possible list
    // pass 1 in stages over the thread's kGenSteps rays, so that each stage's
    // dependent loads (slot order -> hit -> triangle normals -> instance) are in
    // flight for all of them at once (the kernel is latency bound)
    uint32_t rays[kGenSteps];
    GpuHit hits[kGenSteps];
#pragma unroll
    for (uint32_t k = 0; k < kGenSteps; ++k) {
        const uint32_t pos = first + k * 256u + threadIdx.x;
        if (REFL) {
            rays[k] = pos < total ? pos : kNoHit;
        } else {
            const uint32_t q = pos / f.R;
            rays[k] = pos < total ? slotAt(f, q) * f.R + (pos - q * f.R) : kNoHit;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kGenSteps; ++k) {
        hits[k] = rays[k] != kNoHit ? f.hits[rays[k]] : GpuHit { 0.0f, 0.0f, 0.0f, kNoHit };
        if (!REFL && hits[k].t < 0.0f) hits[k].tri = kNoHit; // backface: no shading, no shadow ray
    }
    const bool useMap = sc.sun_map != nullptr; // (wave-uniform; set only with a sun: light 0)
    uint32_t nOccluded = 0, nLit = 0, nListed = 0;
#pragma unroll
    for (uint32_t k = 0; k < kGenSteps; ++k) {
        uint32_t bits = 0;
        int vd = cover::kUndecided;
        if (hits[k].tri != kNoHit) {
            V3 N = hitShadingNormal(sc, hits[k].tri, hits[k].u, hits[k].v);
            if (REFL && hits[k].t < 0.0f) N = -N;
            bits = litLightMask(sc, N);
            // the sun's ray (light 0) resolved from the cover map where its cell decides it:
            // occluded - bit 16 set here, as k_trace_shadow would - or lit; not listed then
            if (useMap && (bits & 1u)) {
                vd = sunMapVerdict(sc, genHitPoint<REFL>(f, rays[k], hits[k].t));
                f.shadow_bits[rays[k]] = bits | (vd == cover::kOccluded ? 1u << 16 : 0u);
                if (vd != cover::kUndecided) bits &= ~1u;
            } else {
                f.shadow_bits[rays[k]] = bits;
            }
        }
        bitsL[k * 256u + threadIdx.x] = bits;
        if (f.cover_counts && useMap) {
            nOccluded += static_cast<uint32_t>(__popcll(__ballot(vd == cover::kOccluded)));
            nLit += static_cast<uint32_t>(__popcll(__ballot(vd == cover::kLit)));
        }
        if (f.cover_counts) nListed += static_cast<uint32_t>(__popcll(__ballot(sc.has_sun && (bits & 1u))));
    }
    // counting updates (ark_ddgi_debug_sun_cover_counts): the sun's rays resolved and listed
    if (f.cover_counts && __lane_id() == 0u) {
        atomicAdd(&f.cover_counts[0], nOccluded);
        atomicAdd(&f.cover_counts[1], nLit);
        atomicAdd(&f.cover_counts[2], nListed);
    }
    // counts packed: world-list rays in bits 0-15, sun-list rays in bits 16-31 (a
    // block has at most kGenSpan x kMaxLights = 11,264 of either, no carry)
    auto packedCount = [&](uint32_t bits) {
        const uint32_t sun = splitSun ? (bits & 1u) : 0u;
        return static_cast<uint32_t>(__builtin_popcount(bits & ~sun)) | (sun << 16);
    };
#pragma unroll
    for (uint32_t k = 0; k < kGenSteps; ++k) {
        const uint32_t x = waveInclusiveScan(packedCount(bitsL[k * 256u + threadIdx.x]));
        if (__lane_id() == 63u) waveOff[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < kGenSteps; ++k)
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t c = waveOff[k][w];
                waveOff[k][w] = run;
                run += c;
            }
        blockBase = (run & 0xffffu) ? atomicAdd(f.shadow_count, run & 0xffffu) : 0u;
        sunBlockBase = (run >> 16) ? atomicAdd(f.sun_count, run >> 16) : 0u;
    }
    __syncthreads();
    for (uint32_t k = 0; k < kGenSteps; ++k) {
        const uint32_t bits = bitsL[k * 256u + threadIdx.x];
        const uint32_t c = packedCount(bits);
        const uint32_t before = waveOff[k][wave] + waveInclusiveScan(c) - c;
        uint32_t sj = blockBase + (before & 0xffffu);
        uint32_t sunj = sunBlockBase + (before >> 16);
        if (bits == 0) continue;
        const uint32_t pos = first + k * 256u + threadIdx.x;
        uint32_t ray;
        if (REFL) {
            ray = pos;
        } else {
            const uint32_t q = pos / f.R;
            ray = slotAt(f, q) * f.R + (pos - q * f.R);
        }
        const V3 hitPoint = genHitPoint<REFL>(f, ray, f.hits[ray].t);
        for (uint32_t b = bits; b; b &= b - 1) {
            const uint32_t l = static_cast<uint32_t>(__builtin_ctz(b));
            V3 ld;
            float tmax;
            shadowRayOf(sc, f.z_far, l, hitPoint, &ld, &tmax);
            const ShadowRay sr { make_float4(hitPoint.x, hitPoint.y, hitPoint.z, tmax), make_float4(ld.x, ld.y, ld.z, __uint_as_float((ray << 4) | l)) };
            if (splitSun && l == 0u) f.sun_rays[sunj++] = sr;
            else f.shadow_rays[sj++] = sr;
        }
    }
}

} // namespace dev
} // namespace ark
