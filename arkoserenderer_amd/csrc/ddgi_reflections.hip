// ddgi_reflections.hip — RT reflections ray generation (rt-reflections/raygen.rgen:54-166,
// WITH_DDGI) as a ray-list pipeline. Every step follows oracle/ddgi_oracle.cpp
// oracle_rt_reflections in the same operation order.
//
//   k_refl_setup      G-buffer decode + GGX VNDF sample per pixel (8 x 8 tiles):
//                     pixels that trace no ray are written here; the others append
//                     {origin, tmax}, {direction, pixel} to the ray list (one list
//                     atomic per 1,024 pixels)
//   k_trace<ListRays> persistent closest-hit traversal of the opaque class with the
//                     probe rays' ballot refill and dual steps
//   k_shadow_gen<true> + k_trace_shadow: the closest hit's shadow rays (both faces;
//                     the update's instances, launch_trace_shadow of ddgi_kernels.hip)
//   k_refl_shade      closest-hit program with the occluded bits, DDGI lookup,
//                     environment on a miss

#include <hip/hip_runtime.h>

#include "../../include/ark_ddgi.h"
#include "ddgi_device.h"
#include "ddgi_kernels.h"
#include "ddgi_sampling.h"
#include "ddgi_shading.h"
#include "ddgi_trace_kernels.h"

namespace ark {
namespace dev {

// k_trace's source (the Src contract: ddgi_trace_kernels.h). ListRays: a ray list of
// {origin, tmax}, {direction, id} (rt-reflections/raygen.rgen:111-119: RayFlags_Opaque,
// cullMask 0x01, tmin 0.01), f.list_count entries, the hit record at the list index.
struct ListRays {
    static constexpr bool kAllClasses = false;
    static constexpr bool kMaskedPass = false;
    static constexpr bool kSeeds = false;
    static constexpr float kTmin = 0.01f;
    __device__ static void grab(const FrameArgs& f, uint32_t home, uint32_t lane, uint32_t& tried, uint32_t& b, uint32_t& e, uint32_t chunk)
    {
        grabItemsWave(f.ray_counter, *f.list_count, home, lane, tried, b, e, chunk);
    }
    __device__ static PoolRec stage(const SceneArgs&, const FrameArgs& f, uint32_t r)
    {
        const float4 a = f.ray_list[2u * r], b = f.ray_list[2u * r + 1u];
        PoolRec rec;
        rec.o = { a.x, a.y, a.z };
        rec.d = { b.x, b.y, b.z };
        rec.a = __float_as_uint(a.w); // tmax
        rec.c = seed::kNone;
        return rec;
    }
    __device__ static void take(const FrameArgs& f, uint32_t r, uint32_t recA, uint32_t& ray, float& tmax)
    {
        ray = r;
        tmax = __uint_as_float(recA);
    }
};

// raygen.rgen:34-50 createIsotropicTBN: rows T, B, N (returned transposed)
struct ReflTBN {
    V3 T, B, N;
};

__device__ __forceinline__ ReflTBN reflIsotropicTBN(V3 N)
{
    V3 T;
    if (fabsf_(N.z) > 0.0f) {
        const float k = sqrtf_(N.y * N.y + N.z * N.z);
        T = v3(0.0f, -N.z / k, N.y / k);
    } else {
        const float k = sqrtf_(N.x * N.x + N.y * N.y);
        T = v3(N.y / k, -N.x / k, 0.0f);
    }
    return { T, cross(N, T), N };
}

// brdf.glsl:99-125 sampleGGXVNDF(Ve, alpha, alpha, U1, U2)
__device__ __forceinline__ V3 reflSampleGGXVNDF(V3 Ve, float alpha, float U1, float U2)
{
    const V3 Vh = normalize(v3(alpha * Ve.x, alpha * Ve.y, Ve.z));
    const float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
    const V3 T1 = lensq > 0.0f ? v3(-Vh.y, Vh.x, 0.0f) * (1.0f / sqrtf_(lensq)) : v3(1.0f, 0.0f, 0.0f);
    const V3 T2 = cross(Vh, T1);
    const float r = sqrtf_(U1);
    const float phi = 2.0f * kPi * U2;
    const float t1 = r * cosf_(phi);
    float t2 = r * sinf_(phi);
    const float s = 0.5f * (1.0f + Vh.z);
    t2 = (1.0f - s) * sqrtf_(1.0f - t1 * t1) + s * t2;
    const V3 Nh = t1 * T1 + t2 * T2 + sqrtf_(fmaxf_(0.0f, 1.0f - t1 * t1 - t2 * t2)) * Vh;
    return normalize(v3(alpha * Nh.x, alpha * Nh.y, fmaxf_(0.0f, Nh.z)));
}

// column-major GLSL mat4 products, sums in index order
__device__ __forceinline__ void reflMat4Mul(const float* A, const float* B, float* C)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r)
            C[c * 4 + r] = A[r] * B[c * 4] + A[4 + r] * B[c * 4 + 1] + A[8 + r] * B[c * 4 + 2] + A[12 + r] * B[c * 4 + 3];
}

__device__ __forceinline__ void reflMulPoint(const float* M, float x, float y, float z, float w, float* out)
{
    for (int i = 0; i < 4; ++i) out[i] = M[i] * x + M[4 + i] * y + M[8 + i] * z + M[12 + i] * w;
}

struct ReflSurface {
    V3 color, baseColor, normal;
    float metallic;
};

// opaque.rchit:105-176 on a front or back face (N flipped on a backface, :121-125);
// traceShadowRay's result for lit light l is bit 16 + l of `bits` (k_trace_shadow)
__device__ ReflSurface reflClosestHit(const SceneArgs& sc, const FrameArgs& f, V3 origin, V3 dir, const RayHit& hit, uint32_t bits)
{
    const GpuTriangle tr = loadTri(sc.tris, hit.tri);
    const uint32_t inst = __builtin_bit_cast(uint32_t, tr.t2[1]);
    const uint32_t prim = __builtin_bit_cast(uint32_t, tr.t2[2]);
    const GpuInstance gi = sc.instances[inst];
    const ArkRTTriangleMesh mesh = sc.meshes[gi.rt_mesh_index];
    const ArkShaderMaterial& mat = sc.materials[mesh.material_index];
    const float bx = 1.0f - hit.u - hit.v, by = hit.u, bz = hit.v;
    const float* vx[3];
    for (int q = 0; q < 3; ++q) {
        const uint32_t idx = sc.indices[static_cast<size_t>(mesh.first_index) + 3u * prim + q];
        vx[q] = sc.vertices + (static_cast<size_t>(mesh.first_vertex) + idx) * 9;
    }
    V3 N = normalize(v3(vx[0][2], vx[0][3], vx[0][4]) * bx + v3(vx[1][2], vx[1][3], vx[1][4]) * by + v3(vx[2][2], vx[2][3], vx[2][4]) * bz);
    N = hit.backface ? -N : N;
    const float* M = gi.normal_matrix;
    const V3 Nw = { M[0] * N.x + M[1] * N.y + M[2] * N.z, M[4] * N.x + M[5] * N.y + M[6] * N.z, M[8] * N.x + M[9] * N.y + M[10] * N.z };
    N = normalize(Nw);
    const float uvx = vx[0][0] * bx + vx[1][0] * by + vx[2][0] * bz;
    const float uvy = vx[0][1] * bx + vx[1][1] * by + vx[2][1] * bz;
    float4 c = sc.sample(mat.base_color, uvx, uvy);
    const V3 baseColor = v3(c.x, c.y, c.z) * v3(mat.color_tint[0], mat.color_tint[1], mat.color_tint[2]);
    c = sc.sample(mat.emissive, uvx, uvy);
    const V3 emissive = v3(c.x, c.y, c.z) * v3(mat.emissive_factor[0], mat.emissive_factor[1], mat.emissive_factor[2]);
    c = sc.sample(mat.metallic_roughness, uvx, uvy);
    const float metallic = c.z * mat.metallic_factor;
    const float roughness = c.y * mat.roughness_factor;
    const float clearcoat = mat.clearcoat, ccRough = mat.clearcoat_roughness;
    const V3 V = -dir;
    V3 color = emissive + f.ambient_amount * baseColor;
    const V3 hitPoint = origin + hit.t * dir; // rt_WorldRayOrigin + rt_RayHitT * rt_WorldRayDirection
    uint32_t l = 0;
    if (sc.has_sun) { // opaque.rchit:56-73
        const V3 L = -normalize(v3(sc.sun_dir[0], sc.sun_dir[1], sc.sun_dir[2]));
        const float LdotN = dot(L, N);
        if (LdotN > 0.0f) {
            const float shadowFactor = (bits >> (16u + l)) & 1u ? 0.0f : 1.0f;
            const V3 brdf = evaluateDefaultBRDF(L, V, N, baseColor, roughness, metallic, clearcoat, ccRough);
            const V3 directLight = v3(sc.sun_color[0], sc.sun_color[1], sc.sun_color[2]) * shadowFactor;
            color = color + brdf * LdotN * directLight;
        }
        l++;
    }
    for (int li = 0; li < sc.spot_count; ++li, ++l) { // opaque.rchit:75-103
        const GpuSpotLight sl = sc.spots[li];
        const V3 sdir = v3(sl.direction[0], sl.direction[1], sl.direction[2]);
        const V3 L = -normalize(sdir);
        const float LdotN = dot(L, N);
        if (LdotN > 0.0f) {
            const V3 toLight = v3(sl.position[0], sl.position[1], sl.position[2]) - hitPoint;
            const float distanceToLight = length(toLight);
            const V3 normalizedToLight = toLight / distanceToLight;
            const float shadowFactor = (bits >> (16u + l)) & 1u ? 0.0f : 1.0f;
            const float distanceAttenuation = 1.0f / square(distanceToLight);
            // evaluateIESLookupTable (lighting.glsl:20-39)
            const V3 lrd = -normalizedToLight;
            float iesValue = 0.0f;
            const float angleV = dot(lrd, sdir);
            if (!(angleV <= 0.0f)) {
                const float hx = dot(lrd, v3(sl.right[0], sl.right[1], sl.right[2]));
                const float hy = dot(lrd, v3(sl.up[0], sl.up[1], sl.up[2]));
                const float angleH = atan2f_(hy, hx) + kPi;
                const float lx = acosf_(angleV) / (2.0f * sl.position[3]);
                const float ly = clampf(angleH / kTwoPi, 0.0f, 1.0f);
                iesValue = sc.sample(sl.ies_texture, lx, ly).x;
            }
            const V3 brdf = evaluateDefaultBRDF(L, V, N, baseColor, roughness, metallic, clearcoat, ccRough);
            const V3 directLight = v3(sl.color[0], sl.color[1], sl.color[2]) * shadowFactor * distanceAttenuation * iesValue;
            color = color + brdf * LdotN * directLight;
        }
    }
    return { color, baseColor, N, metallic };
}

__device__ __forceinline__ void reflStore(uint16_t* out, uint32_t p, V3 c, float w)
{
    uint2 o;
    o.x = static_cast<uint32_t>(f32_to_f16(c.x)) | (static_cast<uint32_t>(f32_to_f16(c.y)) << 16);
    o.y = static_cast<uint32_t>(f32_to_f16(c.z)) | (static_cast<uint32_t>(f32_to_f16(w)) << 16);
    reinterpret_cast<uint2*>(out)[p] = o;
}

// One thread per pixel slot of the 8 x 8 tile order, kReflSetupSteps slots per
// thread; one list atomic per block.
constexpr uint32_t kReflSetupSteps = 4, kReflSetupSpan = kReflSetupSteps * 256u;

__global__ void __launch_bounds__(256) k_refl_setup(FrameArgs f, ArkReflectionsDesc r, float4* rayList, uint32_t* listCount)
{
    __shared__ uint32_t waveOff[kReflSetupSteps][4];
    __shared__ uint32_t blockBase;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float PW[16];
    reflMat4Mul(r.world_from_view, r.view_from_projection, PW); // camera.worldFromView * camera.viewFromProjection
    const uint32_t tilesX = (r.width + 7u) / 8u, tilesY = (r.height + 7u) / 8u;
    const uint64_t n = static_cast<uint64_t>(tilesX) * tilesY * 64u;
    V3 ro[kReflSetupSteps], rd[kReflSetupSteps];
    uint32_t pix[kReflSetupSteps];
#pragma unroll
    for (uint32_t k = 0; k < kReflSetupSteps; ++k) {
        pix[k] = kNoHit;
        const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kReflSetupSpan + k * 256u + threadIdx.x;
        if (i < n) {
            const uint32_t t = static_cast<uint32_t>(i >> 6), q = static_cast<uint32_t>(i & 63u);
            const uint32_t px = (t % tilesX) * 8u + (q & 7u), py = (t / tilesX) * 8u + (q >> 3);
            if (px < r.width && py < r.height) {
                const uint32_t p = py * r.width + px;
                const float pcx = static_cast<float>(px) + 0.5f, pcy = static_cast<float>(py) + 0.5f;
                const float inU = pcx / static_cast<float>(r.width), inV = pcy / static_cast<float>(r.height);
                const float nonLinearDepth = r.depth ? r.depth[p] : 0.0f;
                const uchar4 mp = r.material ? reinterpret_cast<const uchar4*>(r.material)[p] : make_uchar4(0, 0, 0, 0);
                const float roughness = static_cast<float>(mp.x) / 255.0f;
                if (nonLinearDepth >= 1.0f - 1e-6f) { // :60-64 (the direction image is not written)
                    reflStore(r.out_radiance, p, splat(0.0f), 0.0f);
                } else if (roughness >= r.no_tracing_roughness) { // :70-76
                    reflStore(r.out_radiance, p, splat(0.0f), 0.0f);
                    reflStore(r.out_direction, p, splat(0.0f), 0.0f);
                } else {
                    float nvx = 0.0f, nvy = 0.0f;
                    if (r.normal_velocity) {
                        const uint2 nw = reinterpret_cast<const uint2*>(r.normal_velocity)[p];
                        nvx = f16_to_f32(static_cast<uint16_t>(nw.x & 0xffffu));
                        nvy = f16_to_f32(static_cast<uint16_t>(nw.x >> 16));
                    }
                    const V3 viewSpaceNormal = octahedralDecode(nvx, nvy);
                    const float* Wv = r.world_from_view;
                    const V3 N = { Wv[0] * viewSpaceNormal.x + Wv[4] * viewSpaceNormal.y + Wv[8] * viewSpaceNormal.z,
                                   Wv[1] * viewSpaceNormal.x + Wv[5] * viewSpaceNormal.y + Wv[9] * viewSpaceNormal.z,
                                   Wv[2] * viewSpaceNormal.x + Wv[6] * viewSpaceNormal.y + Wv[10] * viewSpaceNormal.z };
                    float co[4], ct[4];
                    reflMulPoint(Wv, 0.0f, 0.0f, 0.0f, 1.0f, co);
                    reflMulPoint(PW, inU * 2.0f - 1.0f, inV * 2.0f - 1.0f, nonLinearDepth, 1.0f, ct);
                    const V3 target = v3(ct[0] / ct[3], ct[1] / ct[3], ct[2] / ct[3]);
                    const V3 viewRay = normalize(target - v3(co[0], co[1], co[2]));
                    float rx = 0.0f, ry = 0.0f;
                    if (r.blue_noise) {
                        const float* bn = r.blue_noise + 2 * (static_cast<size_t>(py % r.noise_height) * r.noise_width + px % r.noise_width);
                        rx = bn[0];
                        ry = bn[1];
                    }
                    const ReflTBN tbn = reflIsotropicTBN(N);
                    const V3 mv = -viewRay;
                    const V3 viewDirection = v3(dot(tbn.T, mv), dot(tbn.B, mv), dot(tbn.N, mv));
                    const V3 sampledNormal = reflSampleGGXVNDF(viewDirection, roughness * roughness, rx, ry);
                    const V3 I = -viewDirection;
                    const V3 reflected = I - 2.0f * dot(sampledNormal, I) * sampledNormal; // reflect(I, N)
                    ro[k] = target;
                    rd[k] = tbn.T * reflected.x + tbn.B * reflected.y + tbn.N * reflected.z;
                    pix[k] = p;
                }
            }
        }
    }
    // list positions in slot order: wave scans + one atomic per block
    uint32_t rank[kReflSetupSteps];
#pragma unroll
    for (uint32_t k = 0; k < kReflSetupSteps; ++k) {
        const uint64_t m = __ballot(pix[k] != kNoHit);
        rank[k] = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
        if (lane == 0) waveOff[k][wave] = static_cast<uint32_t>(__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < kReflSetupSteps; ++k)
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t c = waveOff[k][w];
                waveOff[k][w] = run;
                run += c;
            }
        blockBase = run ? atomicAdd(listCount, run) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kReflSetupSteps; ++k) {
        if (pix[k] == kNoHit) continue;
        const uint32_t j = blockBase + waveOff[k][wave] + rank[k];
        rayList[2u * j] = make_float4(ro[k].x, ro[k].y, ro[k].z, 10000.0f); // tmin 0.01, tmax 10000 (:117-119)
        rayList[2u * j + 1u] = make_float4(rd[k].x, rd[k].y, rd[k].z, __uint_as_float(pix[k]));
    }
}

// The closest-hit program (with the occluded bits of k_trace_shadow), the indirect
// diffuse term at the hit (:121-153) or the environment on a miss (:155-159).
__global__ void __launch_bounds__(256) k_refl_shade(SceneArgs sc, FrameArgs f, ArkReflectionsDesc r)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= *f.list_count) return;
    const float4 a = f.ray_list[2u * i], b = f.ray_list[2u * i + 1u];
    const V3 rayOrigin = v3(a.x, a.y, a.z), rayDirection = v3(b.x, b.y, b.z);
    const uint32_t p = __float_as_uint(b.w);
    const GpuHit gh = f.hits[i];
    float tmax = a.w;
    V3 radiance = splat(0.0f);
    if (gh.tri != kNoHit) { // payload.hitT <= tmax
        const RayHit hit { fabsf_(gh.t), gh.u, gh.v, gh.tri, 0u, 0u, gh.t < 0.0f };
        const uint32_t bits = f.light_count > 0 ? f.shadow_bits[i] : 0u;
        const ReflSurface s = reflClosestHit(sc, f, rayOrigin, rayDirection, hit, bits);
        tmax = gh.t; // signed: negative on a back face
        radiance = s.color;
        const V3 P = rayOrigin + tmax * rayDirection;
        const float hitMetallic = fminf_(s.metallic, 0.6f);
        const V3 irradiance = sampleDDGI<kGatherBatch>(f, P, s.normal, -rayDirection);
        const V3 indirectDiffuse = splat(1.0f - hitMetallic) * splat(1.0f - kDielectricReflectance) * irradiance;
        radiance = radiance + s.baseColor * indirectDiffuse;
    } else {
        // miss.rmiss:12 sets hitT = zFar + 1, which passes the raygen's
        // `payload.hitT <= tmax` test when zFar + 1 <= 10000: the ray length is then
        // zFar + 1 (deterministic), while the radiance the reference writes comes
        // from an unwritten payload (undefined); the environment stands in for it.
        float u, v;
        sphericalUvFromDirection(rayDirection, &u, &v);
        const float4 c = sc.sample(sc.env_texture, u, v);
        radiance = r.environment_multiplier * v3(c.x, c.y, c.z);
        const float missT = f.z_far + 1.0f;
        if (missT <= tmax) tmax = missT;
    }
    reflStore(r.out_radiance, p, radiance, tmax);
    reflStore(r.out_direction, p, rayDirection, 0.0f);
}

} // namespace dev

hipError_t launch_rt_reflections(const SceneArgs& sc, const FrameArgs& f, const ArkReflectionsDesc& r, uint32_t traceBlocks, uint32_t shadowBlocks,
                                 hipStream_t s)
{
    const uint64_t pixels = static_cast<uint64_t>(r.width) * r.height;
    const uint64_t slots = static_cast<uint64_t>((r.width + 7u) / 8u) * ((r.height + 7u) / 8u) * 64u;
    hipLaunchKernelGGL(dev::k_refl_setup, dim3(static_cast<uint32_t>((slots + dev::kReflSetupSpan - 1) / dev::kReflSetupSpan)), dim3(256), 0, s, f, r,
                       const_cast<float4*>(f.ray_list), const_cast<uint32_t*>(f.list_count));
    void* args[] = { const_cast<SceneArgs*>(&sc), const_cast<FrameArgs*>(&f) };
    hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&dev::k_trace<false, 6, dev::ListRays>), dim3(traceBlocks), dim3(kTraceBlock), args, 0, s);
    if (e != hipSuccess) return e;
    if (f.light_count > 0) {
        hipLaunchKernelGGL(dev::k_shadow_gen<true>, dim3(static_cast<uint32_t>((pixels + dev::kGenSpan - 1) / dev::kGenSpan)), dim3(256), 0, s, sc, f);
        e = launch_trace_shadow(sc, f, shadowBlocks, false, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dev::k_refl_shade, dim3(static_cast<uint32_t>((pixels + 255) / 256)), dim3(256), 0, s, sc, f, r);
    return hipGetLastError();
}

} // namespace ark
