// ddgi_path_tracer.hip — the path tracer (PathTracerNode.cpp:81-103, pathtracer/pathtracer.rgen,
// closesthit.rchit, material.glsl, accumulate.comp) as a wavefront pipeline over a compacted
// list of live paths. The per-path arithmetic is path_tracer.h's, shared with the host
// restatement (path_tracer_host.cpp), in the same operation order.
//
//   k_pt_setup            per pixel slot of the 8 x 8 tile order: RNG seed, camera ray, path
//                         state; appends {origin, tmin}, {direction, slot} (one list atomic
//                         per workgroup)
//   per segment (16 times, launched by the host without a wait; the counts stay on the device):
//   k_trace<PathRays>     one closest hit over the opaque, masked and blend classes (tmax
//                         shrinks from class to class; the alpha test on masked-class
//                         candidates whose material is BLEND_MODE_MASKED)
//   k_pt_hit              a miss adds the environment and writes the pixel; a hit builds the
//                         surface (4 x 16 B), stores the lights with LdotN > 0 in the path's
//                         word and appends their shadow rays, owner = (list index << 4) | light
//   k_trace_shadow<kShadowPath>  any hit against opaque + masked (RayFlags_Opaque: no alpha
//                         test; blend geometry does not occlude): bit 16 + light
//   k_pt_shade            direct light, BRDF sample, attenuation and RNG; the path goes to the
//                         other list or its pixel is written
//   k_pt_accumulate       accumulate.comp, or the reset copy
//
// A path's state lives at its slot, not at its list position, and nothing is summed across
// paths: a pixel does not depend on the order of a list.

#include <hip/hip_runtime.h>

#include "../../include/ark_ddgi.h"
#include "ddgi_device.h"
#include "ddgi_kernels.h"
#include "ddgi_shading.h"
#include "ddgi_trace_kernels.h"
#include "path_tracer.h"

namespace ark {
namespace dev {

// k_trace's source (the Src contract: ddgi_trace_kernels.h).
// PathRays: the path tracer's list (pathtracer.rgen:42-50: RayFlags_None, cullMask opaque |
// masked | blend): {origin, tmin}, {direction, slot}, tmax zFar on every segment. One closest
// hit over the three classes: the lane walks the roots in turn and keeps its hit, so tmax
// shrinks from class to class and the tie rule holds across them; `pass` is the class, and
// class 1's candidates take the path tracer's alpha test. An empty list returns at once.
struct PathRays {
    static constexpr bool kAllClasses = true;
    static constexpr bool kMaskedPass = false;
    static constexpr bool kSeeds = false;
    static constexpr float kTmin = 0.0001f; // (each ray carries its own)
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
        rec.a = __float_as_uint(a.w); // tmin
        rec.c = seed::kNone;
        return rec;
    }
    __device__ static void take(const FrameArgs& f, uint32_t r, uint32_t, uint32_t& ray, float& tmax)
    {
        ray = r;
        tmax = f.z_far;
    }
};

__device__ __forceinline__ pt::SceneView<float4> ptView(const SceneArgs& sc)
{
    pt::SceneView<float4> v;
    v.tris = sc.tris;
    v.indices = sc.indices;
    v.vertices = sc.vertices;
    v.meshes = sc.meshes;
    v.materials = sc.materials;
    v.instances = sc.instances;
    v.tex_infos = sc.tex_infos;
    v.texels = sc.texels;
    v.texture_count = sc.texture_count;
    v.white_texture = sc.white_texture;
    v.env_texture = sc.env_texture;
    v.has_sun = sc.has_sun;
    v.spot_count = sc.spot_count;
    for (int k = 0; k < 3; ++k) {
        v.sun_color[k] = sc.sun_color[k];
        v.sun_dir[k] = sc.sun_dir[k];
    }
    v.spots = sc.spots;
    return v;
}

// anyhit.rahit for k_trace<PathRays> (travStepDual's PATH alpha test; declared in ddgi_traversal.h)
__device__ bool alphaAcceptPath(const SceneArgs& sc, uint32_t inst, uint32_t prim, float u, float v)
{
    return pt::alphaAccept(ptView(sc), inst, prim, u, v);
}

// the pixel of global slot g of the 8 x 8 tile order (kNoHit: outside the image)
__device__ __forceinline__ uint32_t ptPixelOf(const PtArgs& a, uint32_t g)
{
    const uint32_t tilesX = (a.width + 7u) / 8u;
    const uint32_t t = g >> 6, q = g & 63u;
    const uint32_t px = (t % tilesX) * 8u + (q & 7u), py = (t / tilesX) * 8u + (q >> 3);
    return px < a.width && py < a.height ? py * a.width + px : kNoHit;
}

// imageStore(pathTraceImage, vec4(radiance, 0)), RNE to fp16
__device__ __forceinline__ void ptWritePixel(const PtArgs& a, uint32_t slot, V3 radiance)
{
    const uint32_t p = ptPixelOf(a, a.slot0 + slot);
    uint2 o;
    o.x = static_cast<uint32_t>(f32_to_f16(radiance.x)) | (static_cast<uint32_t>(f32_to_f16(radiance.y)) << 16);
    o.y = static_cast<uint32_t>(f32_to_f16(radiance.z));
    reinterpret_cast<uint2*>(a.image)[p] = o;
}

// A block's appends to a list in thread order: `n` entries of this thread; returns the index
// of its first (one list atomic per workgroup).
__device__ __forceinline__ uint32_t ptBlockAppend(uint32_t n, uint32_t* count)
{
    __shared__ uint32_t waveTotal[4];
    __shared__ uint32_t blockBase;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t incl = waveInclusiveScan(n);
    if (lane == 63u) waveTotal[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t c = waveTotal[w];
            waveTotal[w] = run;
            run += c;
        }
        blockBase = run ? atomicAdd(count, run) : 0u;
    }
    __syncthreads();
    return blockBase + waveTotal[wave] + (incl - n);
}

__global__ void __launch_bounds__(256) k_pt_setup(PtArgs a, float4* __restrict__ list, uint32_t* count)
{
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = a.slot0 + slot;
    uint32_t p = kNoHit;
    if (g < a.slot1) p = ptPixelOf(a, g);
    V3 o = splat(0.0f), d = splat(0.0f);
    if (p != kNoHit) {
        const pt::PathState s = pt::cameraRay(p % a.width, p / a.width, a.width, a.height, a.frame_index, a.world_from_view, a.view_from_projection, &o, &d);
        a.state[2u * slot] = make_float4(s.attenuation.x, s.attenuation.y, s.attenuation.z, __uint_as_float(s.rng));
        a.state[2u * slot + 1u] = make_float4(s.radiance.x, s.radiance.y, s.radiance.z, 0.0f);
    }
    const uint32_t j = ptBlockAppend(p != kNoHit ? 1u : 0u, count);
    if (p != kNoHit) {
        list[2u * j] = make_float4(o.x, o.y, o.z, a.z_near); // tmin = zNear on the first segment
        list[2u * j + 1u] = make_float4(d.x, d.y, d.z, __uint_as_float(slot));
    }
}

__global__ void __launch_bounds__(256) k_pt_hit(SceneArgs sc, FrameArgs f, PtArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = *f.list_count;
    if (blockIdx.x * 256u >= n) return; // (whole workgroups: the append below has barriers)
    uint32_t lit = 0;
    V3 X = splat(0.0f);
    const pt::SceneView<float4> sv = ptView(sc);
    if (i < n) {
        const float4 ra = f.ray_list[2u * i], rb = f.ray_list[2u * i + 1u];
        const V3 origin = v3(ra.x, ra.y, ra.z), direction = v3(rb.x, rb.y, rb.z);
        const uint32_t slot = __float_as_uint(rb.w);
        const GpuHit gh = f.hits[i];
        if (gh.tri == kNoHit) {
            const float4 s0 = a.state[2u * slot], s1 = a.state[2u * slot + 1u];
            ptWritePixel(a, slot, pt::missRadiance(sv, direction, a.environment_multiplier, v3(s0.x, s0.y, s0.z), v3(s1.x, s1.y, s1.z)));
        } else {
            const pt::Surface s = pt::surfaceOf(sv, gh.tri, gh.u, gh.v, gh.t < 0.0f);
            float4* out = a.surf + 4u * static_cast<size_t>(i);
            out[0] = make_float4(s.N.x, s.N.y, s.N.z, s.roughness);
            out[1] = make_float4(s.baseColor.x, s.baseColor.y, s.baseColor.z, s.metallic);
            out[2] = make_float4(s.emissive.x, s.emissive.y, s.emissive.z, s.alpha);
            out[3] = make_float4(s.clearcoat, s.clearcoatRoughness, __uint_as_float(s.glass), 0.0f);
            lit = pt::litLights(sv, s.N);
            X = origin + fabsf_(gh.t) * direction; // rt_WorldRayOrigin + rt_RayHitT * rt_WorldRayDirection
        }
        f.shadow_bits[i] = lit;
    }
    uint32_t j = ptBlockAppend(static_cast<uint32_t>(__popc(lit)), f.shadow_count);
    for (uint32_t m = lit; m != 0; m &= m - 1u, ++j) {
        const uint32_t l = static_cast<uint32_t>(__builtin_ctz(m));
        V3 dir;
        float tmax;
        pt::shadowRay(sv, a.z_far, l, X, &dir, &tmax);
        f.shadow_rays[j] = ShadowRay { make_float4(X.x, X.y, X.z, tmax), make_float4(dir.x, dir.y, dir.z, __uint_as_float((i << 4) | l)) };
    }
}

__global__ void __launch_bounds__(256) k_pt_shade(SceneArgs sc, FrameArgs f, PtArgs a, uint32_t segment, float4* __restrict__ nextList, uint32_t* nextCount)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = *f.list_count;
    if (blockIdx.x * 256u >= n) return;
    bool goesOn = false;
    V3 nextOrigin = splat(0.0f), scattered = splat(0.0f);
    uint32_t slot = 0;
    if (i < n) {
        const GpuHit gh = f.hits[i];
        if (gh.tri != kNoHit) {
            const pt::SceneView<float4> sv = ptView(sc);
            const float4 ra = f.ray_list[2u * i], rb = f.ray_list[2u * i + 1u];
            const V3 origin = v3(ra.x, ra.y, ra.z), direction = v3(rb.x, rb.y, rb.z);
            slot = __float_as_uint(rb.w);
            const float4* in = a.surf + 4u * static_cast<size_t>(i);
            const float4 q0 = in[0], q1 = in[1], q2 = in[2], q3 = in[3];
            pt::Surface s;
            s.N = v3(q0.x, q0.y, q0.z);
            s.roughness = q0.w;
            s.baseColor = v3(q1.x, q1.y, q1.z);
            s.metallic = q1.w;
            s.emissive = v3(q2.x, q2.y, q2.z);
            s.alpha = q2.w;
            s.clearcoat = q3.x;
            s.clearcoatRoughness = q3.y;
            s.glass = __float_as_uint(q3.z);
            const float4 s0 = a.state[2u * slot], s1 = a.state[2u * slot + 1u];
            V3 attenuation = v3(s0.x, s0.y, s0.z), radiance = v3(s1.x, s1.y, s1.z);
            const float t = fabsf_(gh.t);
            const V3 X = origin + t * direction;
            radiance = radiance + attenuation * pt::directRadiance(sv, s, direction, X, f.shadow_bits[i]);
            const pt::Scatter sc2 = pt::scatter(s, direction, __float_as_uint(s0.w), attenuation);
            attenuation = sc2.attenuation;
            scattered = sc2.direction;
            if (!sc2.alive) {
                // the killed path: hitT stays tmax + 1, the raygen takes the miss branch
                ptWritePixel(a, slot, pt::missRadiance(sv, direction, a.environment_multiplier, attenuation, radiance));
            } else if (pt::goesOn(segment, attenuation)) {
                goesOn = true;
                nextOrigin = X; // ray.origin + abs(payload.hitT) * ray.direction
                a.state[2u * slot] = make_float4(attenuation.x, attenuation.y, attenuation.z, __uint_as_float(sc2.rng));
                a.state[2u * slot + 1u] = make_float4(radiance.x, radiance.y, radiance.z, 0.0f);
            } else {
                ptWritePixel(a, slot, radiance);
            }
        }
    }
    const uint32_t j = ptBlockAppend(goesOn ? 1u : 0u, nextCount);
    if (goesOn) {
        nextList[2u * j] = make_float4(nextOrigin.x, nextOrigin.y, nextOrigin.z, pt::kNextTmin);
        nextList[2u * j + 1u] = make_float4(scattered.x, scattered.y, scattered.z, __uint_as_float(slot));
    }
}

// accumulate.comp with frameCount = accumulated_frames, or copyTexture(pathTraceImage ->
// accumulation): the fp16 texel widened, alpha 0 included
__global__ void __launch_bounds__(256) k_pt_accumulate(PtArgs a)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= static_cast<uint64_t>(a.width) * a.height) return;
    const uint2 w = reinterpret_cast<const uint2*>(a.image)[p];
    const float r = f16_to_f32(static_cast<uint16_t>(w.x & 0xffffu)), g = f16_to_f32(static_cast<uint16_t>(w.x >> 16));
    const float b = f16_to_f32(static_cast<uint16_t>(w.y & 0xffffu)), al = f16_to_f32(static_cast<uint16_t>(w.y >> 16));
    float4* acc = reinterpret_cast<float4*>(a.accumulation) + p;
    if (a.flags & ARK_PATH_TRACER_RESET) {
        *acc = make_float4(r, g, b, al);
    } else {
        const float4 c = *acc;
        const uint32_t n = a.accumulated_frames;
        *acc = make_float4(pt::accumulate(c.x, r, n), pt::accumulate(c.y, g, n), pt::accumulate(c.z, b, n), 1.0f);
    }
}

} // namespace dev

// One batch of the path tracer (global slots [a.slot0, a.slot1) of the 8 x 8 tile order): the
// setup, then kMaxSegments times trace / hit / shadow trace / shade, each launch reading its
// list's count on the device. counters: kPtCounterWords words, zeroed by the caller on `s`
// before. The grids of the hit and shade stages cover the batch; a workgroup past the list
// returns at once.
hipError_t launch_path_trace_batch(const SceneArgs& sc, const FrameArgs& f0, const PtArgs& a, uint32_t* counters, uint32_t traceBlocks, uint32_t shadowBlocks,
                                   hipStream_t s, uint32_t segments)
{
    const uint32_t slots = a.slot1 - a.slot0;
    if (slots == 0 || (slots & 63u)) return hipErrorInvalidValue;
    const uint32_t blocks = (slots + 255u) / 256u;
    hipLaunchKernelGGL(dev::k_pt_setup, dim3(blocks), dim3(256), 0, s, a, a.lists[0], counters + kPtListCountWord);
    for (uint32_t seg = 0; seg < pt::kMaxSegments && seg < segments; ++seg) {
        FrameArgs f = f0;
        uint32_t* const own = counters + seg * kPtSegmentWords;
        f.ray_list = a.lists[seg & 1u];
        f.list_count = own + kPtListCountWord;
        f.ray_counter = own;
        f.shadow_count = own + kPtShadowCountWord;
        f.shadow_heads = own + kPtShadowHeadWord;
        void* args[] = { const_cast<SceneArgs*>(&sc), &f };
        hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&dev::k_trace<false, dev::kTraceWpe, dev::PathRays>), dim3(traceBlocks), dim3(kTraceBlock), args, 0, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(dev::k_pt_hit, dim3(blocks), dim3(256), 0, s, sc, f, a);
        if (f.light_count > 0) {
            e = hipLaunchKernel(reinterpret_cast<const void*>(&dev::k_trace_shadow<false, dev::kShadowWpe, dev::kShadowPath>), dim3(shadowBlocks), dim3(kTraceBlock), args, 0, s);
            if (e != hipSuccess) return e;
        }
        // (the last segment's survivors are written, never listed: goesOn)
        hipLaunchKernelGGL(dev::k_pt_shade, dim3(blocks), dim3(256), 0, s, sc, f, a, seg, a.lists[(seg + 1u) & 1u], own + kPtSegmentWords + kPtListCountWord);
    }
    return hipGetLastError();
}

hipError_t launch_path_trace_accumulate(const PtArgs& a, hipStream_t s)
{
    const uint64_t pixels = static_cast<uint64_t>(a.width) * a.height;
    if (pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_pt_accumulate, dim3(static_cast<uint32_t>((pixels + 255u) / 256u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace ark
