// ddgi_rt_shadows.hip — ray-traced local-light shadow masks (RTLocalShadowNode.cpp:47-90,
// rt-shadow/raygen.rgen:33-80) as a ray-list pipeline. The per-pixel arithmetic is
// rt_shadows.h's, shared with the host restatement (rt_shadows_host.cpp), in the same
// operation order.
//
//   k_rtshadow_gen      depth -> shading point -> disc sample -> per light of the batch the
//                       cone test; a light that needs a ray appends {origin, tmax},
//                       {direction, (pixel << 4) | light} (8 x 8 pixel tiles, one list
//                       atomic per 256 pixels; a tile's rays towards one light are
//                       contiguous). The pixel's result word: bit l = light l's ray is listed.
//   k_trace_shadow<kShadowOpaque>  persistent any-hit traversal of the opaque class only
//                       (cullMask RT_HIT_MASK_OPAQUE): an occluded ray sets bit 16 + l
//                       (the template of ddgi_trace_kernels.h, this mode instantiated here)
//   k_rtshadow_resolve  listed and not occluded -> 255, else 0 (sky, outside the cone,
//                       occluded), one byte per light and pixel
//
// Work set (ark_ddgi_rt_local_shadows): the lights of a call are traced in batches of
// consecutive lights whose worst-case ray lists (pixels x lights x 32 B) fit
// kRtShadowRayBudget = 512 MiB: one traversal launch per batch. 1920 x 1080 pixels take
// 63.3 MiB per light: up to 8 lights are one launch. A batch holds at least one light.

#include <hip/hip_runtime.h>

#include "../../include/ark_ddgi.h"
#include "ddgi_device.h"
#include "ddgi_kernels.h"
#include "ddgi_trace_kernels.h"
#include "rt_shadows.h"

namespace ark {
namespace dev {

__global__ void __launch_bounds__(256) k_rtshadow_gen(RtShadowArgs a, uint32_t l0, uint32_t l1, ShadowRay* __restrict__ list, uint32_t* listCount)
{
    __shared__ uint32_t waveOff[rtshadow::kMaxLights][4];
    __shared__ uint32_t blockBase;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    float PW[16];
    rtshadow::mat4Mul(a.world_from_view, a.view_from_projection, PW); // camera.worldFromView * camera.viewFromProjection
    const uint32_t tilesX = (a.width + 7u) / 8u, tilesY = (a.height + 7u) / 8u;
    const uint64_t n = static_cast<uint64_t>(tilesX) * tilesY * 64u;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    uint32_t p = kNoHit; // the pixel of this slot of the 8 x 8 tile order
    bool surface = false;
    float P[3] = { 0.0f, 0.0f, 0.0f }, diskX = 0.0f, diskY = 0.0f;
    if (i < n) {
        const uint32_t t = static_cast<uint32_t>(i >> 6), q = static_cast<uint32_t>(i & 63u);
        const uint32_t px = (t % tilesX) * 8u + (q & 7u), py = (t / tilesX) * 8u + (q >> 3);
        if (px < a.width && py < a.height) {
            p = py * a.width + px;
            const float nonLinearDepth = a.depth[p];
            if (!(nonLinearDepth >= rtshadow::kSkyDepth)) { // :38-40: sky keeps the clear value
                surface = true;
                rtshadow::shadingPoint(PW, px, py, a.width, a.height, nonLinearDepth, P);
                uint32_t state = rtshadow::pixelSeed(a.frame_index, px, py);
                rtshadow::pointInDisk(state, &diskX, &diskY);
            }
        }
    }
    // pass 1: which lights need a ray; counts per (light, wave)
    uint32_t listed = 0;
    for (uint32_t l = l0; l < l1; ++l) {
        bool need = false;
        if (surface) {
            float L[3], tmax;
            need = rtshadow::lightRay(P, a.lights[l], diskX, diskY, L, &tmax);
        }
        const uint64_t m = __ballot(need);
        if (lane == 0) waveOff[l - l0][wave] = static_cast<uint32_t>(__popcll(m));
        listed |= (need ? 1u : 0u) << l;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t l = 0; l < l1 - l0; ++l)
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t c = waveOff[l][w];
                waveOff[l][w] = run;
                run += c;
            }
        blockBase = run ? atomicAdd(listCount, run) : 0u;
    }
    __syncthreads();
    // the first batch zeroes the word (the occluded bits with it), later ones add their lights
    if (p != kNoHit) a.result[p] = (l0 == 0u ? 0u : a.result[p]) | listed;
    // pass 2: the rays in (light, tile, lane) order
    for (uint32_t l = l0; l < l1; ++l) {
        const bool need = (listed >> l) & 1u;
        const uint64_t m = __ballot(need);
        if (!need) continue;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
        float L[3], tmax;
        rtshadow::lightRay(P, a.lights[l], diskX, diskY, L, &tmax);
        const uint32_t j = blockBase + waveOff[l - l0][wave] + rank;
        list[j] = ShadowRay { make_float4(P[0], P[1], P[2], tmax), make_float4(L[0], L[1], L[2], __uint_as_float((p << 4) | l)) };
    }
}

// One thread per pixel: bit l (listed) and bit 16 + l (occluded) of the result word -> the
// byte of light l's mask.
__global__ void __launch_bounds__(256) k_rtshadow_resolve(RtShadowArgs a)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (p >= static_cast<uint64_t>(a.width) * a.height) return;
    const uint32_t w = a.result[p];
    for (uint32_t l = 0; l < a.light_count; ++l) {
        const bool lit = ((w >> l) & 1u) && !((w >> (16u + l)) & 1u);
        a.masks[l][p] = lit ? uint8_t(255) : uint8_t(0);
    }
}

} // namespace dev

// One batch of lights [l0, l1) of ark_ddgi_rt_local_shadows: the ray list, then its
// traversal through the opaque class (never the counting instantiation: the shadow
// counters stay the DDGI path's).
hipError_t launch_rt_shadow_batch(const SceneArgs& sc, const FrameArgs& f, const RtShadowArgs& a, uint32_t l0, uint32_t l1, uint32_t shadowBlocks, hipStream_t s)
{
    const uint64_t slots = static_cast<uint64_t>((a.width + 7u) / 8u) * ((a.height + 7u) / 8u) * 64u;
    if (slots == 0 || l0 >= l1 || l1 > rtshadow::kMaxLights) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_rtshadow_gen, dim3(static_cast<uint32_t>((slots + 255u) / 256u)), dim3(256), 0, s, a, l0, l1, f.shadow_rays, f.shadow_count);
    void* args[] = { const_cast<SceneArgs*>(&sc), const_cast<FrameArgs*>(&f) };
    return hipLaunchKernel(reinterpret_cast<const void*>(&dev::k_trace_shadow<false, dev::kShadowWpe, dev::kShadowOpaque>), dim3(shadowBlocks), dim3(kTraceBlock), args, 0, s);
}

hipError_t launch_rt_shadow_resolve(const RtShadowArgs& a, hipStream_t s)
{
    const uint64_t pixels = static_cast<uint64_t>(a.width) * a.height;
    if (pixels == 0 || a.light_count == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_rtshadow_resolve, dim3(static_cast<uint32_t>((pixels + 255u) / 256u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace ark
