// ddgi_refl_denoise.hip — the reflection denoiser passes of RTReflectionsNode
// (RTReflectionsNode.cpp:86-139) for gfx950: k_refl_history_copy (historyCopy.comp),
// k_refl_reproject, k_refl_prefilter and k_refl_resolve_temporal (the three compute shaders
// over the FidelityFX reflection denoiser headers). The arithmetic is refl_denoise.h's,
// shared with the host restatement (refl_denoise_host.cpp) and compared with it by bytes.
//
// Unit of work. The reference's 8 x 8 group is one wave64: a wave owns one tile, lane l is
// group thread (l & 7, l >> 3), and a 256-thread workgroup holds four tiles with LDS of
// their own. A tile's 16 x 16 apron is packed as the shaders pack it: two words per texel
// for reproject and resolve (2 KB per tile), four words and an fp32 depth for prefilter
// (5 KB per tile, 20 KB per workgroup), so LDS never limits occupancy. Each lane loads its
// four texels of the apron (RGBA16F as one 8-byte access) before any is stored. Lanes of a
// partial tile outside the image take part in the loads and the reduction and store
// nothing; a tile past the last one (the workgroup's padding) lies outside the image as a
// whole and stores nothing either, so every wave of a workgroup meets every barrier.
//
// reproject's 8 x 8 -> 1 reduction goes through the tile's LDS words at the shader's three
// levels, fp16 at each, 00 + 01 + 10 + 11.
#include <hip/hip_runtime.h>

#include "ddgi_kernels.h"
#include "refl_denoise.h"

namespace ark {
namespace dev {

namespace {

constexpr uint32_t kReflDenoiseBlock = 256, kTilesPerBlock = kReflDenoiseBlock / 64u;

struct TileLane {
    uint32_t wave, tileX, tileY;
    int gx, gy, px, py;
    bool tileInImage;
};
__device__ __forceinline__ TileLane tileLane(const refl::Args& a)
{
    TileLane t;
    const uint32_t lane = threadIdx.x & 63u;
    t.wave = threadIdx.x >> 6;
    const uint32_t tilesX = (a.width + 7u) / 8u, tilesY = (a.height + 7u) / 8u;
    const uint32_t tile = blockIdx.x * kTilesPerBlock + t.wave;
    t.tileX = tile % tilesX;
    t.tileY = tile / tilesX; // >= tilesY for the padding: py >= height
    t.tileInImage = t.tileY < tilesY;
    t.gx = static_cast<int>(lane & 7u);
    t.gy = static_cast<int>(lane >> 3);
    t.px = static_cast<int>(t.tileX * 8u) + t.gx;
    t.py = static_cast<int>(min(t.tileY, tilesY) * 8u) + t.gy;
    return t;
}

} // namespace

__global__ void __launch_bounds__(kReflDenoiseBlock) k_refl_history_copy(refl::Args a, int firstCopy)
{
    const uint64_t p = static_cast<uint64_t>(blockIdx.x) * kReflDenoiseBlock + threadIdx.x;
    if (p >= static_cast<uint64_t>(a.width) * a.height) return;
    refl::historyCopyPixel(a, static_cast<int>(p % a.width), static_cast<int>(p / a.width), firstCopy != 0);
}

__global__ void __launch_bounds__(kReflDenoiseBlock) k_refl_reproject(refl::Args a)
{
    __shared__ uint32_t s0[kTilesPerBlock][refl::kTileWords], s1[kTilesPerBlock][refl::kTileWords];
    const TileLane t = tileLane(a);
    uint32_t* t0 = s0[t.wave];
    uint32_t* t1 = s1[t.wave];
    refl::fillRadianceTile(a, t0, t1, t.px, t.py, t.gx, t.gy);
    __syncthreads();
    const refl::F4 part = refl::reprojectPixel(a, t0, t1, t.px, t.py, t.gx + 4, t.gy + 4);
    __syncthreads(); // every lane's 9 x 9 reads before the reduction overwrites the tile's corner
    refl::tileStore4(t0, t1, t.gx, t.gy, part);
    __syncthreads();
#pragma unroll
    for (int i = 2; i <= 8; i *= 2) {
        refl::reduceStep(t0, t1, t.gx, t.gy, i);
        __syncthreads();
    }
    if (t.gx == 0 && t.gy == 0 && t.tileInImage) refl::storeAverage(a, t0, t1, t.tileX, t.tileY);
}

__global__ void __launch_bounds__(kReflDenoiseBlock) k_refl_prefilter(refl::Args a)
{
    __shared__ uint32_t s0[kTilesPerBlock][refl::kTileWords], s1[kTilesPerBlock][refl::kTileWords], s2[kTilesPerBlock][refl::kTileWords],
        s3[kTilesPerBlock][refl::kTileWords];
    __shared__ float sd[kTilesPerBlock][refl::kTileWords];
    const TileLane t = tileLane(a);
    refl::fillPrefilterTile(a, s0[t.wave], s1[t.wave], s2[t.wave], s3[t.wave], sd[t.wave], t.px, t.py, t.gx, t.gy);
    __syncthreads();
    if (refl::inside(t.px, t.py, a.width, a.height))
        refl::prefilterPixel(a, s0[t.wave], s1[t.wave], s2[t.wave], s3[t.wave], sd[t.wave], t.px, t.py, t.gx + 4, t.gy + 4);
}

__global__ void __launch_bounds__(kReflDenoiseBlock) k_refl_resolve_temporal(refl::Args a)
{
    __shared__ uint32_t s0[kTilesPerBlock][refl::kTileWords], s1[kTilesPerBlock][refl::kTileWords];
    const TileLane t = tileLane(a);
    refl::fillRadianceTile(a, s0[t.wave], s1[t.wave], t.px, t.py, t.gx, t.gy);
    __syncthreads();
    if (refl::inside(t.px, t.py, a.width, a.height)) refl::resolveTemporalPixel(a, s0[t.wave], s1[t.wave], t.px, t.py, t.gx + 4, t.gy + 4);
}

} // namespace dev

// pass: 0 historyCopy (firstCopy), 1 reproject, 2 prefilter, 3 resolveTemporal, 4 historyCopy
hipError_t launch_refl_denoise_pass(const refl::Args& a, int pass, hipStream_t s)
{
    const uint64_t pixels = static_cast<uint64_t>(a.width) * a.height;
    if (pixels == 0) return hipSuccess;
    const uint64_t tiles = static_cast<uint64_t>((a.width + 7u) / 8u) * ((a.height + 7u) / 8u);
    const dim3 block(dev::kReflDenoiseBlock);
    const dim3 tileGrid(static_cast<uint32_t>((tiles + dev::kTilesPerBlock - 1u) / dev::kTilesPerBlock));
    const dim3 pixelGrid(static_cast<uint32_t>((pixels + dev::kReflDenoiseBlock - 1u) / dev::kReflDenoiseBlock));
    switch (pass) {
    case 0: hipLaunchKernelGGL(dev::k_refl_history_copy, pixelGrid, block, 0, s, a, 1); break;
    case 1: hipLaunchKernelGGL(dev::k_refl_reproject, tileGrid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(dev::k_refl_prefilter, tileGrid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(dev::k_refl_resolve_temporal, tileGrid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(dev::k_refl_history_copy, pixelGrid, block, 0, s, a, 0); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace ark
