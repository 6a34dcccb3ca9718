// ddgi_cover_map.hip — the device build of the sun's cover map (sun_cover_map.h, DESIGN.md
// §3) from the world BVHs' triangle records:
//   k_cover_prims   per record: the light-space box, the largest |coordinate| and the
//                   histogram of projected extents (one header, integer atomics)
//   (host)          the grid from the header (cover::chooseGrid)
//   k_cover_raster  per record: its cells topped (wTop) and, where it covers them, wCover;
//                   a triangle over more than kBigCells cells goes to a list instead
//   k_cover_big     one workgroup per listed triangle, its threads striding over its cells
//   k_cover_decode  the ordered words back to fp32, in place
// Every cell value is a maximum of ordered words (atomicMax), so the map does not depend on
// the order the triangles arrive in. No kernel waits on another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ddgi_kernels.h"
#include "sun_cover_map.h"

namespace ark {
namespace dev {

__global__ void __launch_bounds__(256) k_cover_prims(const GpuTriangle* __restrict__ rec, uint32_t records, LbvhFrame frame, cover::Header* __restrict__ hdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    float maxAbs = 0.0f;
    bool live = false;
    if (i < records) {
        float L[3][3];
        live = cover::recordLight(rec[i], frame.m, L, maxAbs);
        if (live) {
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(L[0][a], fminf(L[1][a], L[2][a]));
                hi[a] = fmaxf(L[0][a], fmaxf(L[1][a], L[2][a]));
            }
            atomicAdd(&hdr->hist[cover::extentBin(L)], 1u);
        } else {
            maxAbs = 0.0f;
        }
    }
    const uint64_t alive = __ballot(live);
    for (int m = 1; m < 64; m <<= 1) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], m, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m, 64));
        }
        maxAbs = fmaxf(maxAbs, __shfl_xor(maxAbs, m, 64));
    }
    if ((threadIdx.x & 63u) == 0u && alive) {
        atomicAdd(&hdr->prims, static_cast<uint32_t>(__popcll(alive)));
        for (int a = 0; a < 3; ++a) {
            atomicMin(&hdr->lo[a], lbvh::ordered(lo[a]));
            atomicMax(&hdr->hi[a], lbvh::ordered(hi[a]));
        }
        atomicMax(&hdr->maxAbs, __float_as_uint(maxAbs));
    }
}

// map: [ny][nx] texels of two ordered words (wCover, wTop); in bounds: setupTriangle clamps
// the cell range to the grid
__device__ __forceinline__ void coverCellMax(const cover::TriSetup& t, const cover::Grid& grid, uint32_t* __restrict__ map, int32_t cx, int32_t cy)
{
    uint32_t* texel = map + 2u * (static_cast<size_t>(cy) * grid.nx + static_cast<uint32_t>(cx));
    float topW, wc;
    const bool covers = cover::cellValues(t, grid, cx, cy, topW, wc);
    // (a plain read first: most arrivals do not raise the maximum)
    const uint32_t top = lbvh::ordered(topW);
    if (texel[1] < top) atomicMax(texel + 1, top);
    if (covers) {
        const uint32_t c = lbvh::ordered(wc);
        if (texel[0] < c) atomicMax(texel, c);
    }
}

struct CoverDir {
    float d[3];
};

__global__ void __launch_bounds__(256) k_cover_raster(const GpuTriangle* __restrict__ rec, uint32_t records, LbvhFrame frame, CoverDir dir, cover::Grid grid,
                                                      uint32_t* __restrict__ map, uint32_t* __restrict__ bigList, cover::Header* __restrict__ hdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= records) return;
    const GpuTriangle g = rec[i];
    float L[3][3], unused;
    if (!cover::recordLight(g, frame.m, L, unused)) return;
    cover::TriSetup t;
    const int kind = cover::setupTriangle(g, L, dir.d, grid, t);
    if (kind == cover::kTriSkip) return;
    if (kind == cover::kTriPoison) {
        atomicOr(&hdr->poison, 1u);
        return;
    }
    if (cover::cellCount(t) > cover::kBigCells) {
        bigList[atomicAdd(&hdr->big, 1u)] = i; // at most `records` entries: in bounds
        return;
    }
    for (int32_t cy = t.y0; cy <= t.y1; ++cy)
        for (int32_t cx = t.x0; cx <= t.x1; ++cx) coverCellMax(t, grid, map, cx, cy);
}

__global__ void __launch_bounds__(256) k_cover_big(const GpuTriangle* __restrict__ rec, LbvhFrame frame, CoverDir dir, cover::Grid grid, uint32_t* __restrict__ map,
                                                   const uint32_t* __restrict__ bigList, uint32_t bigCount)
{
    for (uint32_t b = blockIdx.x; b < bigCount; b += gridDim.x) {
        const GpuTriangle g = rec[bigList[b]];
        float L[3][3], unused;
        cover::recordLight(g, frame.m, L, unused);
        cover::TriSetup t;
        if (cover::setupTriangle(g, L, dir.d, grid, t) != cover::kTriOk) continue;
        const uint64_t w = static_cast<uint64_t>(t.x1 - t.x0 + 1), n = cover::cellCount(t);
        for (uint64_t c = threadIdx.x; c < n; c += 256u)
            coverCellMax(t, grid, map, t.x0 + static_cast<int32_t>(c % w), t.y0 + static_cast<int32_t>(c / w));
    }
}

__global__ void __launch_bounds__(256) k_cover_decode(uint32_t* __restrict__ map, uint64_t words)
{
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < words; i += static_cast<uint64_t>(gridDim.x) * 256ull)
        map[i] = __float_as_uint(lbvh::orderedFloat(map[i]));
}

} // namespace dev

hipError_t launch_cover_prims(const GpuTriangle* rec, uint32_t records, const double* frame, cover::Header* hdr, hipStream_t s)
{
    if (records == 0u) return hipSuccess;
    LbvhFrame f;
    for (int k = 0; k < 9; ++k) f.m[k] = frame[k];
    hipLaunchKernelGGL(dev::k_cover_prims, dim3((records + 255u) / 256u), dim3(256), 0, s, rec, records, f, hdr);
    return hipGetLastError();
}

hipError_t launch_cover_raster(const GpuTriangle* rec, uint32_t records, const double* frame, const float* dir, const cover::Grid& grid, uint32_t* map,
                               uint32_t* bigList, cover::Header* hdr, hipStream_t s)
{
    if (records == 0u) return hipSuccess;
    LbvhFrame f;
    for (int k = 0; k < 9; ++k) f.m[k] = frame[k];
    dev::CoverDir d { { dir[0], dir[1], dir[2] } };
    // -inf in ordered bits: below every value a triangle writes
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(map), static_cast<int>(lbvh::ordered(-INFINITY)), static_cast<size_t>(grid.nx) * grid.ny * 2u, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dev::k_cover_raster, dim3((records + 255u) / 256u), dim3(256), 0, s, rec, records, f, d, grid, map, bigList, hdr);
    return hipGetLastError();
}

hipError_t launch_cover_big(const GpuTriangle* rec, const double* frame, const float* dir, const cover::Grid& grid, uint32_t* map, const uint32_t* bigList,
                            uint32_t bigCount, hipStream_t s)
{
    LbvhFrame f;
    for (int k = 0; k < 9; ++k) f.m[k] = frame[k];
    dev::CoverDir d { { dir[0], dir[1], dir[2] } };
    if (bigCount != 0u) {
        hipLaunchKernelGGL(dev::k_cover_big, dim3(bigCount < 65536u ? bigCount : 65536u), dim3(256), 0, s, rec, f, d, grid, map, bigList, bigCount);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const uint64_t words = static_cast<uint64_t>(grid.nx) * grid.ny * 2u;
    hipLaunchKernelGGL(dev::k_cover_decode, dim3(static_cast<uint32_t>(std::min<uint64_t>((words + 255u) / 256u, 65536u))), dim3(256), 0, s, map, words);
    return hipGetLastError();
}

} // namespace ark
