// sun_cover_build.h — building the sun's cover map (sun_cover_map.h): the device build
// (ddgi_cover_map.hip's kernels, sequenced by sun_cover_map.cpp) and its host restatement.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device_bvh.h"
#include "sun_cover_map.h"

namespace ark {

// ddgi_cover_map.hip
hipError_t launch_cover_prims(const GpuTriangle* rec, uint32_t records, const double* frame, cover::Header* hdr, hipStream_t s);
hipError_t launch_cover_raster(const GpuTriangle* rec, uint32_t records, const double* frame, const float* dir, const cover::Grid& grid, uint32_t* map,
                               uint32_t* bigList, cover::Header* hdr, hipStream_t s);
// the listed large triangles, then the ordered words decoded to fp32
hipError_t launch_cover_big(const GpuTriangle* rec, const double* frame, const float* dir, const cover::Grid& grid, uint32_t* map, const uint32_t* bigList,
                            uint32_t bigCount, hipStream_t s);

// The shadow rays' direction -normalize(sunDir) as the kernels compute it in fp32
void sunRayDirection(const float sunDir[3], float L[3]);

// The map of `records` world-space records (holes skipped) for the frame (sun_frame) and
// direction of a sun, serially on the host: [ny][nx] texels (wCover, wTop). False: no map
// (cover::chooseGrid, or a poisoning triangle).
bool hostBuildCoverMap(const GpuTriangle* rec, uint64_t records, const double* frame, const float* dir, uint64_t budgetBytes, cover::Grid& grid,
                       std::vector<float>& map);

// The same on the device from records in device memory, on stream `s`, complete on return
// (two host reads of the header: the grid is chosen between the passes). ok false: no map.
hipError_t deviceBuildCoverMap(const GpuTriangle* devRec, uint64_t records, const double* frame, const float* dir, uint64_t budgetBytes, hipStream_t s,
                               cover::Grid& grid, DeviceBuffer& map, bool& ok);

} // namespace ark
