// sun_bvh.h — the host build of the sun's light-space BVH8 and the sampled cost that
// decides between it and the world BVHs for the sun's shadow rays.
#pragma once

#include <stdint.h>
#include <vector>

#include "bvh_builder.h"

namespace ark {

// The sun's light-space BVH (k_trace_shadow<SUN>): every triangle of every hit-mask
// class in the frame (u, v, w = the shadow rays' direction L = -normalize(sun dir) as
// the kernels compute it in fp32), leaves holding the world-space records.
struct SunBvhInput {
    std::vector<BuildTriangle> tris;  // light-space vertices; primitive = index into world
    std::vector<GpuTriangle> world;   // world-space records (make_gpu_triangle)
    double frame[3][3] = {};          // rows u, v, w
    float maxAbs = 0.0f;              // largest |world coordinate|
    float inflateAbs = 0.0f;          // out (build_sun_bvh): the boxes' absolute inflation (the refit's floor)
};
// L = -normalize(sun_dir) in fp32, the kernels' normalize(): v * (1 / sqrt(dot(v, v))), dot left to right
void sun_ray_dir(const float sun_dir[3], float L[3]);
void sun_frame(const float sun_dir[3], double frame[3][3]);
void sun_add_triangles(SunBvhInput& in, const std::vector<BuildTriangle>& world_tris, int threads = 0);
// The same from world-space triangle records as the world BVHs hold them (holes skipped):
// the background rebuild after a sun-direction change or a refit (scene_rebuild.cpp hostBuildSun)
void sun_add_records(SunBvhInput& in, const std::vector<GpuTriangle>& records, int threads = 0);
// Builds the BVH2 (opt; its inflation replaced by the light-space bound), the BVH8
// (copt, slots sorted by w) and swaps in the world records; consumes in.tris and
// in.world. False when a BVH2 leaf exceeds kBvh8MaxLeafSize.
bool build_sun_bvh(SunBvhInput& in, const BvhBuildOptions& opt, const Bvh8CollapseOptions& copt, Bvh8BuildResult& out);
// Whether the light-space BVH pays for a scene: n sample sun shadow rays (points on
// triangles whose front face faces the sun, deterministic) traced any-hit on the host
// through both structures (exact decoded planes, tmin 0.025; frame == nullptr: the
// world BVHs and their roots, else the light frame with rays along +w), cost = node
// visits + triangle tests per ray - the persistent traversals' steps. Large
// axis-aligned surfaces (walls, a ground plane: C5's city block) become long slanted
// boxes in light space, where the world BVH culls them.
void sun_sample_origins(const std::vector<GpuTriangle>& tris, const float L[3], uint32_t n, std::vector<float>& out_xyz);
double sun_shadow_cost(const std::vector<GpuBvh8Node>& nodes, const std::vector<GpuTriangle>& tris, const int32_t* roots, int nRoots,
                       const double (*frame)[3], const float L[3], const std::vector<float>& origins_xyz);
// The light-space traversal has no LDS node cache, but its node test is a handful of
// byte compares: at C4's sampled ratio 0.948 it is the faster one (shadow phase 0.705 ->
// 0.669 ms, K = 2048 windows 1,384 -> 1,471 Mrays/s, profiles/r04_c_bench_step7/8), so
// it is chosen unless it saves less than 2 % of the sampled steps.
inline bool sun_bvh_pays(double costWorld, double costLight) { return costLight < 0.98 * costWorld; }

} // namespace ark
