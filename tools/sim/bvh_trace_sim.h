// bvh_trace_sim.h — host traversal simulator of the BVH8 (tools/lib/libark_bvhsim.so).
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Traversal statistics of that BVH8 on the host (a scalar simulation of k_trace's
 * closest-hit order: hit children, origin-containing first, then octant order; the
 * leaf triangles of a node right after it): nRays rays of 7 floats (origin,
 * direction, tmax) over `threads` host threads. out[9] = {node visits, triangle
 * tests, hits, BVH8 nodes, SAH cost x 1e6, max steps of one ray, max depth,
 * triangle records (leaf triangle rows, holes included), children the exact box
 * test accepts and the ARK_SIM_BOX form (kernel32 | f16) rejects (must be 0)};
 * per_ray_steps (if not NULL) gets each ray's node visits + triangle tests.
 * For comparing BVH builds (ARK_BVH8_COLLAPSE, ARK_BVH8_TRI_COST,
 * ARK_BVH_INTERSECTION_COST) without a GPU: tools/bvh_stats.py. */
int ark_ddgi_debug_bvh8_trace_stats(const float* triangles, uint64_t n, const float* rays, uint64_t n_rays, int threads, uint64_t* out,
                                    uint32_t* per_ray_steps /* nullable: node visits + triangle tests of each ray */);

/* k_trace's dual step (ARK_SIM_STEP=1) with its hit candidates (csrc/seed_cache.h), for
 * tuning the cache without a GPU (tools/seed_stats.py). `rays` holds `frames` blocks of n_rays
 * rays - the same probes' rays of consecutive updates - traced block by block over one BVH.
 * A ray's candidate is tested as its first pending triangle group. It comes from
 * `candidates` (nullable; first block only: a record index or 0xffffffff per ray), else
 * from a cache of `probes` rows of texels x texels words (row probe_of[ray], the texel of
 * the ray's direction) that takes every block's hits in ray order; texels 0: no cache.
 * frame_out[frames][8] = {node visits, triangle tests (the candidates' included), hits,
 * iterations, rays holding a candidate, candidates hit, 0, 0}; hit_records / hit_t (nullable,
 * [frames][n_rays]): each ray's closest hit's record (0xffffffff: miss) and distance;
 * out[9] as above with the blocks' sums and out[4] = iterations. Equal distances keep the
 * smaller primitive, so the hits do not depend on the candidates. */
int ark_ddgi_debug_bvh8_trace_seeded(const float* triangles, uint64_t n, const float* rays, uint64_t n_rays, uint32_t frames, const uint32_t* probe_of,
                                     uint32_t probes, uint32_t texels, const uint32_t* candidates, int threads, uint64_t* out, uint64_t* frame_out,
                                     uint32_t* hit_records, float* hit_t, uint32_t* per_ray_steps);

#ifdef __cplusplus
}
#endif
