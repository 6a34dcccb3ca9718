/*
 * ark_ddgi_debug.h — diagnostic entry points of libark_ddgi (not used by the
 * DDGI node). They exist so tests can pin the device side of the deterministic
 * math (ark_fmath.h) against the CPU side bit for bit.
 */
#ifndef ARK_DDGI_DEBUG_H
#define ARK_DDGI_DEBUG_H

#include <stdint.h>

#include "ark_ddgi.h" /* the skin entries' structs */

#ifdef __cplusplus
extern "C" {
#endif

/* Extra resource id for ark_ddgi_read: the primary-pass hit records of the last
 * update, 16 B each ({float t (negative = backface, +inf = miss), u, v, uint32
 * leaf-order triangle}) at slot * rays_per_probe + sample (slot = window slot,
 * sample = the ray's Fibonacci sample index). */
#define ARK_DDGI_DEBUG_HITS 100

/* Extra resource id for ark_ddgi_read: the traversal iterations (both passes) of
 * every probe ray of the last counting update (ark_ddgi_set_counting), uint16 at
 * the ray's hit-record index (slot * rays_per_probe + sample), saturating at 65535;
 * sized max_probe_updates x max_rays_per_probe. For the launch-tail analysis
 * (tools/ray_cost.py); counting is enabled first. */
#define ARK_DDGI_DEBUG_RAY_STEPS 101

/* Extra resource id for ark_ddgi_read: the light words of the last update or debug shade, one
 * uint32 per window ray indexed like ARK_DDGI_DEBUG_HITS (slot * rays_per_probe + sample),
 * sized max_probe_updates x max_rays_per_probe: the front hit's lit lights (LdotN > 0) in bits
 * 0-15 - the sun first, then the spots in order - and the lights whose shadow ray was occluded
 * in bits 16-31. Written for front hits only (a miss's or a back face's word keeps what an
 * earlier frame left), and only when the context has lights. The schedule with the shadow-ray
 * generator writes every front hit's word. The sun-only schedule writes every front hit's word
 * only in its counting variant (ark_ddgi_set_counting); without counting it writes the words of
 * the rays its cover map left undecided and no others. Before a scene is set: an error. */
#define ARK_DDGI_DEBUG_SHADOW_BITS 102

/* Evaluates op (0 sin, 1 cos, 2 acos, 3 atan2(x,y), 4 log2, 5 exp2, 6 pow(x,y),
 * 7 fp32->fp16->fp32 round trip, 8 powf_pos_(x,y)) on `device` for n inputs (host arrays). */
int ark_ddgi_debug_fmath(int device, int op, const float* x, const float* y, float* out, uint64_t n);

/* Host-side evaluation of the same functions (for comparison with the device). */
int ark_ddgi_debug_fmath_host(int op, const float* x, const float* y, float* out, uint64_t n);

/* sizeof() of the ABI structs, in this order: ArkDdgiDesc, ArkRTVertex,
 * ArkRTTriangleMesh, ArkShaderMaterial, ArkTexture, ArkRTInstance,
 * ArkDirectionalLight, ArkSpotLight, ArkDdgiScene, ArkDdgiFrameParams,
 * ArkDdgiCounters, ArkDdgiDeviceViews, ArkDdgiBvhStats. Returns the count written. */
int ark_ddgi_debug_struct_sizes(uint32_t* out, int n);

/* Builds the BVH used by ark_ddgi_set_scene (binned-SAH BVH2 with leaves of at most
 * 3 triangles, collapsed into 8-wide quantized nodes) over n world-space triangles
 * (9 floats each) on the host and checks it: every triangle in exactly one leaf,
 * every quantized plane exactly representable, every triangle vertex inside the
 * decoded boxes of its leaf and of all its ancestors. out[8] = {nodes, leaf
 * children, max depth, violations, triangles, bvh2 nodes, internal children, BVH8
 * SAH cost x 1e6 (node cost 1)}. The BVH8 child selection is set_scene's (SAH-optimal
 * collapse, default triangle cost); _opts selects the greedy collapse (sah_optimal 0)
 * or another triangle cost (tri_cost > 0), for comparing builds.
 * Returns 0 when the check passes, 1 when it found violations. No GPU. */
int ark_ddgi_debug_bvh8_check(const float* triangles, uint64_t n, uint64_t* out);
int ark_ddgi_debug_bvh8_check_opts(const float* triangles, uint64_t n, int sah_optimal, float tri_cost, uint64_t* out);

/* The host traversal simulator (ark_ddgi_debug_bvh8_trace_stats) is a tool, not part
 * of this library: tools/sim/bvh_trace_sim.h, tools/lib/libark_bvhsim.so. */

/* The sun's light-space BVH (the one set_scene builds for k_trace_shadow<SUN>) built
 * on the host from n world triangles (9 floats each) and checked without a GPU: a sun
 * shadow ray from each of n_rays origins (3 floats) along L = -normalize(sun_dir),
 * [0.025, tmax], any hit through the BVH with a host restatement of the kernel's
 * light-space node test, and against every triangle. out[8] = {rays, occluded (brute
 * force), occluded (BVH), mismatches, node visits, triangle tests, BVH8 nodes, max
 * stack depth}. Returns 0 when no ray differs, 2 on a mismatch, 1 on a build error. */
int ark_ddgi_debug_sun_bvh_check(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                 uint64_t* out);

/* set_scene's choice of structure for the sun's shadow rays (scene_build.cpp,
 * ArkDdgiDesc.sun_bvh = ARK_DDGI_SUN_BVH_AUTO): the world BVH8 and the light-space BVH8 of the triangles are built, sample
 * sun shadow rays from sun-facing points traced any-hit through both on the host;
 * out[4] = {world steps per ray, light-space steps per ray, 1 if the light-space BVH
 * is chosen, samples}. No GPU. */
int ark_ddgi_debug_sun_choice(const float* triangles, uint64_t n, const float* sun_dir, uint32_t n_samples, double* out);

/* FNV-1a 64 digests of the geometry the context's kernels read now (the front copy,
 * after everything it enqueued): out[4] = {world BVH8 nodes, world triangle records,
 * light-space sun BVH8 nodes, its records} (the sun's 0 without one). For the refit
 * tests: refits that reach only the nodes of moved instances leave the same bytes as
 * one that reaches every node. Synchronous. */
int ark_ddgi_debug_scene_digest(struct ArkDdgiCtx* ctx, uint64_t* out);

/* The device LBVH build of the world BVH8s (ARK_DDGI_FLAG_GPU_REBUILD) run serially on
 * the host over n world triangles (9 floats each), with the very functions the kernels
 * call (csrc/lbvh_build.h): Morton keys, the radix tree, the BVH2 -> BVH8 cut, slots and
 * private rows; the boxes from the records upward and the planes by the host collapse's
 * node writer. The checks and out[8] are ark_ddgi_debug_bvh8_check's (out[5]: the radix
 * tree's nodes, 2 n - 1); also: the nodes are one contiguous range, each depth's one
 * range behind the depth above's, and every record is the input's bit for bit. _opts: the member a cut opens next (0 the
 * one of most triangles, 1 the one of the largest Morton cell area - the default).
 * Returns 0 when the check passes, 1 when it found violations. No GPU. */
int ark_ddgi_debug_lbvh_check(const float* triangles, uint64_t n, uint64_t* out);
int ark_ddgi_debug_lbvh_check_opts(const float* triangles, uint64_t n, int criterion, uint64_t* out);
/* The same with the SAH pass of ARK_DDGI_FLAG_GPU_REBUILD_SAH restated serially between the
 * radix tree and the cut (sah != 0; the cut then opens by the pass's boxes whatever
 * `criterion`; sah = 0: _opts' result word for word). out[9]: _opts' eight, [8] the treelets
 * the pass rebuilt. */
int ark_ddgi_debug_lbvh_check_sah(const float* triangles, uint64_t n, int criterion, int sah, uint64_t* out);
/* The same with the collapse plan of ARK_DDGI_FLAG_GPU_REBUILD_PLAN (plan != 0; it does nothing
 * unless sah != 0): the treelets down to single primitives, the plans, and the cut by their
 * picks. plan = 0: _sah's result word for word. out[11]: _sah's nine, [9] the plan's cost of
 * the root as one BVH8 node (the fp32 word; 0 without the plan or for a root of at most three
 * triangles), [10] the BVH8 nodes other than the root with at most three triangles below them
 * (0 expected; counted from the finished tree in either mode; with the plan they fail the check). */
int ark_ddgi_debug_lbvh_check_plan(const float* triangles, uint64_t n, int criterion, int sah, int plan, uint64_t* out);

/* The device LBVH build itself (ARK_DDGI_FLAG_GPU_REBUILD, ARK_DDGI_FLAG_GPU_REBUILD_SUN: the
 * product's driver and kernels, nothing else) run once on `device`, synchronously and without
 * a context, over n_records 48-byte triangle records as a snapshot holds them (holes -
 * instance 0xffffffff - included), and compared bit for bit with the host restatement
 * (ark_ddgi_debug_lbvh_check's) of the same records. class_of[n_instances]: instance -> hit-mask
 * class 0..2. sun_dir null: the world build; set: the light build in sun_frame's frame with
 * slots in ascending w, w_bits of the key's Morton bits for w (negative: the default; the
 * world build ignores it). The device's compaction order of the records comes from atomics;
 * it is checked to be a permutation of exactly the records that are not holes and handed to
 * the host restatement, which makes every later stage comparable, ties included. out[32]:
 * [0] primitives, [1] nodes, [2] records with holes, [3] depth (of the device build), [4] the
 * reason the device left the scene to the host (0 none, 1 no records, 2 no triangles, 3 a
 * record of an unknown instance, 4 too deep, 5 node scratch, 6 4 GiB, 7 another), then the
 * mismatch counts: [5] compaction not that permutation, [6] light build: a wave's survivors
 * not one ascending run, [7] header counts and error word, [8] header box (compared with ==
 * as floats), [9] largest |coordinate| bits, [10] inflation bits, [11] sorted keys, [12]
 * sorted record indices, [13] splits (every internal index of every class range), and the
 * trees in canonical form (walked from each root in slot order, internal children by rank):
 * [14] shape (roots, opaqueNodes, depth, nodes per depth, counts), [15] imask / leaf_mask /
 * leaf_tris / tri_stride, [16] p and e, [17] qlo / qhi bytes of occupied slots, [18] child
 * indices, [19] records of leaf slots (48 bytes, row by row), [20] their perm entries, [21]
 * row positions that are not holes, [22] the level order against the one recomputed from the
 * nodes, [23] the padding record not all zero; [24], [25] the first differing node pair
 * (device, host; ~0: none), [26] the HIP error, [27] node pairs visited, [28] host nodes.
 * Returns 0 when every count is 0, 1 on a mismatch, 2 when the device left the scene to the
 * host ([4]; nothing built, nothing compared), negative on an invalid argument or a HIP error. */
int ark_ddgi_debug_lbvh_device_parity(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                      const float* sun_dir, int w_bits, uint64_t* out);
/* The same of the device build with the SAH pass (ARK_DDGI_FLAG_GPU_REBUILD_SAH; sah != 0)
 * against the host restatement with it; sah = 0: the entry above, word for word. out[40]:
 * [0..28] as above ([12] the sorted record indices as the sort left them, [13] the splits as
 * the pass left them), [29] the treelets, and the mismatch counts [30] the treelet list as a
 * set, [31] the sorted record indices after the pass, [32] the boxes per BVH2 node and [33]
 * per sorted primitive, by bits; they count towards the return value. */
int ark_ddgi_debug_lbvh_device_parity_sah(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                          const float* sun_dir, int w_bits, int sah, uint64_t* out);
/* The same with the collapse plan (ARK_DDGI_FLAG_GPU_REBUILD_PLAN; plan != 0, with sah != 0)
 * on both sides; plan = 0: the entry above, word for word. out[48]: [0..33] as above, [34]
 * the nodes above the treelets, and the mismatch counts [35] the packed picks at every node
 * index, [36] the eight cost words of every treelet root and upper node, by bits, [37] the
 * upper nodes' boxes, by bits, [38] the upper list as a set; they count towards the return
 * value. [39] the rounds the host restatement took above the treelets. */
int ark_ddgi_debug_lbvh_device_parity_plan(int device, const void* records, uint64_t n_records, const int32_t* class_of, uint32_t n_instances,
                                           const float* sun_dir, int w_bits, int sah, int plan, uint64_t* out);

/* compare_bvh8_canonical (the tree comparison of ark_ddgi_debug_lbvh_device_parity) tried on
 * the host: the LBVH restatement's tree of n triangles (9 floats each; triangle i of instance
 * and class i mod 3; sun_dir set: the light build instead) against a twin whose sibling blocks
 * and rows within each level are renumbered in a seeded random order, as the device's atomics
 * do, and against six mutations of the twin: (a) one occupied plane one quantum looser, (b) one
 * node's grid exponent raised by one with its planes re-quantised outward, (c) two internal
 * children of a node exchanged, (d) two leaf members of a node exchanged between slots, (e) two
 * records of different leaf slots exchanged, (f) one perm entry altered. out[16]: [0] nodes,
 * [1] nodes the twin renumbered, [2] differences reported for the twin (0 expected), [3] node
 * pairs visited, [4] the full check's violations for the twin, [5..10] differences of the
 * expected kind reported for (a)..(f) (non-zero expected), [11], [12] the full check's
 * violations for (a), (b) (0: it cannot tell them from the intended tree). Returns 0 when all
 * is as expected. No GPU. */
int ark_ddgi_debug_bvh8_compare_selftest(const float* triangles, uint64_t n, const float* sun_dir, uint64_t seed, uint64_t* out);

/* The world BVH8s the context's kernels read now (the front copy, after everything it
 * enqueued), downloaded and checked on the host. out[8] = {nodes, leaf children, max
 * depth, violations, records that are not holes, records with holes, order-independent
 * digest of the records that are not holes (sum of their FNV-1a 64), installed builder
 * (0 host, 1 device)}. A violation: the structure check set_scene's and the rebuilds'
 * BVHs pass fails; a plane is not exactly decodable; a triangle vertex (v0, v0 + e1,
 * v0 + e2) lies outside the decoded box of its leaf slot or of an ancestor; a triangle
 * sits under another hit-mask class's root; a class's nodes are not one contiguous
 * range from its root (a device build's: each depth's nodes one range behind the depth
 * above's; the host collapse orders each subtree's block breadth first instead); the
 * refit's level order differs from the one recomputed from the
 * downloaded nodes. Returns 0 when there is none, 1 otherwise. Synchronous. */
int ark_ddgi_debug_world_bvh_check(struct ArkDdgiCtx* ctx, uint64_t* out);

/* The device build of the sun's light-space BVH8 (ARK_DDGI_FLAG_GPU_REBUILD_SUN) run
 * serially on the host over n world triangles (9 floats each) with the very functions the
 * kernels call (csrc/lbvh_build.h: the light vertices, the light-space key, the radix
 * tree, the cut, the slots in ascending w, the rows), in sun_frame's frame; the boxes from
 * the records' light coordinates upward and the planes by the host collapse's node
 * writer. Then ark_ddgi_debug_sun_bvh_check's ray comparison through it. out[12]: [0..7]
 * as that function's; [8] structure violations (the structure check, the level order, each
 * depth one range behind the depth above's, every record the input's bit for bit, a node
 * whose occupied slots do not ascend in the low w edge of their Morton cells); [9] 1 when
 * the boxes' absolute inflation differs in bits from the host build's of the same input;
 * [10], [11] any-hit steps per ray x 1e6 (sun_shadow_cost) from these origins through the
 * LBVH and through the host build's tree. Returns 0 when clean, 2 on a ray mismatch, 1 on
 * a build error, a violation or an inflation difference. _opts: w_bits of the key's 60
 * Morton bits go to w (even, at most 20; negative: the default), the rest to u and v in halves; out[16], with
 * [12] leaf children, [13] depth, [14] records with holes, [15] w_bits. No GPU. */
int ark_ddgi_debug_sun_lbvh_check(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                  uint64_t* out);
int ark_ddgi_debug_sun_lbvh_check_opts(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                       int w_bits, uint64_t* out);
/* _opts with the SAH pass (sah != 0; [8] then counts slots that do not ascend in the low w
 * edge of their members' boxes; sah = 0: _opts' result word for word). out[17]: _opts'
 * sixteen, [16] the treelets the pass rebuilt. */
int ark_ddgi_debug_sun_lbvh_check_sah(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                      int w_bits, int sah, uint64_t* out);
/* _sah with the collapse plan (plan != 0, with sah != 0; plan = 0: _sah's result word for
 * word). out[19]: _sah's seventeen, [17] the plan's cost of the root as one BVH8 node (the
 * fp32 word), [18] the BVH8 nodes other than the root with at most three triangles below them. */
int ark_ddgi_debug_sun_lbvh_check_plan(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                       int w_bits, int sah, int plan, uint64_t* out);

/* ark_ddgi_debug_world_bvh_check for the installed light-space sun BVH. out[8] = {nodes,
 * leaf children, max depth, violations, records that are not holes, records with holes,
 * the order-independent record digest (equal to the world BVHs': the same records),
 * installed builder (0 host, 1 device)}. A violation: the structure check fails; a plane is
 * not exactly decodable; a light vertex of a record lies outside the decoded box of its
 * leaf slot or of an ancestor; the nodes are not one contiguous range from node 0 (a
 * device build's: each depth one range behind the depth above's); the refit's level order
 * differs from the recomputed one. Returns 0 when there is none, 1 otherwise - also when
 * no light-space BVH is installed (out all zero). Synchronous. */
int ark_ddgi_debug_sun_bvh_installed_check(struct ArkDdgiCtx* ctx, uint64_t* out);

/* How far the last refit (ark_ddgi_set_instances[_async]) went. out[4] = {world BVH nodes,
 * world nodes it reached, light-space sun BVH nodes, sun nodes it reached}: a node is
 * reached when an instance of the refit's dirty set lies below it by the node masks (bit
 * instance id mod 64, so instances 64 apart count as one); every other node kept its
 * planes. The last two are 0 without a light-space BVH, all four before the first refit
 * (and a BVH's two after a rebuild was installed, until the next refit). Synchronous. */
int ark_ddgi_debug_refit_reach(struct ArkDdgiCtx* ctx, uint64_t* out);

/* What ark_ddgi_update_geometry has allocated for the context's scene. out[4] = {allocations
 * of the triangle -> record map, its fills (the first use, then one per installed world
 * rebuild in between updates), device bytes held for the feature, update calls that wrote
 * positions}: all 0 for a scene that never made such a call. No device work. */
int ark_ddgi_debug_geometry_update_info(struct ArkDdgiCtx* ctx, uint64_t* out);

/* The sun's cover map (csrc/sun_cover_map.h) built on the host (no GPU) from n triangles
 * (9 floats each) for sun_dir, and its verdicts for n_rays origins (3 floats each) against a
 * brute-force any-hit over every triangle with the kernels' fp32 Moller-Trumbore
 * ([0.025, tmax]). budget_bytes: the map's byte budget (0: the default, 64 MB). out[13] =
 * {rays, occluded (brute force), resolved occluded, resolved lit, wrong verdicts, cells in u,
 * cells in v, map valid (0: no map for this scene or tmax - every ray undecided), cells with a
 * cover, undecided, and the fp32 bits of the grid's lower corner u0, v0 and of its cells per
 * unit length}. A wrong verdict: resolved occluded but not hit, or resolved lit but hit. */
int ark_ddgi_debug_cover_map_check(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                   uint64_t budget_bytes, uint64_t* out);

/* The device build of the same map against the host restatement. out[6] = {differing words
 * (all ones: the grids differ), cells in u, cells in v, host built a map, device built a
 * map, device build microseconds}. Synchronous. */
int ark_ddgi_debug_cover_map_device(int device, const float* triangles, uint64_t n, const float* sun_dir, uint64_t budget_bytes, uint64_t* out);

/* The sun's cover map as the context's last update used it. The update must have been a
 * counting one (ark_ddgi_set_counting). out[12] = {sun rays resolved occluded, resolved lit,
 * listed (k_shadow_gen's counts), map in use (0: none valid for this context - then the
 * first two are 0), cells in u, cells in v, map bytes, map build microseconds, and the host
 * restatement for the same rays - the update's hit points read back, the map rebuilt on the
 * host from the installed records: resolved occluded, resolved lit, listed, words in which
 * the installed map differs from the host's}. With no valid map the last four are computed
 * for no map (0, 0, listed, 0). Synchronous. */
int ark_ddgi_debug_sun_cover_counts(struct ArkDdgiCtx* ctx, uint64_t* out);
/* The same without the host restatement (a large scene's takes long): out[8..11] stay 0. */
int ark_ddgi_debug_sun_cover_counts_device(struct ArkDdgiCtx* ctx, uint64_t* out);

/* The shading schedule of the context's last update (csrc/shade_schedule.h). out[2] = {1: the
 * sun-only schedule ran (k_shade resolved the sun's rays from the cover map; no k_shadow_gen) -
 * 0: the generator schedule, the rays that update deferred to its second shading pass (the
 * undecided ones it listed; 0 under the generator schedule)}. Synchronous. */
int ark_ddgi_debug_shade_schedule(struct ArkDdgiCtx* ctx, uint64_t* out);
/* By default a pipelined window whose traversal runs the half-occupancy grid (fewer than 5 Mi
 * rays with frames in flight) keeps the generator schedule, which is faster there. enabled != 0:
 * such windows run the sun-only schedule too when the other conditions hold (tests: the
 * schedule's chunk and list edge cases at sizes a test can afford). Results are the same. */
int ark_ddgi_debug_set_sun_only_small_windows(struct ArkDdgiCtx* ctx, int enabled);

/* The probe rays' hit candidates (csrc/seed_cache.h; ARK_DDGI_FLAG_NO_RAY_SEEDS turns them
 * off). _seed_texel: the cache texel in [0, T * T) of a direction, on the host (the function
 * the kernels use). _seed_candidate_ok: the lookup's guard, on the host - 1 when `word` may be
 * tested by a launch whose opaque class owns the records [first, end), else 0 (the sentinel
 * 0xffffffff, records of other classes, indices past the array). No GPU for either.
 * _seed_info: out[5] = {1 if the context keeps a cache, T, first, end of the scene's opaque
 * records, probe rays of the last counting update whose candidate was hit}.
 * _seed_fill overwrites the whole cache (synchronous; the device is idle): mode 0 the
 * sentinel, 1 random records of the opaque class from the seed `value`, 2 the record `value`
 * everywhere. Every word is checked by the guard on the host first: a value outside the
 * opaque class is refused (ARK_DDGI_E_INVALID_ARGUMENT) and nothing is written. */
uint32_t ark_ddgi_debug_seed_texel(float x, float y, float z);
int ark_ddgi_debug_seed_candidate_ok(uint32_t word, uint32_t first, uint32_t end);
int ark_ddgi_debug_seed_info(struct ArkDdgiCtx* ctx, uint64_t* out);
int ark_ddgi_debug_seed_fill(struct ArkDdgiCtx* ctx, int mode, uint64_t value);

/* The absolute inflation steps of the last refit's boxes (a power of two each, from the
 * instances' object-space boxes through their transforms): out[2] = {world BVHs, light-space
 * sun BVH}; 0 before the first refit. A scene whose object-space boxes only ever grow would
 * see them grow with it. No device work. */
int ark_ddgi_debug_refit_inflation(struct ArkDdgiCtx* ctx, float* out);

/* The skinning pass (csrc/skinning.h) restated serially on the host, no GPU: the skin `desc`
 * describes (ark_ddgi_register_skin's checks; first_vertex is not used) run for `pose`
 * (pose->skin is not used). prev_positions: the previous run's positions, or NULL: the
 * skin's first run (velocity 0). out_positions and out_velocities vertex_count x 3,
 * out_vertices vertex_count, out_bounds[6] the host bound of the pose's positions (lo, hi)
 * that ark_ddgi_skin_geometry hands the refit. ARK_DDGI_E_INVALID_ARGUMENT for a desc or a
 * pose that registration or ark_ddgi_skin_geometry would refuse. */
int ark_ddgi_debug_skin_host(const ArkDdgiSkinDesc* desc, const ArkDdgiSkinPose* pose, const float* prev_positions, float* out_positions, ArkRTVertex* out_vertices,
                             float* out_velocities, float* out_bounds);
/* k_skin_vertices against that restatement for the same input, on a stream of its own
 * without a context; the kernel's outputs start at vertex dst_first_vertex of larger arrays
 * (a destination range may begin at any vertex). out[5] = {position words that differ by
 * bits, vertex words, velocity words (a NaN equals any NaN), words outside the outputs'
 * ranges that were written, nanoseconds of a second, timed run of the kernel (HIP events)}.
 * Synchronous. */
int ark_ddgi_debug_skin_device_parity(int device, const ArkDdgiSkinDesc* desc, const ArkDdgiSkinPose* pose, const float* prev_positions, uint32_t dst_first_vertex,
                                      uint64_t* out);

/* The ray-traced local-light shadow masks (ark_ddgi_rt_local_shadows) restated serially on
 * the host from the functions the generator kernel calls (csrc/rt_shadows.h), each ray
 * tested against every triangle record by brute force with the kernels' Möller–Trumbore.
 * `desc` is the entry's, except that depth and every out_mask are HOST pointers.
 * _host: no GPU. records: n_records x 12 words as the world BVHs hold them (instance
 * 0xffffffff: a hole); class_of[instance]: hit-mask class 0 opaque, 1 masked, 2 translucent;
 * bit c of class_mask: class c occludes (1 is what ark_ddgi_rt_local_shadows traces, 7 what
 * the DDGI path's shadow rays do). _host_ctx: the same over the records of the context's
 * front copy and its instances' classes, downloaded; it follows refits and vertex updates by
 * construction. Synchronous. counts (may be NULL): 4 per light = {sky, outside the cone,
 * lit, occluded} pixels. ARK_DDGI_E_INVALID_ARGUMENT for a descriptor the entry refuses.
 * _check_desc: the entry's argument checks alone (struct_size included), no context and no
 * device: ARK_DDGI_OK or ARK_DDGI_E_INVALID_ARGUMENT; pointers are compared, never followed.
 * _sample: the generator of pixel (px, py) at frame_index: out_state[3] = {the seed after
 * wang_hash, the state after the first and after the second xorshift}, out_disk[2] =
 * randomPointInDisk() (radius 1). _layout: out[0 .. n) of {offsetof(ArkRtShadowLight,
 * direction), outer_cone_angle_cos, source_radius, out_mask, offsetof(ArkRtShadowsDesc,
 * frame_index), world_from_view, view_from_projection, depth, lights, light_count,
 * reserved}; returns how many it wrote. */
int ark_ddgi_debug_rt_shadows_host(const uint32_t* records, uint64_t n_records, const int32_t* class_of, uint64_t n_instances, uint32_t class_mask,
                                   const ArkRtShadowsDesc* desc, uint64_t* counts);
int ark_ddgi_debug_rt_shadows_host_ctx(struct ArkDdgiCtx* ctx, uint32_t class_mask, const ArkRtShadowsDesc* desc, uint64_t* counts);
int ark_ddgi_debug_rt_shadows_check_desc(const ArkRtShadowsDesc* desc);
int ark_ddgi_debug_rt_shadows_sample(uint32_t frame_index, uint32_t px, uint32_t py, uint32_t* out_state, float* out_disk);
int ark_ddgi_debug_rt_shadows_layout(uint32_t* out, int n);

/* The reflection denoiser passes (ark_ddgi_rt_reflections_denoise) restated serially on the
 * host, tile by tile and lane by lane through the functions the kernels call
 * (csrc/refl_denoise.h). All host-only, no context and no device.
 * _host: `desc` is the entry's, except that every plane is a HOST pointer; the same planes
 * are written. ARK_DDGI_E_INVALID_ARGUMENT for a descriptor the entry refuses.
 * _check_desc: the entry's argument checks alone (struct_size included); pointers are
 * compared, never followed.
 * _layout: out[0 .. n) of the offsets of ArkReflDenoiseDesc's fields from width on, in
 * declaration order (24 words), then sizeof(ArkReflDenoiseDesc); returns how many it wrote.
 * _kat: known answers of the shared functions, in[n_in] -> out[n_out]:
 *   ROUND_UP8 1 -> 1; CLIP_AABB {min, max, sample} 9 -> 3; KERNEL_WEIGHT 1 -> 1;
 *   TILE_REDUCTION 64 lanes x 4 (lane = gy * 8 + gx) -> the 4 sums after the three fp16
 *   levels; EXP, POW512 (x^512), HALF (through fp16 and back) n -> n. */
#define ARK_REFL_KAT_ROUND_UP8      0
#define ARK_REFL_KAT_CLIP_AABB      1
#define ARK_REFL_KAT_KERNEL_WEIGHT  2
#define ARK_REFL_KAT_TILE_REDUCTION 3
#define ARK_REFL_KAT_EXP            4
#define ARK_REFL_KAT_POW512         5
#define ARK_REFL_KAT_HALF           6
int ark_ddgi_debug_refl_denoise_host(const ArkReflDenoiseDesc* desc);
int ark_ddgi_debug_refl_denoise_check_desc(const ArkReflDenoiseDesc* desc);
int ark_ddgi_debug_refl_denoise_layout(uint32_t* out, int n);
int ark_ddgi_debug_refl_denoise_kat(int which, const float* in, int n_in, float* out, int n_out);
/* One pass of ark_ddgi_rt_reflections_denoise alone, on the device with the entry's checks
 * and ordering: 0 historyCopy with firstCopy, 1 reproject, 2 prefilter, 3 resolveTemporal,
 * 4 historyCopy. For timing the passes (tools/refl_denoise_cost.py). */
int ark_ddgi_debug_refl_denoise_pass(struct ArkDdgiCtx* ctx, const ArkReflDenoiseDesc* desc, int pass, void* hip_stream);

/* The path tracer (ark_ddgi_path_trace) restated serially on the host from the functions its
 * kernels call (csrc/path_tracer.h): every path walked segment by segment, hits found by
 * brute force over the triangle records with the kernels' Möller–Trumbore and tie rule, the
 * image and (with a flag) the accumulation plane written. `desc` is the entry's, except that
 * image and accumulation are HOST pointers.
 * _host: no GPU; the scene preprocessed on the host as ark_ddgi_set_scene does it. _host_ctx:
 * over the context's own scene downloaded (the front copy's records and instance table, the
 * shading pools, the context's lights); it follows refits by construction. Synchronous.
 * vertices: NULL, or width * height * 16 records of 33 words, pixel-major, one per segment:
 *   [0] status (0 the path had ended, 1 scattered on, 2 missed, 3 killed (pdf <= 0), 4 hit and
 *   ended by the loop's condition), [1] RNG state before, [2..4] origin, [5..7] direction,
 *   [8] tmin, [9] record index of the hit (0xffffffff none), [10..12] t, u, v, [13] back face,
 *   [14] shadow bits (bit l: light l cast a ray, bit 16 + l: occluded), [15..17] attenuation
 *   and [18..20] radiance before, [21..23] and [24..26] after, [27..29] scattered direction,
 *   [30] RNG state after, [31] candidates the alpha test refused, [32] the glass program ran.
 * counts (may be NULL): 8 = {glass vertices, alpha-refused candidates, killed paths, paths
 * with a segment 8, occluded shadow rays, lit shadow rays, missed segments, vertices}.
 * _check_desc: the entry's argument checks alone (struct_size included), no context and no
 * device; pointers are compared, never followed. _layout: out[0 .. n) of the offsets of
 * ArkPathTracerDesc's fields from width on in declaration order (14 words), then
 * sizeof(ArkPathTracerDesc) and the bytes of a vertex record; returns how many it wrote.
 * _accumulate_host: the accumulate step or the reset copy alone over host planes (a flag is
 * required). _sample: out_state[2] = {the pixel's seed, the state after the two jitter
 * draws}, out_ray[6] = the camera ray's origin and direction. */
int ark_ddgi_debug_path_tracer_host(const ArkDdgiScene* scene, const ArkPathTracerDesc* desc, void* vertices, uint64_t* counts);
int ark_ddgi_debug_path_tracer_host_ctx(struct ArkDdgiCtx* ctx, const ArkPathTracerDesc* desc, void* vertices, uint64_t* counts);
int ark_ddgi_debug_path_tracer_check_desc(const ArkPathTracerDesc* desc);
int ark_ddgi_debug_path_tracer_layout(uint32_t* out, int n);
int ark_ddgi_debug_path_tracer_accumulate_host(const ArkPathTracerDesc* desc);
/* The list counts the last batch of the context's last ark_ddgi_path_trace call left on the
 * device: out[0 .. 16) the live paths of each segment, out[16 .. 32) the shadow rays each
 * segment listed. All zero before the first call. Synchronous. (A frame that fits one batch
 * is counted whole: tools/path_tracer_cost.py.) */
int ark_ddgi_debug_path_tracer_last_counts(struct ArkDdgiCtx* ctx, uint32_t* out);
/* _set_segments: the segments (1..16, default 16) the context's next ark_ddgi_path_trace calls
 * enqueue. For timing only (tools/path_tracer_cost.py): with fewer than 16 the pixels of paths
 * that would have gone on are not written. _random: pt_randomFloat alone. */
int ark_ddgi_debug_path_tracer_set_segments(struct ArkDdgiCtx* ctx, uint32_t segments);
int ark_ddgi_debug_path_tracer_random(uint32_t state, float* out_value, uint32_t* out_next);
int ark_ddgi_debug_path_tracer_sample(uint32_t px, uint32_t py, uint32_t width, uint32_t height, uint32_t frame_index, const float* world_from_view,
                                      const float* view_from_projection, uint32_t* out_state, float* out_ray);

/* The probe update's launches alone, over planted inputs (tests/test_gpu_probe_update_model.py):
 * the slot table, then the probe offsets when params->update_offsets, then the irradiance and
 * visibility blend with its border copy - the update's own launches with the update's own
 * arguments, as one serial frame ordered like ark_ddgi_update after whatever the context did
 * before. No traversal, no shading, no lights, and no scene is needed. The blend reads the
 * surfels the context holds (ark_ddgi_write of ARK_DDGI_SURFELS plants them); the offsets read
 * hit records: `hits` is a host array of [window probes][rays_per_probe] records in slot order
 * (on a Z-slab rank the rank's probes of the window, compacted), tri = 0xffffffff for a miss,
 * t negative for a back face; required when update_offsets is set, else it may be NULL. The
 * records are uploaded before the launches (the call waits for that copy, not for the kernels).
 * The planted records name no triangles of a scene, so the probe rays' hit candidates are not
 * written. The rolling window does not advance. Refuses what ark_ddgi_update refuses of
 * `params`. _layout: out[0 .. n) of {sizeof(ArkDdgiDebugHit), offsetof t, offsetof tri};
 * returns how many it wrote. */
typedef struct ArkDdgiDebugHit {
    float t;
    uint32_t tri;
} ArkDdgiDebugHit;
int ark_ddgi_debug_probe_update(struct ArkDdgiCtx* ctx, const ArkDdgiFrameParams* params, const ArkDdgiDebugHit* hits, void* hip_stream);
int ark_ddgi_debug_probe_update_layout(uint32_t* out, int n);

/* Hit shading alone, over planted hits (tests/test_gpu_hit_shading.py): one serial frame ordered
 * like ark_ddgi_update after whatever the context did before - the slot table, then `hits`
 * uploaded in place of the primary traversal, then exactly the shadow-ray and shading launches
 * of an update with the update's own arguments, in the schedule the update would pick (the
 * shadow-ray generator, the shadow traversal and k_shade; or, for the sun alone with its cover
 * map, k_shade, the traversal of what it left undecided and the deferred pass). The shadow rays
 * are really traced through the scene's BVH from the planted hit points. No probe offsets and no
 * blend run: surfels and ARK_DDGI_DEBUG_SHADOW_BITS are the outputs, ARK_DDGI_DEBUG_HITS reads
 * the planted records back. The rolling window does not advance and the probe rays' hit
 * candidates are not written.
 * `hits`: a host array of [window probes][rays_per_probe] records in slot order (on a Z-slab
 * rank the rank's probes of the window, compacted): instance 0xffffffff for a miss, else the
 * instance and the primitive within it, the hit attributes (u, v) and t, negative for a back
 * face. A hit need not lie where its ray meets the triangle: the hit point is origin + t dir.
 * The call maps them to the front copy's leaf-order records on the host (it waits for the device
 * first) and refuses, with ARK_DDGI_E_INVALID_ARGUMENT and before any launch: an instance or
 * primitive the scene does not hold (a hole names none), a non-finite t or |t| outside
 * [1e-4, z_far], a non-finite u or v, u < 0, v < 0 or u + v > 1. Refuses what ark_ddgi_update
 * refuses of `params`. _layout: out[0 .. n) of {sizeof(ArkDdgiDebugShadeHit), offsetof instance,
 * primitive, u, v, t}; returns how many it wrote.
 * _map: the entry's own mapping and refusals alone, on the host (no context, no GPU):
 * `record_words` are `records` triangle records of 12 words each as the world BVH holds them
 * (word 9 the instance, word 10 the primitive, instance 0xffffffff a hole), `instances` the
 * instance count; out_tri[i] receives the leaf-order record of hits[i] (0xffffffff for a
 * miss). Returns ARK_DDGI_E_INVALID_ARGUMENT for exactly what ark_ddgi_debug_shade refuses. */
/* _world_records: the triangle records the context's kernels read now (the front copy), in leaf
 * order, 12 words each, downloaded: *out_records receives their count, out_words the records
 * when it is not NULL and `capacity` (in records) holds them. What ARK_DDGI_DEBUG_HITS' triangle
 * indices point into. Synchronous. */
int ark_ddgi_debug_world_records(struct ArkDdgiCtx* ctx, uint32_t* out_words, uint64_t capacity, uint64_t* out_records);
typedef struct ArkDdgiDebugShadeHit {
    uint32_t instance, primitive;
    float u, v, t;
} ArkDdgiDebugShadeHit;
int ark_ddgi_debug_shade(struct ArkDdgiCtx* ctx, const ArkDdgiFrameParams* params, const ArkDdgiDebugShadeHit* hits, void* hip_stream);
int ark_ddgi_debug_shade_layout(uint32_t* out, int n);
int ark_ddgi_debug_shade_map(const uint32_t* record_words, uint64_t records, uint32_t instances, float z_far, const ArkDdgiDebugShadeHit* hits, uint64_t n,
                             uint32_t* out_tri);

#ifdef __cplusplus
}
#endif

#endif /* ARK_DDGI_DEBUG_H */
