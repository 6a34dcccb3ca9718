// bvh_builder.h — binned-SAH BVH2 builder producing the 64 B node / 48 B triangle
// HBM layout consumed by the traversal kernels (ddgi_types.h). Replaces the
// acceleration structure build the Vulkan driver performs for the reference
// (VulkanAccelerationStructureKHR.cpp, build flag PREFER_FAST_TRACE).
#pragma once

#include <stdint.h>
#include <string>
#include <vector>

#include "ddgi_types.h"
#include "lbvh_build.h"

namespace ark {

struct BuildTriangle {
    float v0[3], v1[3], v2[3]; // world space
    uint32_t instance;
    uint32_t primitive;
    uint32_t flip_facing; // the instance's det(ObjectToWorld) < 0, stored in GpuTriangle t2.w
};

struct BvhBuildOptions {
    int max_leaf_size = 4;   // <= kMaxLeafSize
    int bins = 32;
    int max_depth = 60;      // hard cap: splits fall back to object median near it
    int threads = 0;         // 0 = hardware concurrency
    float inflate_abs = 0.0f; // absolute box inflation on top of the relative one (see collapse_bvh8 / visitNode8)
    float traversal_cost = 1.0f;
    float intersection_cost = 1.0f;
    float area_w[3] = { 1.0f, 1.0f, 1.0f }; // SAH face weights {xy, yz, zx} (surface area: all 1)
    // Early split clipping (Ernst & Greiner 2007): a triangle whose box surface exceeds
    // presplit_ratio x twice its area enters the build as up to 2^presplit_levels
    // references, the bounds of its pieces clipped at the box's longest-axis midpoints
    // (rounded outward) (0: off)
    int presplit_levels = 0;
    float presplit_ratio = 8.0f;
};

struct BvhBuildResult {
    std::vector<GpuBvhNode> nodes; // node 0 is the root (always an internal node)
    std::vector<GpuTriangle> tris; // leaf order
    uint32_t max_depth = 0;
    uint32_t max_leaf = 0;
    float sah_cost = 0.0f;
};

// Builds one BVH over `tris` (all of one hit-mask class). Node indices and
// triangle indices are offset by node_base / tri_base so several BVHs can share
// one node array and one triangle array.
BvhBuildResult build_bvh(const std::vector<BuildTriangle>& tris, const BvhBuildOptions& opt, uint32_t node_base, uint32_t tri_base);

struct Bvh8BuildResult {
    std::vector<GpuBvh8Node> nodes; // node 0 (+ node_base) is the root
    std::vector<GpuTriangle> tris;  // leaf triangle rows (GpuBvh8Node), holes included
    uint32_t max_depth = 0;
    uint32_t leaf_children = 0;
    uint64_t triangles = 0; // records of `tris` that are not holes
    float sah_cost = 0.0f; // SAH cost (node 1, triangle Bvh8CollapseOptions::tri_cost) relative to the root
};

// Collapses a BVH2 (built with max_leaf_size <= kBvh8MaxLeafSize, node_base 0,
// tri_base 0) into the 8-wide quantized layout: every node adopts the largest-area
// internal descendants of its BVH2 node until it has 8 children (or the SAH-optimal
// set, Bvh8CollapseOptions::sah_optimal), children are
// placed in octant slots, and the triangles of each node's leaf children are
// stored contiguously. Node/triangle indices are offset by node_base/tri_base.
struct Bvh8CollapseOptions {
    // true: the SAH-optimal child selection of Ylitie et al. 2017 (dynamic programming
    // over BVH2 subtrees, also merging subtrees of <= kBvh8MaxLeafSize triangles into
    // one leaf slot; the default: C4 traversal 2.26 -> 2.24 ms, shadow 0.74 -> 0.70 ms,
    // 2,148 -> 2,174 Mrays/s, profiles/r03_h_ab); false: greedy largest-area opening
    bool sah_optimal = true;
    float node_cost = 1.0f; // SAH cost of visiting a BVH8 node (8 box tests)
    float tri_cost = 1.0f;  // SAH cost of one triangle test
    float area_w[3] = { 1.0f, 1.0f, 1.0f }; // SAH face weights {xy, yz, zx}, as BvhBuildOptions::area_w
    // -1: internal children in octant slots (visited in slot ^ ray octant order);
    // 0-2: in slots 0, 1, ... by their box's lower bound along that axis (a BVH that
    // only rays along +axis traverse: the sun's light-space BVH, slot order = octant 0)
    int slot_sort_axis = -1;
    int threads = 0; // subtrees collapsed in parallel (0 = hardware concurrency)
};
Bvh8BuildResult collapse_bvh8(const BvhBuildResult& bvh2, uint32_t node_base, uint32_t tri_base, const Bvh8CollapseOptions& opt);

// The hit-mask class of an instance (ARK_RT_HIT_MASK_*): 0 opaque, 1 masked, 2 blend
int hit_mask_class(uint32_t hit_mask);

// The world BVHs: one BVH8 per hit-mask class, packed into one node array and one record
// array (opaque first; roots[c] -1: the class is empty).
struct WorldBvh8 {
    std::vector<GpuBvh8Node> nodes;
    std::vector<GpuTriangle> tris; // leaf triangle rows, holes included
    int32_t roots[3] = { -1, -1, -1 };
    uint32_t opaqueNodes = 0, depth = 0, maxLeaf = 0;
    uint64_t triangles = 0;   // records that are not holes
    float sah = 0.0f;         // BVH2 SAH cost of the opaque class
    float inflateAbs = 0.0f;  // one absolute box inflation for all classes (shadow rays test all): bvh8_inflation_box of their bounds
    bool tooLarge = false;    // failed on the 31-bit index limit
};
// Builds them from the classes' world-space triangles (each class's input freed once its
// BVH2 stands): opt's leaf size and inflation are set here; false with `why` when a BVH2
// leaf exceeds kBvh8MaxLeafSize (out.maxLeaf), the set exceeds 31-bit indices
// (out.tooLarge) or checkBvh8Structure fails.
bool build_world_bvh8(std::vector<BuildTriangle> cls[3], BvhBuildOptions opt, const Bvh8CollapseOptions& copt, WorldBvh8& out, std::string& why);

// Structural check of a BVH8 before anything reaches the GPU: every node is
// referenced once from a root-reachable parent (no cycles, no sharing), every leaf's
// triangles lie inside the triangle array and every triangle (every record but the
// holes of the rows) is covered once.
bool checkBvh8Structure(const std::vector<GpuBvh8Node>& allNodes, const std::vector<GpuTriangle>& allTris, const int32_t* roots, int nRoots, std::string& why);
// The nodes of a BVH8 by depth, deepest first (a node's internal children are one level
// deeper): the refit's launch order, order[offsets[i] .. offsets[i + 1]) one level.
bool bvhLevelOrder(const GpuBvh8Node* h, uint64_t n, const int32_t* roots, int nRoots, std::vector<uint32_t>& order, std::vector<uint32_t>& offsets);

// The 48-B triangle record of a build triangle (v0, e1 = v1 - v0, e2 = v2 - v0 in
// fp32, instance, primitive, facing flip): what the traversal's Möller–Trumbore reads.
GpuTriangle make_gpu_triangle(const BuildTriangle& t);

// Hole records of the triangle rows (kHoleInstance)
GpuTriangle holeTriangle();
bool isHoleTriangle(const GpuTriangle& t);
// Triangle indices of leaf slot s of a node (tri_base + s + stride * i for the
// consecutive set bits of its row from i = 0); 0 for a slot that is not a leaf, -1
// when a leaf slot has no triangle, an internal slot is marked leaf, or the slot's
// spread reaches another slot's triangle (GpuBvh8Node)
int bvh8SlotTriangles(const GpuBvh8Node& nd, int s, uint32_t out[kBvh8MaxLeafSize]);

// The device LBVH build (ddgi_bvh_build.hip) restated serially on the host with the same
// lbvh_build.h functions: the three classes' BVH8s over the records that are not holes
// (classOf: instance -> class), each node's rows private, the records copied bit for
// bit, the boxes from the records upward and the planes by the collapse's node writer.
struct LbvhHostResult {
    std::vector<GpuBvh8Node> nodes; // each class one breadth-first range from roots[c], opaque first
    std::vector<GpuTriangle> tris;  // rows, holes included (no padding record)
    std::vector<uint32_t> perm, order, levelOffsets;
    int32_t roots[3] = { -1, -1, -1 };
    uint32_t opaqueNodes = 0, depth = 0;
    uint64_t triangles = 0, leafChildren = 0;
    double sah = 0.0; // BVH8 SAH cost of the opaque class (node 1, triangle 1), as Bvh8BuildResult::sah_cost
    float inflateAbs = 0.0f;            // the boxes' absolute inflation
    uint64_t slotOrderViolations = 0;   // sun: nodes whose occupied slots do not ascend in their cells' low w edge
    // the stages before the tree, as the device build holds them (ark_ddgi_debug_lbvh_device_parity):
    // the header's counts, box and largest |world coordinate| (sun; else 0), the sorted keys,
    // the record of each sorted primitive, and split[] (set at the internal indices
    // [first, last) of each class range, 0 elsewhere)
    uint32_t classCount[3] = { 0, 0, 0 };
    float sceneLo[3] = { 0, 0, 0 }, sceneHi[3] = { 0, 0, 0 }, maxAbs = 0.0f;
    std::vector<uint64_t> keysSorted;
    std::vector<uint32_t> idxSorted, split;
    // the SAH pass (sah: true): idxSorted and split above are as the pass leaves them,
    // idxMorton as the sort left them; its work list (any order), a box per BVH2 node of a
    // treelet (0 elsewhere) and per sorted primitive, 6 floats each
    std::vector<uint32_t> idxMorton;
    std::vector<lbvh::Member> treelets;
    std::vector<float> nbox, pbox;
};
// sun: the light-space BVH8 of the sun's shadow rays instead (k_lbvh_prims_light /
// k_lbvh_keys_light): one tree over every class (roots[0]), keys and boxes of the records'
// light coordinates in `frame` (rows u, v, w), w given wBits of the key, slots by ascending w
struct LbvhSunOptions {
    double frame[9];
    int wBits = lbvh::kSunKeyBitsW;
};
// primOrder: the compacted primitive order (a permutation of the indices of the records that
// are not holes; null: ascending). The device's comes from atomics, and the stable sort
// carries it into runs of equal keys: given the device's order, the result is the tree the
// device has to build, ties included.
// sah: the SAH pass over the treelets (k_lbvh_treelet_sah restated serially) between the
// hierarchy and the collapse, which then opens by lbvh::kOpenLargestBox whatever `criterion`.
LbvhHostResult build_lbvh_host(const std::vector<GpuTriangle>& records, const std::vector<int>& classOf, int criterion, const LbvhSunOptions* sun = nullptr,
                               const std::vector<uint32_t>* primOrder = nullptr, bool sah = false);

// Two BVH8 sets of the same records compared in canonical form (ark_ddgi_debug_lbvh_device_parity:
// the device build against build_lbvh_host). Node numbers within a level and tri_base come
// from atomics on the device, so both trees are walked from each root in slot order, internal
// children matched by rank. At every pair of nodes: equal imask, leaf_mask, leaf_tris and
// tri_stride (header); equal p and e (grid); equal qlo / qhi bytes of every occupied slot
// (planes); every row position of a leaf slot the same 48 bytes (records) and the same source
// record in perm (perm; skipped when either perm is null); every other position of the rows a
// hole (holes). shape: the classes' roots present alike, opaqueNodes, depth, the node count of
// every depth, the node and record counts, and each tree's rows together exactly its records.
// children: a child index outside the nodes, or a node met twice. levelOrder: a tree's order /
// levelOffsets (when given) differ from bvhLevelOrder of its nodes. padding: a tree's padding
// record (when given) is not all zero.
struct Bvh8TreeView {
    const std::vector<GpuBvh8Node>* nodes = nullptr;
    const std::vector<GpuTriangle>* tris = nullptr; // rows, holes included, no padding record
    const std::vector<uint32_t>* perm = nullptr;
    const std::vector<uint32_t>* order = nullptr;
    const std::vector<uint32_t>* levelOffsets = nullptr;
    const GpuTriangle* padding = nullptr;
    int32_t roots[3] = { -1, -1, -1 };
    uint32_t opaqueNodes = 0, depth = 0;
};
struct Bvh8CanonicalDiff {
    uint64_t shape = 0, header = 0, grid = 0, planes = 0, children = 0, records = 0, perm = 0, holes = 0, levelOrder = 0, padding = 0;
    int64_t firstA = -1, firstB = -1; // the first differing pair of nodes (-1: none)
    uint64_t pairs = 0;               // pairs of nodes visited
    uint64_t total() const { return shape + header + grid + planes + children + records + perm + holes + levelOrder + padding; }
};
Bvh8CanonicalDiff compare_bvh8_canonical(const Bvh8TreeView& a, const Bvh8TreeView& b);

// The full check of a BVH8 set (ark_ddgi_debug_lbvh_check, ark_ddgi_debug_world_bvh_check):
// every class's nodes one contiguous range from its root (counted in violations; depths
// whose nodes are not one range behind the depth above's in notBreadthFirst alone: the
// host collapse orders its subtrees' blocks breadth first, not the whole class), valid rows, every
// plane exactly decodable, every record that is not a hole in exactly one leaf, under its
// class's root (classOf: instance -> class, null: unchecked), its vertices (v0, v0 + e1,
// v0 + e2; with `vertices`, also the 9 floats of its primitive) inside the decoded box of
// its leaf slot and of every ancestor. lightFrame (rows u, v, w): the sun's light-space BVH,
// whose boxes hold the records' light coordinates (lbvh::lightVertices) instead.
struct Bvh8CheckResult {
    uint64_t violations = 0, nodes = 0, leafChildren = 0, internalChildren = 0, maxDepth = 0, triangles = 0;
    uint64_t notContiguous = 0, notBreadthFirst = 0;
};
Bvh8CheckResult check_bvh8_full(const std::vector<GpuBvh8Node>& nodes, const std::vector<GpuTriangle>& tris, const int32_t* roots, int nRoots,
                                const std::vector<int>* classOf, const float* vertices, const double* lightFrame = nullptr);

// Absolute box inflation for the BVH8 slab test: 1e-6 of the diagonal of the
// bounding box of nTriangles world-space triangles (9 floats each). It bounds
// the rounding of (p - o) * idir for anchors p and ray origins o in the scene
// (about 2 ulp of the diagonal, i.e. 2.4e-7 of it) with a 4x margin.
float bvh8_inflation(const float* xyz, uint64_t nTriangles);
float bvh8_inflation_box(const float lo[3], const float hi[3]);

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
void sun_frame(const float sun_dir[3], double frame[3][3]);
void sun_add_triangles(SunBvhInput& in, const std::vector<BuildTriangle>& world_tris, int threads = 0);
// The same from world-space triangle records as the world BVHs hold them (holes skipped):
// the background rebuild after a sun-direction change or a refit (scene_store.cpp hostBuildSun)
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
