// bvh_builder.h — the host build of the world BVHs: the binned-SAH BVH2 builder, its
// collapse into the 8-wide quantized nodes and triangle rows the traversal kernels read
// (ddgi_types.h), the hit-mask classes' BVH8s as one set, that layout's structural checks
// and record helpers. Replaces the acceleration structure build the Vulkan driver performs
// for the reference (VulkanAccelerationStructureKHR.cpp, build flag PREFER_FAST_TRACE).
#pragma once

#include <stdint.h>
#include <string>
#include <vector>

#include "ddgi_types.h"

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
    uint32_t opaqueRecords = 0; // the opaque class's records: tris[0 .. opaqueRecords), holes included
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
// The box of a node's slot as the kernels decode it in fp32 (fma(q, 2^(e - 127), p));
// false when a plane's fp32 value is not exactly p + q 2^(e - 127)
bool decodeSlotBox(const GpuBvh8Node& nd, int slot, float lo[3], float hi[3]);

// The build triangles of a soup of n triangles, 9 floats each: instance 0, primitive i,
// no facing flip (the debug entry points' input)
std::vector<BuildTriangle> soupTriangles(const float* triangles, uint64_t n);

// Absolute box inflation for the BVH8 slab test: 1e-6 of the diagonal of the
// bounding box of nTriangles world-space triangles (9 floats each). It bounds
// the rounding of (p - o) * idir for anchors p and ray origins o in the scene
// (about 2 ulp of the diagonal, i.e. 2.4e-7 of it) with a 4x margin.
float bvh8_inflation(const float* xyz, uint64_t nTriangles);
float bvh8_inflation_box(const float lo[3], const float hi[3]);

} // namespace ark
