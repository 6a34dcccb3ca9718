// bvh8_check.h — checks of finished BVH8 sets beyond checkBvh8Structure (the debug entry
// points, the world BVH check after refits, the device build's parity with the host's).
#pragma once

#include <stdint.h>
#include <vector>

#include "ddgi_types.h"

namespace ark {

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

// The rows of a build over `source` (source[i]'s primitive is i) against it: the row
// records that are not source[primitive] bit for bit or that perm does not name, plus
// the source records that are not in exactly one row.
uint64_t recordViolations(const std::vector<GpuTriangle>& rows, const std::vector<uint32_t>& perm, const std::vector<GpuTriangle>& source);

} // namespace ark
