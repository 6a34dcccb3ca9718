// lbvh_host.h — the device LBVH build restated on the host: what the device build is
// compared with bit for bit (tests and parity checks; no production path builds with it).
#pragma once

#include <stdint.h>
#include <vector>

#include "ddgi_types.h"
#include "lbvh_build.h"

namespace ark {

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
    // the collapse plan (plan: true): treelets then lists ranges of 2 and 3 too and nbox holds
    // every node's box, the upper nodes' included; the nodes above the treelets (any order),
    // the packed picks per BVH2 node (lbvh::planCosts' word, kPlanDone set; 0 elsewhere), the
    // eight costs of every treelet root and upper node (0 elsewhere), the opaque class's
    // root's cost[1] as a word (0: a root of at most kBvh8MaxLeafSize triangles), the rounds
    // the upper nodes took, and the BVH8 nodes but the roots with at most kBvh8MaxLeafSize
    // triangles below them (the plan never makes one)
    std::vector<lbvh::Member> upper;
    std::vector<uint32_t> picks;
    std::vector<float> pcost;
    uint32_t planRootCost = 0, planRounds = 0;
    bool planStalled = false;
    uint64_t smallInternal = 0;
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
// plan (with sah only): the collapse plan - the treelets down to single primitives, the plans
// of their nodes and of the nodes above them, and the collapse by lbvh::planCut.
LbvhHostResult build_lbvh_host(const std::vector<GpuTriangle>& records, const std::vector<int>& classOf, int criterion, const LbvhSunOptions* sun = nullptr,
                               const std::vector<uint32_t>* primOrder = nullptr, bool sah = false, bool plan = false);

} // namespace ark
