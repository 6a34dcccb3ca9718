// bvh8_check.cpp — the full check of a BVH8 set and the canonical comparison of two.
#include "bvh8_check.h"

#include <algorithm>
#include <cstring>
#include <utility>

#include "bvh_builder.h"
#include "bvh_internal.h"
#include "lbvh_build.h"

namespace ark {

Bvh8CheckResult check_bvh8_full(const std::vector<GpuBvh8Node>& nodes, const std::vector<GpuTriangle>& tris, const int32_t* roots, int nRoots,
                                const std::vector<int>* classOf, const float* vertices, const double* lightFrame)
{
    Bvh8CheckResult R;
    struct Box {
        float lo[3], hi[3];
    };
    struct Item {
        uint32_t node;
        int32_t parent; // item of the parent's slot box (-1: a root)
        Box box;        // this node's box as its parent decodes it
        uint32_t depth;
    };
    std::vector<uint8_t> seenTri(tris.size(), 0), seenNode(nodes.size(), 0);
    for (int c = 0; c < nRoots; ++c) {
        if (roots[c] < 0) continue;
        // breadth first: the class's nodes must be roots[c], roots[c] + 1, ... in this order
        std::vector<Item> items;
        items.push_back({ static_cast<uint32_t>(roots[c]), -1, {}, 1u });
        uint32_t lowest = 0xffffffffu, highest = 0u;
        uint64_t classNodes = 0;
        std::vector<uint32_t> levelLo, levelHi, levelCount; // of the nodes of each depth
        for (size_t qi = 0; qi < items.size(); ++qi) {
            const Item it = items[qi];
            if (it.node >= nodes.size() || seenNode[it.node]) {
                R.violations++;
                continue;
            }
            seenNode[it.node] = 1;
            R.nodes++;
            if (levelLo.size() < it.depth) {
                levelLo.resize(it.depth, 0xffffffffu);
                levelHi.resize(it.depth, 0u);
                levelCount.resize(it.depth, 0u);
            }
            levelLo[it.depth - 1] = std::min(levelLo[it.depth - 1], it.node);
            levelHi[it.depth - 1] = std::max(levelHi[it.depth - 1], it.node);
            levelCount[it.depth - 1]++;
            lowest = std::min(lowest, it.node);
            highest = std::max(highest, it.node);
            classNodes++;
            R.maxDepth = std::max<uint64_t>(R.maxDepth, it.depth);
            const GpuBvh8Node& nd = nodes[it.node];
            if ((nd.leaf_tris >> 24) || (nd.leaf_mask & nd.imask)) R.violations++;
            uint32_t internal = 0;
            for (int s = 0; s < 8; ++s) {
                const bool in = (nd.imask >> s) & 1u;
                uint32_t slotTris[kBvh8MaxLeafSize];
                const int cnt = bvh8SlotTriangles(nd, s, slotTris);
                if (cnt < 0) {
                    R.violations++;
                    continue;
                }
                if (!in && cnt == 0) continue;
                Box b;
                if (!decodeSlotBox(nd, s, b.lo, b.hi)) R.violations++;
                if (in) {
                    R.internalChildren++;
                    items.push_back({ nd.child_base + internal++, static_cast<int32_t>(qi), b, it.depth + 1u });
                    continue;
                }
                R.leafChildren++;
                for (int ti = 0; ti < cnt; ++ti) {
                    const uint32_t t = slotTris[ti];
                    if (t >= tris.size() || isHoleTriangle(tris[t]) || seenTri[t]) {
                        R.violations++;
                        continue;
                    }
                    seenTri[t] = 1;
                    R.triangles++;
                    const GpuTriangle& g = tris[t];
                    uint32_t inst, prim;
                    std::memcpy(&inst, &g.t2[1], 4);
                    std::memcpy(&prim, &g.t2[2], 4);
                    if (classOf && (inst >= classOf->size() || (*classOf)[inst] != c)) R.violations++; // under the wrong class's root
                    float v[6][3];
                    recordVertices(g, v);
                    if (lightFrame) {
                        const float e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
                        float m;
                        lbvh::lightVertices(g.t0, e1, e2, lightFrame, v, m);
                    }
                    int nv = 3;
                    if (vertices) {
                        std::memcpy(v[3], vertices + 9ull * prim, 9 * sizeof(float));
                        nv = 6;
                    }
                    // inside the leaf slot's box and every ancestor's
                    const Box* bx = &b;
                    for (int32_t up = static_cast<int32_t>(qi);; up = items[up].parent) {
                        for (int k = 0; k < nv; ++k)
                            for (int a = 0; a < 3; ++a)
                                if (!(v[k][a] >= bx->lo[a] && v[k][a] <= bx->hi[a])) R.violations++;
                        if (items[up].parent < 0) break;
                        bx = &items[up].box;
                    }
                }
            }
        }
        // the class's nodes are the range [root, root + count)
        if (classNodes && (lowest != static_cast<uint32_t>(roots[c]) || highest - lowest + 1u != classNodes)) R.notContiguous++;
        // breadth first: each depth's nodes one range behind the depth above's
        uint32_t at = static_cast<uint32_t>(roots[c]);
        for (size_t d = 0; d < levelCount.size(); ++d) {
            if (levelLo[d] != at || levelHi[d] - levelLo[d] + 1u != levelCount[d]) R.notBreadthFirst++;
            at += levelCount[d];
        }
    }
    for (size_t t = 0; t < tris.size(); ++t)
        if (!seenTri[t] && !isHoleTriangle(tris[t])) R.violations++; // unreachable
    R.violations += R.notContiguous;
    return R;
}

Bvh8CanonicalDiff compare_bvh8_canonical(const Bvh8TreeView& A, const Bvh8TreeView& B)
{
    Bvh8CanonicalDiff D;
    const Bvh8TreeView* T[2] = { &A, &B };
    const std::vector<GpuBvh8Node>& na = *A.nodes;
    const std::vector<GpuBvh8Node>& nb = *B.nodes;
    auto span = [](const GpuBvh8Node& nd) { return nd.leaf_tris ? 32u - static_cast<uint32_t>(__builtin_clz(nd.leaf_tris)) : 0u; };
    // each tree on its own: the level order, the padding record, the rows exactly the records
    std::vector<uint64_t> perDepth[2];
    for (int t = 0; t < 2; ++t) {
        const std::vector<GpuBvh8Node>& nodes = *T[t]->nodes;
        std::vector<uint32_t> order, offsets;
        const bool walked = bvhLevelOrder(nodes.data(), nodes.size(), T[t]->roots, 3, order, offsets);
        if (!walked) D.children++;
        if (T[t]->order && T[t]->levelOffsets && (!walked || order != *T[t]->order || offsets != *T[t]->levelOffsets)) D.levelOrder++;
        for (size_t l = 0; walked && l + 1 < offsets.size(); ++l) perDepth[t].push_back(offsets[l + 1] - offsets[l]); // (deepest first)
        if (walked && (order.size() != nodes.size() || offsets.size() != static_cast<size_t>(T[t]->depth) + 1u)) D.shape++;
        uint64_t rows = 0;
        for (const GpuBvh8Node& nd : nodes) rows += span(nd);
        if (rows != T[t]->tris->size()) D.shape++;
        if (T[t]->perm && T[t]->perm->size() != T[t]->tris->size()) D.shape++;
        if (T[t]->padding) {
            const GpuTriangle zero {};
            if (std::memcmp(T[t]->padding, &zero, sizeof(zero)) != 0) D.padding++;
        }
    }
    if (perDepth[0] != perDepth[1]) D.shape++;
    if (na.size() != nb.size() || A.tris->size() != B.tris->size() || A.opaqueNodes != B.opaqueNodes || A.depth != B.depth) D.shape++;
    const bool perms = A.perm && B.perm && A.perm->size() == A.tris->size() && B.perm->size() == B.tris->size();
    std::vector<uint8_t> seenA(na.size(), 0), seenB(nb.size(), 0);
    std::vector<std::pair<uint32_t, uint32_t>> work;
    for (int c = 0; c < 3; ++c) {
        if ((A.roots[c] >= 0) != (B.roots[c] >= 0)) D.shape++;
        else if (A.roots[c] >= 0) work.push_back({ static_cast<uint32_t>(A.roots[c]), static_cast<uint32_t>(B.roots[c]) });
    }
    while (!work.empty()) {
        const auto [ia, ib] = work.back();
        work.pop_back();
        const uint64_t before = D.total();
        if (ia >= na.size() || ib >= nb.size() || seenA[ia] || seenB[ib]) {
            D.children++;
        } else {
            seenA[ia] = seenB[ib] = 1;
            D.pairs++;
            const GpuBvh8Node& a = na[ia];
            const GpuBvh8Node& b = nb[ib];
            const bool sameHeader = a.imask == b.imask && a.leaf_mask == b.leaf_mask && a.leaf_tris == b.leaf_tris && a.tri_stride == b.tri_stride;
            if (!sameHeader) D.header++;
            if (std::memcmp(a.p, b.p, sizeof(a.p)) != 0 || std::memcmp(a.e, b.e, sizeof(a.e)) != 0) D.grid++;
            if (sameHeader) {
                for (int s = 0; s < 8; ++s) {
                    if (!(((a.imask | a.leaf_mask) >> s) & 1u)) continue;
                    for (int ax = 0; ax < 3; ++ax)
                        if (a.qlo[ax][s] != b.qlo[ax][s] || a.qhi[ax][s] != b.qhi[ax][s]) D.planes++;
                }
                // the rows, position by position: a leaf slot's records, holes elsewhere
                for (uint32_t pos = 0; pos < span(a); ++pos) {
                    const uint64_t ra = static_cast<uint64_t>(a.tri_base) + pos, rb = static_cast<uint64_t>(b.tri_base) + pos;
                    if (ra >= A.tris->size() || rb >= B.tris->size()) {
                        D.records++;
                        continue;
                    }
                    const GpuTriangle& ta = (*A.tris)[ra];
                    const GpuTriangle& tb = (*B.tris)[rb];
                    if ((a.leaf_tris >> pos) & 1u) {
                        if (std::memcmp(&ta, &tb, sizeof(GpuTriangle)) != 0 || isHoleTriangle(ta)) D.records++;
                        if (perms && (*A.perm)[ra] != (*B.perm)[rb]) D.perm++;
                    } else {
                        const GpuTriangle hole = holeTriangle();
                        if (std::memcmp(&ta, &hole, sizeof(hole)) != 0 || std::memcmp(&tb, &hole, sizeof(hole)) != 0) D.holes++;
                        if (perms && ((*A.perm)[ra] != 0xffffffffu || (*B.perm)[rb] != 0xffffffffu)) D.holes++;
                    }
                }
            }
            // internal children by rank (as far as both have them)
            const uint32_t ka = static_cast<uint32_t>(__builtin_popcount(a.imask)), kb = static_cast<uint32_t>(__builtin_popcount(b.imask));
            for (uint32_t k = std::min(ka, kb); k-- > 0;) work.push_back({ a.child_base + k, b.child_base + k });
        }
        if (D.total() != before && D.firstA < 0) {
            D.firstA = ia;
            D.firstB = ib;
        }
    }
    return D;
}

uint64_t recordViolations(const std::vector<GpuTriangle>& rows, const std::vector<uint32_t>& perm, const std::vector<GpuTriangle>& source)
{
    uint64_t n = source.size(), violations = 0;
    std::vector<uint32_t> seen(n, 0);
    for (size_t i = 0; i < rows.size(); ++i) {
        if (isHoleTriangle(rows[i])) continue;
        uint32_t prim;
        std::memcpy(&prim, &rows[i].t2[2], 4);
        if (prim >= n || perm[i] != prim || std::memcmp(&rows[i], &source[prim], sizeof(GpuTriangle)) != 0) violations++;
        else seen[prim]++;
    }
    for (uint64_t i = 0; i < n; ++i)
        if (seen[i] != 1) violations++;
    return violations;
}

} // namespace ark
