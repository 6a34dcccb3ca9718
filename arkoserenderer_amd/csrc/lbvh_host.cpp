// lbvh_host.cpp — the device LBVH's build logic on the host (lbvh_build.h), serially.
#include "lbvh_host.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

#include "bvh_builder.h"
#include "bvh_internal.h"

namespace ark {
namespace {
// k_lbvh_treelet_sah, serially: the binary tree of one treelet T (4 .. kTreeletPrims
// primitives) by a three-axis sweep SAH. box: 6 ordered words per sorted primitive, as the
// sort left them. sorted and split are rewritten inside T's range, nbox and pbox filled.
// plan (the collapse plan; T of 2 primitives or more): split down to single primitives, nbox
// of every node, then the nodes' plans bottom-up: their words in picks, the root's costs in pcost.
void treeletSahHost(const lbvh::Member& T, const std::vector<uint32_t>& box, std::vector<uint32_t>& sorted, std::vector<uint32_t>& split, std::vector<float>& nbox,
                    std::vector<float>& pbox, bool plan, std::vector<uint32_t>& picks, std::vector<float>& pcost)
{
    const uint32_t leafMost = plan ? 1u : static_cast<uint32_t>(kBvh8MaxLeafSize);
    const uint32_t first = T.r.first, n = lbvh::count(T.r);
    auto at = [&](uint32_t prim) { return &box[6ull * (first + prim)]; };
    std::vector<uint32_t> ord[3];
    for (int ax = 0; ax < 3; ++ax) {
        std::vector<uint32_t> key(n);
        for (uint32_t p = 0; p < n; ++p) key[p] = lbvh::sweepKey(lbvh::orderedFloat(at(p)[ax]), lbvh::orderedFloat(at(p)[3 + ax]));
        ord[ax].resize(n);
        for (uint32_t p = 0; p < n; ++p) ord[ax][p] = p;
        std::stable_sort(ord[ax].begin(), ord[ax].end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    }
    struct Segment {
        uint32_t f, l, node; // positions and node index relative to `first`
    };
    std::vector<Segment> todo(1, Segment { 0u, n - 1u, T.node - first }), final, made;
    std::vector<float> area(n, 0.0f);
    std::vector<uint32_t> splitRel(n, 0xffffffffu);
    std::vector<uint8_t> side(n, 0);
    auto unite = [](uint32_t u[6], const uint32_t* b) {
        for (int c = 0; c < 3; ++c) {
            u[c] = std::min(u[c], b[c]);
            u[3 + c] = std::max(u[3 + c], b[3 + c]);
        }
    };
    while (!todo.empty()) {
        const Segment sg = todo.back();
        todo.pop_back();
        const uint32_t cnt = sg.l - sg.f + 1u;
        if (cnt <= leafMost) {
            final.push_back(sg);
            continue;
        }
        made.push_back(sg);
        uint64_t best = lbvh::kNoSplit;
        for (int ax = 0; ax < 3; ++ax) {
            std::vector<std::array<uint32_t, 6>> pre(cnt), suf(cnt);
            uint32_t u[6] = { ~0u, ~0u, ~0u, 0u, 0u, 0u };
            for (uint32_t i = 0; i < cnt; ++i) {
                unite(u, at(ord[ax][sg.f + i]));
                std::copy(u, u + 6, pre[i].begin());
            }
            uint32_t v[6] = { ~0u, ~0u, ~0u, 0u, 0u, 0u };
            for (uint32_t i = cnt; i-- > 0;) {
                unite(v, at(ord[ax][sg.f + i]));
                std::copy(v, v + 6, suf[i].begin());
            }
            if (ax == 0) {
                for (int c = 0; c < 6; ++c) nbox[6ull * (first + sg.node) + c] = lbvh::orderedFloat(pre[cnt - 1u][c]);
                area[sg.node] = lbvh::halfArea(pre[cnt - 1u].data());
            }
            for (uint32_t k = 1; k < cnt; ++k) best = std::min(best, lbvh::splitKey(lbvh::halfArea(pre[k - 1u].data()), lbvh::halfArea(suf[k].data()), k, cnt, static_cast<uint32_t>(ax)));
        }
        uint32_t axis, k;
        lbvh::chosenSplit(best, cnt, axis, k);
        for (uint32_t i = 0; i < cnt; ++i) side[ord[axis][sg.f + i]] = i >= k ? 1 : 0;
        for (int b = 0; b < 3; ++b) std::stable_partition(ord[b].begin() + sg.f, ord[b].begin() + sg.l + 1u, [&](uint32_t p) { return side[p] == 0; });
        splitRel[sg.node] = sg.f + k - 1u;
        todo.push_back(Segment { sg.f, sg.f + k - 1u, sg.f + k - 1u });
        todo.push_back(Segment { sg.f + k, sg.l, sg.f + k });
    }
    for (const Segment& sg : final)
        for (uint32_t i = sg.f; i <= sg.l; ++i)
            if (splitRel[i] == 0xffffffffu) splitRel[i] = sg.f;
    std::vector<uint32_t> src(n);
    for (uint32_t i = 0; i < n; ++i) src[i] = sorted[first + i];
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t prim = ord[0][i];
        sorted[first + i] = src[prim];
        for (int c = 0; c < 6; ++c) pbox[6ull * (first + i) + c] = lbvh::orderedFloat(at(prim)[c]);
        if (first + i != lbvh::treeletSpareIndex(T)) split[first + i] = first + splitRel[i];
    }
    if (!plan) return;
    // the plans, children before parents (a child is made after its parent)
    std::vector<std::array<float, 8>> cost(n);
    auto childCosts = [&](uint32_t f, uint32_t l, uint32_t node, float C[8]) {
        if (f == l) return lbvh::planLeafCosts(at(ord[0][f]), C);
        std::copy(cost[node].begin(), cost[node].end(), C);
    };
    for (size_t k = made.size(); k-- > 0;) {
        const Segment& sg = made[k];
        const uint32_t sp = splitRel[sg.node];
        float L[8], R[8];
        childCosts(sg.f, sp, sp, L);
        childCosts(sp + 1u, sg.l, sp + 1u, R);
        picks[first + sg.node] = lbvh::planCosts(area[sg.node], sg.l - sg.f + 1u, L, R, cost[sg.node].data()) | lbvh::kPlanDone;
    }
    std::copy(cost[T.node - first].begin(), cost[T.node - first].end(), pcost.begin() + 8ull * T.node);
}
} // namespace

LbvhHostResult build_lbvh_host(const std::vector<GpuTriangle>& rec, const std::vector<int>& classOf, int criterion, const LbvhSunOptions* sun,
                               const std::vector<uint32_t>* primOrder, bool sahPass, bool plan)
{
    LbvhHostResult R;
    if (sahPass) criterion = lbvh::kOpenLargestBox;
    plan = plan && sahPass; // (the flag does nothing without the SAH pass)
    const lbvh::KeyLayout layout = { sun ? sun->wBits : lbvh::kMortonBits };
    const int slotRule = sun ? lbvh::kSlotsAscendingW : lbvh::kSlotsOctant;
    // the vertices a record is boxed by: the world ones, or their light coordinates
    float maxAbs = 0.0f;
    auto boxVertices = [&](const GpuTriangle& g, float v[3][3]) {
        if (!sun) return recordVertices(g, v);
        const float e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
        float m;
        lbvh::lightVertices(g.t0, e1, e2, sun->frame, v, m);
        maxAbs = std::max(maxAbs, m);
    };
    // primitives: the records that are not holes, their boxes, the scene box
    std::vector<uint32_t> idx;
    std::vector<Aabb> pbox;
    Aabb scene;
    if (primOrder) {
        idx = *primOrder;
    } else {
        for (size_t i = 0; i < rec.size(); ++i)
            if (!isHoleTriangle(rec[i])) idx.push_back(static_cast<uint32_t>(i));
    }
    for (uint32_t i : idx) {
        float v[3][3];
        boxVertices(rec[i], v);
        Aabb b;
        for (int k = 0; k < 3; ++k) b.grow(v[k]);
        scene.grow(b);
        pbox.push_back(b);
    }
    const uint32_t n = static_cast<uint32_t>(idx.size());
    // (the light-space inflation: build_sun_bvh's expression)
    const float inflateAbs = !n ? 0.0f : sun ? 2.0f * bvh8_inflation_box(scene.lo, scene.hi) + 2e-6f * maxAbs : bvh8_inflation_box(scene.lo, scene.hi);
    R.inflateAbs = inflateAbs;
    float scale[3], extent[3];
    for (int a = 0; a < 3; ++a) {
        scale[a] = n ? lbvh::mortonScale(scene.lo[a], scene.hi[a]) : 0.0f;
        extent[a] = n ? scene.hi[a] - scene.lo[a] : 0.0f;
    }
    auto instanceOf = [&](uint32_t record) {
        uint32_t inst;
        std::memcpy(&inst, &rec[record].t2[1], 4);
        return inst;
    };
    std::vector<uint64_t> key(n);
    uint32_t classCount[3] = { 0, 0, 0 };
    for (uint32_t j = 0; j < n; ++j) {
        float c[3];
        for (int a = 0; a < 3; ++a) c[a] = 0.5f * pbox[j].lo[a] + 0.5f * pbox[j].hi[a];
        const uint32_t inst = instanceOf(idx[j]);
        const int cls = sun ? 0 : inst < classOf.size() ? classOf[inst] : 0; // the sun's: one tree for all classes
        classCount[cls]++;
        key[j] = sun ? lbvh::lightKey(c, scene.lo, scene.hi, layout) : lbvh::mortonKey(c, scene.lo, scale, static_cast<uint32_t>(cls));
    }
    std::vector<uint32_t> sorted(n);
    for (uint32_t j = 0; j < n; ++j) sorted[j] = j;
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    std::vector<uint64_t> keys(n);
    for (uint32_t j = 0; j < n; ++j) keys[j] = key[sorted[j]];
    std::vector<uint32_t> split(n, 0u), position(n, 0u);
    // the record of each sorted primitive; the SAH pass permutes it inside its treelets
    std::vector<uint32_t> sortedRec(n);
    for (uint32_t j = 0; j < n; ++j) sortedRec[j] = idx[sorted[j]];
    lbvh::SahBoxes boxes {};
    std::vector<uint32_t> obox; // the sorted primitives' boxes as ordered words
    if (sahPass) {
        R.idxMorton = sortedRec;
        R.nbox.assign(n * 6ull, 0.0f);
        R.pbox.assign(n * 6ull, 0.0f);
        obox.resize(n * 6ull);
        for (uint32_t j = 0; j < n; ++j) {
            float v[3][3];
            boxVertices(rec[sortedRec[j]], v);
            lbvh::primBox(v, &obox[6ull * j]);
        }
        if (plan) {
            R.picks.assign(n, 0u);
            R.pcost.assign(n * 8ull, 0.0f);
        }
        boxes.nbox = R.nbox.data();
        boxes.pbox = R.pbox.data();
        for (int a = 0; a < 3; ++a) {
            boxes.lo[a] = scene.lo[a];
            boxes.hi[a] = scene.hi[a];
        }
    }
    const lbvh::SahBoxes* sahBoxes = sahPass ? &boxes : nullptr;
    // hierarchy and collapse, class by class, level by level (the kernels' atomics: plain counters)
    uint32_t records = 0, first = 0;
    std::vector<std::vector<uint32_t>> levels; // node counts [depth][class]
    for (int c = 0; c < 3; ++c) {
        const uint32_t lo = first, hi = first + classCount[c];
        first = hi;
        if (lo == hi) continue;
        const size_t firstTreelet = R.treelets.size(), firstUpper = R.upper.size();
        for (uint32_t i = lo; i + 1u < hi; ++i) {
            const lbvh::Range r = lbvh::nodeRange(keys.data(), lo, hi, i);
            split[i] = lbvh::findSplit(keys.data(), lo, hi, r);
            if (!sahPass) continue;
            // the SAH pass's work list (k_lbvh_hierarchy's appends; any order)
            lbvh::Member m[2];
            const int k = lbvh::treeletsOf(r, split[i], i == lo, m, plan);
            R.treelets.insert(R.treelets.end(), m, m + k);
            // the nodes above the treelets (k_lbvh_hierarchy's second list)
            if (plan && lbvh::count(r) > lbvh::kTreeletPrims) R.upper.push_back(lbvh::Member { r, i });
        }
        for (size_t t = firstTreelet; t < R.treelets.size(); ++t) treeletSahHost(R.treelets[t], obox, sortedRec, split, R.nbox, R.pbox, plan, R.picks, R.pcost);
        if (plan) {
            // k_lbvh_upper_plan: rounds over the class's upper nodes until none is left; a
            // node whose children are done is boxed and planned (the device's schedule differs,
            // the result does not: unions of ordered words, plans of finished children)
            std::vector<lbvh::Member> todo(R.upper.begin() + static_cast<std::ptrdiff_t>(firstUpper), R.upper.end());
            auto done = [&](const lbvh::Member& m) { return lbvh::count(m.r) <= lbvh::kTreeletPrims || (R.picks[m.node] & lbvh::kPlanDone) != 0u; };
            auto childPlan = [&](const lbvh::Member& m, uint32_t b[6], float C[8]) {
                if (lbvh::count(m.r) == 1u) {
                    // a stray primitive: its box from its vertices, kept for the collapse too
                    std::copy(&obox[6ull * m.r.first], &obox[6ull * m.r.first] + 6, b);
                    for (int q = 0; q < 6; ++q) R.pbox[6ull * m.r.first + q] = lbvh::orderedFloat(b[q]);
                    return lbvh::planLeafCosts(b, C);
                }
                for (int q = 0; q < 6; ++q) b[q] = lbvh::ordered(R.nbox[6ull * m.node + q]);
                std::copy(&R.pcost[8ull * m.node], &R.pcost[8ull * m.node] + 8, C);
            };
            while (!todo.empty()) {
                std::vector<lbvh::Member> later, now;
                for (const lbvh::Member& m : todo) {
                    lbvh::Member a, b;
                    lbvh::childrenOf(split.data(), m, a, b);
                    (done(a) && done(b) ? now : later).push_back(m);
                }
                if (now.empty()) {
                    R.planStalled = true; // (never: the list is a tree's)
                    break;
                }
                for (const lbvh::Member& m : now) {
                    lbvh::Member a, b;
                    lbvh::childrenOf(split.data(), m, a, b);
                    uint32_t lb[6], rb[6], box[6];
                    float L[8], Rc[8], Cn[8];
                    childPlan(a, lb, L);
                    childPlan(b, rb, Rc);
                    const uint32_t word = lbvh::planUpperNode(lb, L, rb, Rc, lbvh::count(m.r), box, Cn);
                    for (int q = 0; q < 6; ++q) R.nbox[6ull * m.node + q] = lbvh::orderedFloat(box[q]);
                    std::copy(Cn, Cn + 8, &R.pcost[8ull * m.node]);
                    R.picks[m.node] = word | lbvh::kPlanComputed | lbvh::kPlanDone;
                }
                todo.swap(later);
                R.planRounds++;
            }
            if (c == 0 && hi - lo > static_cast<uint32_t>(kBvh8MaxLeafSize)) std::memcpy(&R.planRootCost, &R.pcost[8ull * lo], 4);
        }
        R.roots[c] = static_cast<int32_t>(R.nodes.size());
        std::vector<lbvh::Member> level(1), next;
        level[0].r.first = lo;
        level[0].r.last = hi - 1u;
        level[0].node = lo;
        R.nodes.resize(R.nodes.size() + 1);
        uint32_t levelBase = static_cast<uint32_t>(R.roots[c]), depth = 0;
        while (!level.empty()) {
            ++depth;
            next.clear();
            const uint32_t nextBase = levelBase + static_cast<uint32_t>(level.size());
            for (size_t i = 0; i < level.size(); ++i) {
                lbvh::WideNode w;
                lbvh::planNode(keys.data(), split.data(), level[i], criterion, extent, w, slotRule, layout, sahBoxes, plan ? R.picks.data() : nullptr);
                const uint32_t slot0 = static_cast<uint32_t>(next.size());
                const uint32_t triBase = w.rows.span ? records : 0u;
                records += w.rows.span;
                GpuBvh8Node nd;
                std::memset(&nd, 0, sizeof(nd));
                nd.imask = static_cast<uint8_t>(w.imask);
                nd.child_base = nextBase + slot0;
                nd.tri_base = triBase;
                nd.leaf_tris = w.rows.leaf_tris;
                nd.tri_stride = static_cast<uint8_t>(w.rows.stride);
                nd.leaf_mask = static_cast<uint8_t>(w.rows.leaf_mask);
                R.nodes[levelBase + i] = nd;
                int64_t lastLow = -1;
                for (uint32_t s = 0; s < 8u; ++s) {
                    const int k = lbvh::memberInSlot(w, s);
                    if (k < 0) continue;
                    const lbvh::Member& m = w.member[k];
                    if (sun) {
                        // the occupied slots' Morton cells ascend in their low w edge, without a gap
                        const int64_t low = lbvh::memberLowW(keys.data(), m, layout, sahBoxes);
                        if (low < lastLow || s >= static_cast<uint32_t>(w.members)) R.slotOrderViolations++;
                        lastLow = low;
                    }
                    if ((w.imask >> s) & 1u) {
                        next.push_back(m);
                    } else {
                        R.leafChildren++;
                        for (uint32_t t = 0; t < lbvh::count(m.r); ++t) position[m.r.first + t] = triBase + s + w.rows.stride * t;
                    }
                }
            }
            R.nodes.resize(R.nodes.size() + next.size());
            if (levels.size() < depth) levels.resize(depth, std::vector<uint32_t>(3, 0u));
            levels[depth - 1][c] = static_cast<uint32_t>(level.size());
            levelBase = nextBase;
            level.swap(next);
        }
        if (c == 0) R.opaqueNodes = static_cast<uint32_t>(R.nodes.size());
        R.depth = std::max(R.depth, depth);
    }
    for (int c = 0; c < 3; ++c) R.classCount[c] = classCount[c];
    for (int a = 0; a < 3 && n; ++a) {
        R.sceneLo[a] = scene.lo[a];
        R.sceneHi[a] = scene.hi[a];
    }
    R.maxAbs = maxAbs;
    R.idxSorted.resize(n);
    for (uint32_t j = 0; j < n; ++j) R.idxSorted[j] = sortedRec[j];
    R.keysSorted = keys;
    R.split = split;
    // scatter
    R.tris.assign(records, holeTriangle());
    R.perm.assign(records, 0xffffffffu);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t src = sortedRec[j];
        R.tris[position[j]] = rec[src];
        R.perm[position[j]] = src;
    }
    R.triangles = n;
    // level order: deepest first, ascending node index within a level (bvhLevelOrder's format)
    {
        std::vector<uint32_t> classBase(3, 0u);
        for (int c = 0; c < 3; ++c) classBase[c] = R.roots[c] >= 0 ? static_cast<uint32_t>(R.roots[c]) : 0u;
        std::vector<std::vector<uint32_t>> byDepth(levels.size());
        for (size_t d = 0; d < levels.size(); ++d)
            for (int c = 0; c < 3; ++c) {
                for (uint32_t k = 0; k < levels[d][c]; ++k) byDepth[d].push_back(classBase[c] + k);
                classBase[c] += levels[d][c];
            }
        R.levelOffsets.assign(1, 0u);
        for (size_t d = byDepth.size(); d-- > 0;) {
            R.order.insert(R.order.end(), byDepth[d].begin(), byDepth[d].end());
            R.levelOffsets.push_back(static_cast<uint32_t>(R.order.size()));
        }
    }
    // boxes from the records upward, the planes by the node writer (what k_refit_nodes
    // does on the device): children have higher indices than their parent
    std::vector<Aabb> nodeBox(R.nodes.size());
    double sah = 0.0;
    std::vector<double> childArea(R.nodes.size(), 0.0); // sum over a node's children of area x cost
    std::vector<double> unionArea(R.nodes.size(), 0.0); // area of the union of a node's child boxes
    std::vector<uint64_t> below(R.nodes.size(), 0u);    // triangles below a node
    for (size_t k = R.nodes.size(); k-- > 0;) {
        GpuBvh8Node& nd = R.nodes[k];
        Aabb slot[8], box;
        const Aabb* slotBox[8];
        uint32_t internal = 0;
        for (int s = 0; s < 8; ++s) {
            slotBox[s] = nullptr;
            double cost = 1.0;
            if ((nd.imask >> s) & 1u) {
                below[k] += below[nd.child_base + internal];
                if (below[nd.child_base + internal] <= static_cast<uint64_t>(kBvh8MaxLeafSize)) R.smallInternal++;
                slot[s] = nodeBox[nd.child_base + internal++];
            } else if ((nd.leaf_mask >> s) & 1u) {
                uint32_t t[kBvh8MaxLeafSize];
                const int cnt = bvh8SlotTriangles(nd, s, t);
                for (int i = 0; i < cnt; ++i) {
                    float v[3][3];
                    boxVertices(R.tris[t[i]], v);
                    for (int q = 0; q < 3; ++q) slot[s].grow(v[q]);
                }
                inflateChildBox(slot[s], inflateAbs);
                cost = std::max(cnt, 0);
                below[k] += static_cast<uint64_t>(std::max(cnt, 0));
            } else {
                continue;
            }
            slotBox[s] = &slot[s];
            box.grow(slot[s]);
            childArea[k] += static_cast<double>(slot[s].area()) * cost;
        }
        writeNodePlanes(nd, box, slotBox);
        nodeBox[k] = box;
        unionArea[k] = box.area();
        inflateChildBox(nodeBox[k], inflateAbs);
    }
    // BVH8 SAH cost of the opaque class relative to its root's box (node 1, triangle 1: collapseQueue's)
    if (R.roots[0] >= 0) {
        const uint32_t r0 = static_cast<uint32_t>(R.roots[0]);
        const double rootArea = std::max(1e-30, unionArea[r0]);
        sah = 1.0;
        for (uint32_t k = r0; k < r0 + R.opaqueNodes; ++k) sah += childArea[k] / rootArea;
    }
    R.sah = sah;
    return R;
}

} // namespace ark
