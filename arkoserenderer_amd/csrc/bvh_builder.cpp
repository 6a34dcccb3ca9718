// bvh_builder.cpp — the host build of the world BVHs (C++ threads): the binned-SAH BVH2
// over world-space triangles, its collapse into the 8-wide quantized layout and the
// structural checks every build passes before it reaches the GPU.
#include "bvh_builder.h"

#include "../../include/ark_ddgi.h"
#include "bvh_internal.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <utility>

namespace ark {
namespace {

struct Ref {
    Aabb box;
    float c[3];
    uint32_t tri; // the BuildTriangle this reference stands for
};

// --- early split clipping (BvhBuildOptions::presplit_levels) -----------------------
struct Poly {
    double p[9][3]; // a triangle clipped by up to 6 planes has at most 9 vertices
    int n = 0;
};

// The part of `in` on one side of the plane x[axis] = at (keepLow: <=), exactly in
// double but for the interpolated crossing points.
Poly clipPoly(const Poly& in, int axis, double at, bool keepLow)
{
    Poly out;
    for (int i = 0; i < in.n; ++i) {
        const double* a = in.p[i];
        const double* b = in.p[(i + 1) % in.n];
        const double da = keepLow ? at - a[axis] : a[axis] - at, db = keepLow ? at - b[axis] : b[axis] - at;
        if (da >= 0.0 && out.n < 9) std::memcpy(out.p[out.n++], a, sizeof(double) * 3);
        if ((da >= 0.0) != (db >= 0.0) && out.n < 9) {
            const double t = da / (da - db);
            for (int k = 0; k < 3; ++k) out.p[out.n][k] = a[k] + (b[k] - a[k]) * t;
            out.p[out.n][axis] = at; // on the plane
            out.n++;
        }
    }
    return out;
}

// float bounds of a double polygon, rounded outward (plus a relative hair for the
// crossing points' interpolation error), so the box contains the exact piece
Aabb polyBox(const Poly& P)
{
    Aabb b;
    for (int i = 0; i < P.n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double v = P.p[i][a], e = std::fabs(v) * 1e-12 + 1e-30;
            b.lo[a] = std::min(b.lo[a], std::nextafter(static_cast<float>(v - e), -INFINITY));
            b.hi[a] = std::max(b.hi[a], std::nextafter(static_cast<float>(v + e), INFINITY));
        }
    return b;
}

void splitRefs(const Poly& P, const Aabb& box, uint32_t tri, int level, double stopArea, std::vector<Ref>& out)
{
    const float e0 = box.hi[0] - box.lo[0], e1 = box.hi[1] - box.lo[1], e2 = box.hi[2] - box.lo[2];
    if (level == 0 || box.area() <= stopArea) {
        Ref r;
        r.box = box;
        for (int a = 0; a < 3; ++a) r.c[a] = 0.5f * (box.lo[a] + box.hi[a]);
        r.tri = tri;
        out.push_back(r);
        return;
    }
    const int axis = (e0 >= e1 && e0 >= e2) ? 0 : (e1 >= e2 ? 1 : 2);
    const double at = 0.5 * (static_cast<double>(box.lo[axis]) + static_cast<double>(box.hi[axis]));
    for (int side = 0; side < 2; ++side) {
        const Poly Q = clipPoly(P, axis, at, side == 0);
        if (Q.n < 3) continue;
        Aabb qb = polyBox(Q);
        for (int a = 0; a < 3; ++a) { // never outside the parent's (already conservative) box
            qb.lo[a] = std::max(qb.lo[a], box.lo[a]);
            qb.hi[a] = std::min(qb.hi[a], box.hi[a]);
        }
        splitRefs(Q, qb, tri, level - 1, stopArea, out);
    }
}

struct Range {
    int32_t code; // >= 0 node index, < 0 leaf code
    Aabb box;
};

// f(begin, end) over [0, n) in `threads` contiguous chunks (one when n is small)
template<class F>
void parallelFor(size_t n, int threads, F f)
{
    const int T = std::max(1, std::min<int>(threads, static_cast<int>(n >> 16) + 1));
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back([&, t] { f(n * t / T, n * (t + 1) / T); });
    f(0, n / T);
    for (std::thread& th : pool) th.join();
}

class Builder {
public:
    Builder(const std::vector<BuildTriangle>& tris, const BvhBuildOptions& opt, uint32_t nodeBase, uint32_t triBase)
        : m_opt(opt), m_nodeBase(nodeBase), m_triBase(triBase)
    {
        const size_t nt = tris.size();
        const int hw = opt.threads > 0 ? opt.threads : static_cast<int>(std::thread::hardware_concurrency());
        m_refs.resize(nt);
        parallelFor(nt, hw, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; ++i) {
                Ref& r = m_refs[i];
                r.box.grow(tris[i].v0);
                r.box.grow(tris[i].v1);
                r.box.grow(tris[i].v2);
                for (int a = 0; a < 3; ++a) r.c[a] = 0.5f * (r.box.lo[a] + r.box.hi[a]);
                r.tri = static_cast<uint32_t>(i);
            }
        });
        if (opt.presplit_levels > 0) {
            std::vector<Ref> refs;
            refs.reserve(nt + nt / 2);
            for (size_t i = 0; i < nt; ++i) {
                const BuildTriangle& t = tris[i];
                double e1[3], e2[3];
                for (int a = 0; a < 3; ++a) {
                    e1[a] = static_cast<double>(t.v1[a]) - t.v0[a];
                    e2[a] = static_cast<double>(t.v2[a]) - t.v0[a];
                }
                const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
                const double area2 = std::sqrt(cx * cx + cy * cy + cz * cz); // twice the area
                const double stop = opt.presplit_ratio * area2;
                if (!(m_refs[i].box.area() > stop)) {
                    refs.push_back(m_refs[i]);
                    continue;
                }
                Poly P;
                P.n = 3;
                for (int a = 0; a < 3; ++a) {
                    P.p[0][a] = t.v0[a];
                    P.p[1][a] = t.v1[a];
                    P.p[2][a] = t.v2[a];
                }
                const size_t before = refs.size();
                splitRefs(P, m_refs[i].box, static_cast<uint32_t>(i), opt.presplit_levels, stop, refs);
                if (refs.size() == before) refs.push_back(m_refs[i]); // degenerate clip: keep the whole
            }
            m_refs.swap(refs);
        }
        const size_t n = m_refs.size();
        // a binary tree over n leaves has at most n - 1 internal nodes (+ node 0's slot);
        // written before read, so not zero-filled (1.3 GB at C4)
        m_nodes.reset(new GpuBvhNode[n + 1]);
        m_threads = std::max(1, hw);
        m_threadsAvail = std::max(0, hw - 1);
    }

    BvhBuildResult run(const std::vector<BuildTriangle>& tris)
    {
        BvhBuildResult res;
        const uint32_t n = static_cast<uint32_t>(m_refs.size());
        m_nodeCount = 1; // node 0 = root
        Bin all = binRange(0, n, nullptr, nullptr);
        Range root = buildRange(0, n, 1, all.b, all.c, 0);
        if (root.code < 0) {
            // whole set fits one leaf: root with the leaf + an unreachable far child
            Aabb far;
            const float p[3] = { 1e30f, 1e30f, 1e30f };
            far.grow(p);
            writeNode(0, root.box, root.code, far, ~0);
        }
        res.nodes.assign(m_nodes.get(), m_nodes.get() + m_nodeCount.load());
        m_nodes.reset();
        res.tris.resize(n);
        parallelFor(n, m_threads, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; ++i) res.tris[i] = make_gpu_triangle(tris[m_refs[i].tri]);
        });
        res.max_depth = m_maxDepth.load();
        res.max_leaf = m_maxLeaf.load();
        res.sah_cost = sahCost(res.nodes, root.box);
        return res;
    }

private:
    float sahCost(const std::vector<GpuBvhNode>& nodes, const Aabb& rootBox) const
    {
        const float ra = rootBox.area();
        if (!(ra > 0.0f)) return 0.0f;
        double cost = 0.0;
        for (const GpuBvhNode& nd : nodes) {
            Aabb b[2];
            b[0].lo[0] = nd.n0[0]; b[0].hi[0] = nd.n0[1]; b[0].lo[1] = nd.n0[2]; b[0].hi[1] = nd.n0[3];
            b[1].lo[0] = nd.n1[0]; b[1].hi[0] = nd.n1[1]; b[1].lo[1] = nd.n1[2]; b[1].hi[1] = nd.n1[3];
            b[0].lo[2] = nd.n2[0]; b[0].hi[2] = nd.n2[1]; b[1].lo[2] = nd.n2[2]; b[1].hi[2] = nd.n2[3];
            for (int c = 0; c < 2; ++c) {
                if (b[c].lo[0] > 1e29f) continue;
                double a = b[c].area() / ra;
                if (nd.child[c] >= 0) cost += m_opt.traversal_cost * a;
                else cost += m_opt.intersection_cost * a * ((static_cast<uint32_t>(~nd.child[c]) & (kMaxLeafSize - 1)) + 1);
            }
        }
        return static_cast<float>(cost + m_opt.traversal_cost);
    }

    void writeNode(uint32_t local, const Aabb& b0, int32_t c0, const Aabb& b1, int32_t c1)
    {
        GpuBvhNode& nd = m_nodes[local];
        Aabb bb[2] = { b0, b1 };
        for (int c = 0; c < 2; ++c) {
            if (bb[c].lo[0] > 1e29f) continue; // far sentinel stays exact
            inflateChildBox(bb[c], m_opt.inflate_abs);
        }
        nd.n0[0] = bb[0].lo[0]; nd.n0[1] = bb[0].hi[0]; nd.n0[2] = bb[0].lo[1]; nd.n0[3] = bb[0].hi[1];
        nd.n1[0] = bb[1].lo[0]; nd.n1[1] = bb[1].hi[0]; nd.n1[2] = bb[1].lo[1]; nd.n1[3] = bb[1].hi[1];
        nd.n2[0] = bb[0].lo[2]; nd.n2[1] = bb[0].hi[2]; nd.n2[2] = bb[1].lo[2]; nd.n2[3] = bb[1].hi[2];
        nd.child[0] = c0;
        nd.child[1] = c1;
        nd.child[2] = 0;
        nd.child[3] = 0;
    }

    int32_t leafCode(uint32_t first, uint32_t count) const
    {
        uint32_t v = ((m_triBase + first) << kLeafCountBits) | (count - 1u);
        return ~static_cast<int32_t>(v);
    }

    // Bounds of a run of references (box of their boxes, box of their centroids) and
    // their count; with scale != null also their binning along all three axes at once
    // (bins[a][k]: the references whose centroid falls in bin k of axis a of `cbox`).
    // The references are the builder's own array, partitioned in place level by level,
    // so every pass reads them sequentially.
    struct Bin {
        Aabb b, c;
        uint32_t n = 0;
        void add(const Ref& r)
        {
            b.grow(r.box);
            c.grow(r.c);
            ++n;
        }
        void add(const Bin& o)
        {
            b.grow(o.b);
            c.grow(o.c);
            n += o.n;
        }
    };
    static constexpr int kMaxBins = 64;
    struct Bins {
        Bin k[3][kMaxBins];
    };

    Bin binRange(uint32_t first, uint32_t count, const Aabb* cbox, Bins* bins) const
    {
        const int B = std::max(4, std::min(m_opt.bins, kMaxBins));
        float lo[3] = { 0, 0, 0 }, scale[3] = { 0, 0, 0 };
        bool axis[3] = { false, false, false };
        if (bins)
            for (int a = 0; a < 3; ++a) {
                const float ext = cbox->hi[a] - cbox->lo[a];
                axis[a] = ext > 0.0f;
                lo[a] = cbox->lo[a];
                scale[a] = axis[a] ? static_cast<float>(B) / ext : 0.0f;
            }
        auto work = [&](uint32_t b, uint32_t e, Bin& all, Bins* out) {
            for (uint32_t i = b; i < e; ++i) {
                const Ref& r = m_refs[i];
                all.add(r);
                if (out)
                    for (int a = 0; a < 3; ++a)
                        if (axis[a]) out->k[a][std::min(B - 1, std::max(0, static_cast<int>((r.c[a] - lo[a]) * scale[a])))].add(r);
            }
        };
        Bin all;
        // the top levels in parallel: per-thread partial bins, merged (unions and counts
        // do not depend on the order)
        const int T = count >= (1u << 20) ? std::min(m_threads, static_cast<int>(count >> 18)) : 1;
        if (T <= 1) {
            work(first, first + count, all, bins);
            return all;
        }
        std::vector<Bin> part(T);
        std::vector<Bins> partBins(bins ? T : 0);
        std::vector<std::thread> pool;
        for (int t = 0; t < T; ++t) {
            const uint32_t b = first + static_cast<uint32_t>(static_cast<uint64_t>(count) * t / T);
            const uint32_t e = first + static_cast<uint32_t>(static_cast<uint64_t>(count) * (t + 1) / T);
            pool.emplace_back([&, t, b, e] { work(b, e, part[t], bins ? &partBins[t] : nullptr); });
        }
        for (std::thread& th : pool) th.join();
        for (int t = 0; t < T; ++t) {
            all.add(part[t]);
            if (bins)
                for (int a = 0; a < 3; ++a)
                    for (int k = 0; k < B; ++k) bins->k[a][k].add(partBins[t].k[a][k]);
        }
        return all;
    }

    // box / cbox: the bounds of the range (from the parent's bins)
    Range buildRange(uint32_t first, uint32_t count, int depth, const Aabb& box, const Aabb& cbox, int forcedLocal = -1)
    {
        {
            int md = m_maxDepth.load();
            while (depth > md && !m_maxDepth.compare_exchange_weak(md, depth)) {}
        }
        const int maxLeaf = std::min(m_opt.max_leaf_size, kMaxLeafSize);
        if (count == 1 || (count <= 2 && maxLeaf >= 2)) return makeLeaf(first, count, box);

        // split: binned SAH over 3 axes, object-median fallback near the depth cap
        const int log2n = static_cast<int>(std::ceil(std::log2(std::max(1.0, static_cast<double>(count) / maxLeaf))));
        const bool forceMedian = depth + log2n + 2 >= m_opt.max_depth;
        uint32_t mid = first + count / 2;
        bool split = true, childBounds = false;
        Bin left, right;
        if (!forceMedian) {
            const int B = std::max(4, std::min(m_opt.bins, kMaxBins));
            float bestCost = INFINITY;
            int bestAxis = -1, bestBin = -1;
            if (count <= kSmallCount) {
                // few references: the same SAH sweep over the bins they occupy only (a
                // split between two occupied bins equals the one at the upper bin, which
                // the full sweep - descending, strict < - would keep), without
                // initialising 3 x B bins per node
                bestSmallSplit(first, count, cbox, B, bestCost, bestAxis, bestBin);
            }
            Bins bins;
            if (count > kSmallCount) binRange(first, count, &cbox, &bins);
            for (int a = 0; a < 3 && count > kSmallCount; ++a) {
                const float ext = cbox.hi[a] - cbox.lo[a];
                if (!(ext > 0.0f)) continue;
                const Bin* bb = bins.k[a];
                float leftArea[kMaxBins];
                uint32_t leftCount[kMaxBins];
                Aabb acc;
                uint32_t n = 0;
                for (int k = 0; k < B - 1; ++k) {
                    acc.grow(bb[k].b);
                    n += bb[k].n;
                    leftArea[k] = acc.area(m_opt.area_w);
                    leftCount[k] = n;
                }
                Aabb accR;
                uint32_t nr = 0;
                for (int k = B - 1; k > 0; --k) {
                    accR.grow(bb[k].b);
                    nr += bb[k].n;
                    const uint32_t nl = leftCount[k - 1];
                    if (nl == 0 || nr == 0) continue;
                    const float cost = leftArea[k - 1] * nl + accR.area(m_opt.area_w) * nr;
                    if (cost < bestCost) {
                        bestCost = cost;
                        bestAxis = a;
                        bestBin = k;
                    }
                }
            }
            const float area = box.area(m_opt.area_w);
            const float splitCost = m_opt.traversal_cost + (area > 0.0f ? bestCost / area : 0.0f) * m_opt.intersection_cost;
            const float leafCost = m_opt.intersection_cost * count;
            if (static_cast<int>(count) <= maxLeaf && (bestAxis < 0 || leafCost <= splitCost)) split = false;
            if (split && bestAxis >= 0) {
                const int a = bestAxis;
                const float ext = cbox.hi[a] - cbox.lo[a];
                const float scale = static_cast<float>(B) / ext;
                const float lo = cbox.lo[a];
                auto it = std::partition(m_refs.begin() + first, m_refs.begin() + first + count, [&](const Ref& r) {
                    int k = std::min(B - 1, std::max(0, static_cast<int>((r.c[a] - lo) * scale)));
                    return k < bestBin;
                });
                mid = static_cast<uint32_t>(it - m_refs.begin());
                // the children's bounds are their bins' unions
                if (count > kSmallCount) {
                    for (int k = 0; k < B; ++k) (k < bestBin ? left : right).add(bins.k[a][k]);
                    childBounds = true;
                }
            }
            if (split && (bestAxis < 0 || mid == first || mid == first + count)) {
                medianSplit(first, count, cbox);
                mid = first + count / 2;
                childBounds = false;
            }
        } else {
            if (static_cast<int>(count) <= maxLeaf) split = false;
            else medianSplit(first, count, cbox);
        }
        if (!split) return makeLeaf(first, count, box);

        const uint32_t local = forcedLocal >= 0 ? static_cast<uint32_t>(forcedLocal) : m_nodeCount.fetch_add(1);
        Range l, r;
        const uint32_t nl = mid - first, nr = first + count - mid;
        if (!childBounds) {
            left = binRange(first, nl, nullptr, nullptr);
            right = binRange(mid, nr, nullptr, nullptr);
        }
        bool spawned = false;
        if (count > 65536) {
            int avail = m_threadsAvail.fetch_sub(1);
            if (avail > 0) {
                spawned = true;
                std::thread t([&] { l = buildRange(first, nl, depth + 1, left.b, left.c); });
                r = buildRange(mid, nr, depth + 1, right.b, right.c);
                t.join();
            }
            m_threadsAvail.fetch_add(1);
        }
        if (!spawned) {
            l = buildRange(first, nl, depth + 1, left.b, left.c);
            r = buildRange(mid, nr, depth + 1, right.b, right.c);
        }
        writeNode(local, l.box, l.code, r.box, r.code);
        return Range { static_cast<int32_t>(m_nodeBase + local), box };
    }

    static constexpr uint32_t kSmallCount = 48;
    void bestSmallSplit(uint32_t first, uint32_t count, const Aabb& cbox, int B, float& bestCost, int& bestAxis, int& bestBin) const
    {
        for (int a = 0; a < 3; ++a) {
            const float ext = cbox.hi[a] - cbox.lo[a];
            if (!(ext > 0.0f)) continue;
            const float scale = static_cast<float>(B) / ext;
            int key[kSmallCount];
            uint32_t ord[kSmallCount];
            for (uint32_t i = 0; i < count; ++i) {
                key[i] = std::min(B - 1, std::max(0, static_cast<int>((m_refs[first + i].c[a] - cbox.lo[a]) * scale)));
                ord[i] = i;
            }
            std::sort(ord, ord + count, [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
            // prefix boxes over the occupied bins in ascending order
            Aabb pre[kSmallCount];
            Aabb acc;
            for (uint32_t j = 0; j < count; ++j) {
                acc.grow(m_refs[first + ord[j]].box);
                pre[j] = acc;
            }
            Aabb accR;
            for (uint32_t j = count; j-- > 0;) {
                accR.grow(m_refs[first + ord[j]].box);
                // a candidate split at k = key of the first reference of a bin run
                if (j == 0 || key[ord[j - 1]] == key[ord[j]]) continue;
                const uint32_t nl = j, nr = count - j;
                const float cost = pre[j - 1].area(m_opt.area_w) * nl + accR.area(m_opt.area_w) * nr;
                if (cost < bestCost) {
                    bestCost = cost;
                    bestAxis = a;
                    bestBin = key[ord[j]];
                }
            }
        }
    }

    void medianSplit(uint32_t first, uint32_t count, const Aabb& cbox)
    {
        int a = 0;
        float e0 = cbox.hi[0] - cbox.lo[0], e1 = cbox.hi[1] - cbox.lo[1], e2 = cbox.hi[2] - cbox.lo[2];
        if (e1 > e0 && e1 >= e2) a = 1;
        else if (e2 > e0 && e2 > e1) a = 2;
        std::nth_element(m_refs.begin() + first, m_refs.begin() + first + count / 2, m_refs.begin() + first + count,
                         [&](const Ref& x, const Ref& y) { return x.c[a] < y.c[a]; });
    }

    Range makeLeaf(uint32_t first, uint32_t count, const Aabb& box)
    {
        // (two split references of one triangle in one leaf stay two records: the
        // collapse merges leaves as contiguous ranges of the leaf order, so a leaf
        // range must not leave a gap)
        uint32_t ml = m_maxLeaf.load();
        while (count > ml && !m_maxLeaf.compare_exchange_weak(ml, count)) {}
        return Range { leafCode(first, count), box };
    }

    const BvhBuildOptions m_opt;
    const uint32_t m_nodeBase, m_triBase;
    std::vector<Ref> m_refs; // partitioned in place: leaf order at the end
    std::unique_ptr<GpuBvhNode[]> m_nodes;
    int m_threads = 1;
    std::atomic<uint32_t> m_nodeCount { 0 };
    std::atomic<int> m_maxDepth { 0 };
    std::atomic<uint32_t> m_maxLeaf { 0 };
    std::atomic<int> m_threadsAvail { 0 };
};

// --- 8-wide collapse -------------------------------------------------------------

struct Child8 {
    int32_t code; // BVH2 child code: >= 0 internal node, < 0 leaf
    Aabb box;
};

void childrenOf(const GpuBvhNode& nd, Child8 out[2], int& n)
{
    n = 0;
    const float lo[2][3] = { { nd.n0[0], nd.n0[2], nd.n2[0] }, { nd.n1[0], nd.n1[2], nd.n2[2] } };
    const float hi[2][3] = { { nd.n0[1], nd.n0[3], nd.n2[1] }, { nd.n1[1], nd.n1[3], nd.n2[3] } };
    for (int c = 0; c < 2; ++c) {
        if (lo[c][0] > 1e29f) continue; // far sentinel of a single-leaf root
        Child8& ch = out[n++];
        ch.code = nd.child[c];
        for (int a = 0; a < 3; ++a) {
            ch.box.lo[a] = lo[c][a];
            ch.box.hi[a] = hi[c][a];
        }
    }
}

// Grid for one axis of a node box [L, H]: step 2^e, anchor p = k * 2^e <= L with
// p + 255 * 2^e >= H and |k| + 256 < 2^24 (every plane p + q * 2^e exact in fp32).
void quantGrid(float L, float H, int& e, double& p)
{
    const double ext = static_cast<double>(H) - static_cast<double>(L);
    e = ext > 0.0 ? static_cast<int>(std::ceil(std::log2(ext / 255.0))) : -100;
    e = std::max(-100, e);
    for (;; ++e) {
        const double step = std::ldexp(1.0, e);
        const double k = std::floor(static_cast<double>(L) / step);
        if (std::fabs(k) + 256.0 >= 16777216.0) continue;
        p = k * step;
        if (p + 255.0 * step < static_cast<double>(H)) continue;
        return;
    }
}

// First-fit placement of a node's leaf-triangle rows (a 24-bit pattern over
// positions base + 0..23) into the triangle array: the lowest base, at most
// kRowWindow below the end of the array, whose positions are all free. The search
// is bounded, so the collapse stays linear; rows of neighbouring nodes interleave.
class RowPlacer {
public:
    uint32_t place(uint32_t pattern)
    {
        constexpr uint32_t back = kRowWindow;
        uint32_t lo = m_end > back ? m_end - back : 0u;
        // every position below m_firstFree is taken, so no base whose lowest pattern
        // position falls below it fits: the same first fit, without re-testing the
        // filled front of the window for every node (C4 collapse 6.5 -> s)
        const uint32_t low = static_cast<uint32_t>(__builtin_ctz(pattern));
        if (m_firstFree > low) lo = std::max(lo, m_firstFree - low);
        for (uint32_t b = lo;; ++b)
            if ((window(b) & pattern) == 0) {
                mark(b, pattern);
                while (taken(m_firstFree)) ++m_firstFree;
                return b;
            }
    }

private:
    static constexpr uint32_t kRowWindow = 512;
    uint64_t window(uint32_t b) const // occupancy of positions b .. b + 23
    {
        const size_t i = b >> 6;
        const uint32_t sh = b & 63u;
        uint64_t w = i < m_bits.size() ? m_bits[i] >> sh : 0u;
        if (sh && i + 1 < m_bits.size()) w |= m_bits[i + 1] << (64u - sh);
        return w & 0xffffffu;
    }
    void mark(uint32_t b, uint32_t pattern)
    {
        const size_t i = b >> 6;
        const uint32_t sh = b & 63u;
        if (m_bits.size() < i + 2) m_bits.resize(i + 2, 0u);
        m_bits[i] |= static_cast<uint64_t>(pattern) << sh;
        if (sh > 40u) m_bits[i + 1] |= static_cast<uint64_t>(pattern) >> (64u - sh);
        m_end = std::max(m_end, b + 32u - static_cast<uint32_t>(__builtin_clz(pattern)));
    }
    bool taken(uint32_t p) const { return (p >> 6) < m_bits.size() && ((m_bits[p >> 6] >> (p & 63u)) & 1u); }
    std::vector<uint64_t> m_bits;
    uint32_t m_end = 0;
    uint32_t m_firstFree = 0; // lowest position not taken
};

// The smallest row stride (GpuBvh8Node) under which every position s + stride * i
// (i < 3) of a leaf slot s is free or s's own triangle i, so a hit leaf slot's
// spread never reaches another slot's triangle, and the rows fit in 24 positions.
uint32_t leafRowStride(const uint32_t cnt[8])
{
    for (uint32_t st = 1u; st < 8; ++st) {
        int owner[24];
        for (int& o : owner) o = -1;
        bool ok = true;
        for (uint32_t s = 0; s < 8 && ok; ++s)
            for (uint32_t i = 0; i < cnt[s] && ok; ++i) {
                const uint32_t p = s + st * i;
                ok = p < 24u && owner[p] < 0;
                if (ok) owner[p] = static_cast<int>(s);
            }
        for (uint32_t s = 0; s < 8 && ok; ++s)
            if (cnt[s])
                for (uint32_t i = 0; i < 3u && ok; ++i) {
                    const uint32_t p = s + st * i;
                    ok = p >= 24u || owner[p] < 0 || owner[p] == static_cast<int>(s);
                }
        if (ok) return st;
    }
    return 8u;
}

} // namespace

// bvh_internal.h: the node writer
void writeNodePlanes(GpuBvh8Node& nd, const Aabb& box, const Aabb* const slotBox[8])
{
    double step[3], p[3];
    for (int a = 0; a < 3; ++a) {
        int e;
        quantGrid(box.lo[a], box.hi[a], e, p[a]);
        step[a] = std::ldexp(1.0, e);
        nd.p[a] = static_cast<float>(p[a]);
        nd.e[a] = static_cast<uint8_t>(e + 127);
    }
    for (int s = 0; s < 8; ++s) {
        if (!slotBox[s]) continue;
        const Aabb& b = *slotBox[s];
        for (int a = 0; a < 3; ++a) {
            double ql = std::floor((static_cast<double>(b.lo[a]) - p[a]) / step[a]);
            double qh = std::ceil((static_cast<double>(b.hi[a]) - p[a]) / step[a]);
            ql = std::min(255.0, std::max(0.0, ql));
            qh = std::min(255.0, std::max(0.0, qh));
            // outward rounding, checked on the exact fp32 decode
            while (ql > 0.0 && static_cast<double>(static_cast<float>(p[a] + ql * step[a])) > b.lo[a]) ql -= 1.0;
            while (qh < 255.0 && static_cast<double>(static_cast<float>(p[a] + qh * step[a])) < b.hi[a]) qh += 1.0;
            nd.qlo[a][s] = static_cast<uint8_t>(ql);
            nd.qhi[a][s] = static_cast<uint8_t>(qh);
        }
    }
}

// bvh_internal.h: Builder::writeNode's inflation of a child box
void inflateChildBox(Aabb& b, float inflateAbs)
{
    float m = 0.0f, e = 0.0f;
    for (int a = 0; a < 3; ++a) {
        m = std::max(m, std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
        e = std::max(e, b.hi[a] - b.lo[a]);
    }
    const float eps = m * 2e-6f + e * 1e-5f + 1e-7f + inflateAbs;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] -= eps;
        b.hi[a] += eps;
    }
}

GpuTriangle make_gpu_triangle(const BuildTriangle& t)
{
    GpuTriangle g;
    float e1[3], e2[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = t.v1[a] - t.v0[a];
        e2[a] = t.v2[a] - t.v0[a];
    }
    g.t0[0] = t.v0[0]; g.t0[1] = t.v0[1]; g.t0[2] = t.v0[2]; g.t0[3] = e1[0];
    g.t1[0] = e1[1]; g.t1[1] = e1[2]; g.t1[2] = e2[0]; g.t1[3] = e2[1];
    g.t2[0] = e2[2];
    std::memcpy(&g.t2[1], &t.instance, 4);
    std::memcpy(&g.t2[2], &t.primitive, 4);
    std::memcpy(&g.t2[3], &t.flip_facing, 4);
    return g;
}

GpuTriangle holeTriangle()
{
    GpuTriangle t;
    std::memset(&t, 0, sizeof(t));
    std::memcpy(&t.t2[1], &kHoleInstance, 4);
    return t;
}

bool isHoleTriangle(const GpuTriangle& t)
{
    uint32_t inst;
    std::memcpy(&inst, &t.t2[1], 4);
    return inst == kHoleInstance;
}

int bvh8SlotTriangles(const GpuBvh8Node& nd, int s, uint32_t out[kBvh8MaxLeafSize])
{
    const bool leaf = (nd.leaf_mask >> s) & 1u;
    if (!leaf) return 0;
    if (((nd.imask >> s) & 1u) || nd.tri_stride < 1u || nd.tri_stride > 8u) return -1;
    int n = 0;
    bool ended = false;
    for (uint32_t i = 0; i < static_cast<uint32_t>(kBvh8MaxLeafSize); ++i) {
        const uint32_t pos = static_cast<uint32_t>(s) + nd.tri_stride * i;
        const bool set = pos < 24u && ((nd.leaf_tris >> pos) & 1u);
        if (set && ended) return -1; // the slot's spread reaches another slot's triangle
        if (!set) ended = true;
        else out[n++] = nd.tri_base + pos;
    }
    return n > 0 ? n : -1;
}

bool decodeSlotBox(const GpuBvh8Node& nd, int slot, float lo[3], float hi[3])
{
    bool exact = true;
    for (int a = 0; a < 3; ++a) {
        const float step = std::ldexp(1.0f, static_cast<int>(nd.e[a]) - 127);
        lo[a] = std::fma(static_cast<float>(nd.qlo[a][slot]), step, nd.p[a]);
        hi[a] = std::fma(static_cast<float>(nd.qhi[a][slot]), step, nd.p[a]);
        if (static_cast<double>(lo[a]) != static_cast<double>(nd.p[a]) + nd.qlo[a][slot] * static_cast<double>(step)) exact = false;
        if (static_cast<double>(hi[a]) != static_cast<double>(nd.p[a]) + nd.qhi[a][slot] * static_cast<double>(step)) exact = false;
    }
    return exact;
}

std::vector<BuildTriangle> soupTriangles(const float* triangles, uint64_t n)
{
    std::vector<BuildTriangle> tris(n);
    for (uint64_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) {
            tris[i].v0[a] = triangles[9 * i + a];
            tris[i].v1[a] = triangles[9 * i + 3 + a];
            tris[i].v2[a] = triangles[9 * i + 6 + a];
        }
        tris[i].instance = tris[i].flip_facing = 0;
        tris[i].primitive = static_cast<uint32_t>(i);
    }
    return tris;
}

float bvh8_inflation(const float* xyz, uint64_t nTriangles)
{
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint64_t i = 0; i < nTriangles * 3; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], xyz[3 * i + a]);
            hi[a] = std::max(hi[a], xyz[3 * i + a]);
        }
    return bvh8_inflation_box(lo, hi);
}

float bvh8_inflation_box(const float lo[3], const float hi[3])
{
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a)
        if (hi[a] >= lo[a]) d2 += (static_cast<double>(hi[a]) - lo[a]) * (static_cast<double>(hi[a]) - lo[a]);
    return static_cast<float>(1e-6 * std::sqrt(d2));
}

// SAH-optimal collapse plan (Ylitie, Karras, Laine 2017, "Efficient incoherent ray
// traversal on GPUs through compressed wide BVHs", §3.1). For every BVH2 internal
// node n and i = 1..8: cost[n][i] = the least SAH cost of the subtree below n when it
// is represented by at most i children of a BVH8 node - n itself as one BVH8 node
// (A(n) Cnode + its best 8-way distribution) or one leaf slot (A(n) Ctri T(n), when its
// T(n) <= kBvh8MaxLeafSize triangles, contiguous in leaf order), or its two subtrees
// sharing the i slots. Leaf children of the BVH2 stay leaves (A Ctri count).
struct CollapsePlan {
    std::vector<float> cost;    // [node][8]
    std::vector<uint8_t> pick;  // [node][8]: i = 1: 0 node, 1 leaf; i >= 2: 0 = as i - 1, else k slots to the left child
    std::vector<uint32_t> first, count; // triangle range of the subtree (leaf order)
    float cNode = 1.0f, cTri = 1.0f;
    float areaW[3] = { 1.0f, 1.0f, 1.0f };
};

float childCost(const CollapsePlan& P, const Child8& c, int i)
{
    if (c.code >= 0) return P.cost[8u * static_cast<uint32_t>(c.code) + (i - 1)];
    return P.cTri * c.box.area(P.areaW) * static_cast<float>((static_cast<uint32_t>(~c.code) & (kMaxLeafSize - 1)) + 1);
}

// The plan of BVH2 node k from its children's (planCollapse).
void planNode(const BvhBuildResult& bvh2, CollapsePlan& P, size_t k)
{
    const float cNode = P.cNode, cTri = P.cTri;
    {
        Child8 ch[2];
        int m = 0;
        childrenOf(bvh2.nodes[k], ch, m);
        uint32_t lo = UINT32_MAX, tot = 0;
        for (int c = 0; c < m; ++c) {
            if (ch[c].code >= 0) {
                lo = std::min(lo, P.first[ch[c].code]);
                tot += P.count[ch[c].code];
            } else {
                const uint32_t code = static_cast<uint32_t>(~ch[c].code);
                lo = std::min(lo, code >> kLeafCountBits);
                tot += (code & (kMaxLeafSize - 1)) + 1u;
            }
        }
        P.first[k] = lo;
        P.count[k] = tot;
        Aabb box;
        for (int c = 0; c < m; ++c) box.grow(ch[c].box);
        const float area = box.area(P.areaW);
        float* C = &P.cost[8 * k];
        uint8_t* pk = &P.pick[8 * k];
        // distributions of j slots over the two subtrees
        auto dist = [&](int j, int& bestK) {
            float best = INFINITY;
            bestK = 0;
            if (m == 1) {
                bestK = j;
                return childCost(P, ch[0], j);
            }
            for (int kk = 1; kk < j; ++kk) {
                const float v = childCost(P, ch[0], kk) + childCost(P, ch[1], j - kk);
                if (v < best) {
                    best = v;
                    bestK = kk;
                }
            }
            return best;
        };
        int k8;
        const float asNode = cNode * area + dist(8, k8);
        const float asLeaf = tot <= static_cast<uint32_t>(kBvh8MaxLeafSize) ? cTri * area * static_cast<float>(tot) : INFINITY;
        C[0] = std::min(asNode, asLeaf);
        pk[0] = asLeaf < asNode ? 1 : 0;
        for (int i = 2; i <= 8; ++i) {
            int kk;
            const float d = dist(i, kk);
            if (d < C[i - 2]) {
                C[i - 1] = d;
                pk[i - 1] = static_cast<uint8_t>(kk);
            } else {
                C[i - 1] = C[i - 2];
                pk[i - 1] = 0;
            }
        }
    }
}

// Children before parents: the subtrees of the top levels on their own threads (each
// node's plan reads only its children's), identical to a sweep in decreasing index.
void planSubtree(const BvhBuildResult& bvh2, CollapsePlan& P, size_t k, int spawnLevels)
{
    Child8 ch[2];
    int m = 0;
    childrenOf(bvh2.nodes[k], ch, m);
    int32_t inner[2];
    int ni = 0;
    for (int c = 0; c < m; ++c)
        if (ch[c].code >= 0) inner[ni++] = ch[c].code;
    if (ni == 2 && spawnLevels > 0) {
        std::thread t([&] { planSubtree(bvh2, P, static_cast<size_t>(inner[0]), spawnLevels - 1); });
        planSubtree(bvh2, P, static_cast<size_t>(inner[1]), spawnLevels - 1);
        t.join();
    } else {
        for (int c = 0; c < ni; ++c) planSubtree(bvh2, P, static_cast<size_t>(inner[c]), spawnLevels - 1);
    }
    planNode(bvh2, P, k);
}

CollapsePlan planCollapse(const BvhBuildResult& bvh2, float cNode, float cTri, const float* areaW, int threads)
{
    CollapsePlan P;
    P.cNode = cNode;
    P.cTri = cTri;
    for (int k = 0; k < 3; ++k) P.areaW[k] = areaW[k];
    const size_t N = bvh2.nodes.size();
    P.cost.assign(8 * N, 0.0f);
    P.pick.assign(8 * N, 0);
    P.first.assign(N, 0);
    P.count.assign(N, 0);
    int levels = 0;
    for (int t = threads > 0 ? threads : static_cast<int>(std::thread::hardware_concurrency()); (1 << levels) < 2 * t && levels < 8; ++levels) {}
    if (N > (1u << 16)) planSubtree(bvh2, P, 0, levels);
    else
        for (size_t k = N; k-- > 0;) planNode(bvh2, P, k); // children have larger indices
    return P;
}

// The children the plan gives a subtree (BVH2 item `c`) when it gets `i` slots.
void emitChildren(const BvhBuildResult& bvh2, const CollapsePlan& P, const Child8& c, int i, Child8* out, int& n)
{
    if (c.code < 0) {
        out[n++] = c;
        return;
    }
    const uint32_t k = static_cast<uint32_t>(c.code);
    while (i > 1 && P.pick[8 * k + (i - 1)] == 0) --i;
    if (i == 1) {
        Child8 x = c;
        if (P.pick[8 * k] == 1) // the whole subtree as one leaf slot
            x.code = ~static_cast<int32_t>((P.first[k] << kLeafCountBits) | (P.count[k] - 1u));
        out[n++] = x;
        return;
    }
    Child8 two[2];
    int m = 0;
    childrenOf(bvh2.nodes[k], two, m);
    const int kk = P.pick[8 * k + (i - 1)];
    if (m == 1) {
        emitChildren(bvh2, P, two[0], i, out, n);
        return;
    }
    emitChildren(bvh2, P, two[0], kk, out, n);
    emitChildren(bvh2, P, two[1], i - kk, out, n);
}

namespace {
struct CollapseItem {
    uint32_t src;   // BVH2 node
    uint32_t dst;   // BVH8 node (index in its part)
    uint32_t depth;
};

// One part of a collapse: the BVH8 nodes of a subtree (or of the top levels) in BFS
// order with part-local child and triangle indices, its triangle rows.
struct CollapsePart {
    std::vector<GpuBvh8Node> nodes;
    std::vector<GpuTriangle> tris;
    RowPlacer rows;
    uint32_t max_depth = 0;
    uint32_t leaf_children = 0;
    uint64_t triangles = 0;
    double sah = 0.0;
};

// Collapses the queue's items breadth first into `out`; items deeper than stopDepth go
// to `frontier` unprocessed (their node slots are allocated).
void collapseQueue(const BvhBuildResult& bvh2, const CollapsePlan& plan, const Bvh8CollapseOptions& copt, double& rootArea, CollapsePart& out,
                   std::vector<CollapseItem> queue, uint32_t stopDepth, std::vector<CollapseItem>* frontier)
{
    for (size_t qi = 0; qi < queue.size(); ++qi) {
        const CollapseItem it = queue[qi];
        if (it.depth > stopDepth) {
            frontier->push_back(it);
            continue;
        }
        const bool isRoot = frontier && qi == 0; // the top part's first item is the BVH's root
        out.max_depth = std::max(out.max_depth, it.depth);
        Child8 ch[8];
        int n = 0;
        if (copt.sah_optimal) {
            // the plan's best 8-way distribution below this node
            Child8 two[2];
            int m = 0;
            childrenOf(bvh2.nodes[it.src], two, m);
            if (m == 1) {
                emitChildren(bvh2, plan, two[0], 8, ch, n);
            } else {
                int kk = 1;
                float best = INFINITY;
                for (int k = 1; k < 8; ++k) {
                    const float v = childCost(plan, two[0], k) + childCost(plan, two[1], 8 - k);
                    if (v < best) {
                        best = v;
                        kk = k;
                    }
                }
                emitChildren(bvh2, plan, two[0], kk, ch, n);
                emitChildren(bvh2, plan, two[1], 8 - kk, ch, n);
            }
        } else {
            // gather up to 8 children: open the largest-area internal child first
            {
                Child8 two[2];
                int m = 0;
                childrenOf(bvh2.nodes[it.src], two, m);
                for (int c = 0; c < m; ++c) ch[n++] = two[c];
            }
            for (;;) {
                int best = -1;
                float bestArea = -1.0f;
                for (int c = 0; c < n; ++c)
                    if (ch[c].code >= 0 && ch[c].box.area() > bestArea) {
                        bestArea = ch[c].box.area();
                        best = c;
                    }
                if (best < 0) break;
                Child8 two[2];
                int m = 0;
                childrenOf(bvh2.nodes[ch[best].code], two, m);
                if (n - 1 + m > 8) break;
                ch[best] = two[0];
                for (int c = 1; c < m; ++c) ch[n++] = two[c];
                if (m == 0) ch[best] = ch[--n];
            }
        }
        // octant slots: greedy on the alignment of child centre offsets with slot signs
        Aabb box;
        for (int c = 0; c < n; ++c) box.grow(ch[c].box);
        // SAH cost of the result (node cost 1, the plan's triangle cost), for reports
        if (isRoot) {
            rootArea = std::max(1e-30, static_cast<double>(box.area()));
            out.sah += 1.0;
        }
        for (int c = 0; c < n; ++c) {
            const double a = ch[c].box.area() / rootArea;
            out.sah += ch[c].code >= 0 ? a : a * copt.tri_cost * static_cast<double>((static_cast<uint32_t>(~ch[c].code) & (kMaxLeafSize - 1)) + 1);
        }
        float pc[3];
        for (int a = 0; a < 3; ++a) pc[a] = 0.5f * (box.lo[a] + box.hi[a]);
        struct Cand {
            float score;
            int c, s;
        };
        // Internal children take their octant slots first; leaf children only decide
        // which triangles a hit slot adds (their order does not matter), so they fill
        // the remaining slots in ascending order, most triangles first, which keeps a
        // node's triangle rows compact (leafRowStride; leaves competing for octant slots
        // like internal children measured no better, round 3).
        constexpr bool leafOctant = false;
        Cand cand[64];
        int nc = 0;
        int slotOf[8], childIn[8];
        for (int k = 0; k < 8; ++k) slotOf[k] = childIn[k] = -1;
        if (copt.slot_sort_axis >= 0 && copt.slot_sort_axis < 3) {
            // one ray direction (+axis): internal children in slots 0, 1, ... by the
            // lower bound of their box along it, the order a ray from below meets them
            const int ax = copt.slot_sort_axis;
            int internal[8], ni = 0;
            for (int c = 0; c < n; ++c)
                if (ch[c].code >= 0 || leafOctant) internal[ni++] = c;
            std::stable_sort(internal, internal + ni, [&](int a, int b) { return ch[a].box.lo[ax] < ch[b].box.lo[ax]; });
            for (int k = 0; k < ni; ++k) {
                slotOf[internal[k]] = k;
                childIn[k] = internal[k];
            }
        } else {
            for (int c = 0; c < n; ++c)
                for (int s = 0; s < 8; ++s) {
                    if (!leafOctant && ch[c].code < 0) break;
                    float sc = 0.0f;
                    for (int a = 0; a < 3; ++a) {
                        const float off = 0.5f * (ch[c].box.lo[a] + ch[c].box.hi[a]) - pc[a];
                        sc += ((s >> a) & 1) ? off : -off;
                    }
                    cand[nc++] = { sc, c, s };
                }
            std::stable_sort(cand, cand + nc, [](const Cand& x, const Cand& y) { return x.score > y.score; });
            for (int k = 0; k < nc; ++k)
                if (slotOf[cand[k].c] < 0 && childIn[cand[k].s] < 0) {
                    slotOf[cand[k].c] = cand[k].s;
                    childIn[cand[k].s] = cand[k].c;
                }
        }
        if (!leafOctant) {
            int leaves[8], nl = 0;
            for (int c = 0; c < n; ++c)
                if (ch[c].code < 0) leaves[nl++] = c;
            auto cnt = [&](int c) { return (static_cast<uint32_t>(~ch[c].code) & (kMaxLeafSize - 1)) + 1u; };
            std::stable_sort(leaves, leaves + nl, [&](int a, int b) { return cnt(a) > cnt(b); });
            int sl = 0;
            for (int i = 0; i < nl; ++i) {
                while (childIn[sl] >= 0) ++sl;
                slotOf[leaves[i]] = sl;
                childIn[sl] = leaves[i];
            }
        }
        // quantization grid of this node, the planes of its children
        GpuBvh8Node nd;
        std::memset(&nd, 0, sizeof(nd));
        {
            const Aabb* slotBox[8];
            for (int s = 0; s < 8; ++s) slotBox[s] = childIn[s] >= 0 ? &ch[childIn[s]].box : nullptr;
            writeNodePlanes(nd, box, slotBox);
        }
        // children in slot order: internal ones get consecutive node indices; leaf
        // triangle i of slot s goes to position s + stride * i (GpuBvh8Node), the
        // rows placed at the first base in the tail of the array where all of their
        // positions are free
        const uint32_t childBase = static_cast<uint32_t>(out.nodes.size());
        uint32_t leafCnt[8] = {}, leafMask = 0;
        for (int s = 0; s < 8; ++s) {
            const int c = childIn[s];
            if (c < 0 || ch[c].code >= 0) continue;
            leafCnt[s] = (static_cast<uint32_t>(~ch[c].code) & (kMaxLeafSize - 1)) + 1u;
            leafMask |= 1u << s;
        }
        const uint32_t stride = leafRowStride(leafCnt);
        uint32_t rows = 0;
        for (uint32_t s = 0; s < 8; ++s)
            for (uint32_t i = 0; i < leafCnt[s]; ++i) rows |= 1u << (s + stride * i);
        const uint32_t triStart = rows ? out.rows.place(rows) : 0u;
        if (rows && out.tris.size() < triStart + 24u) out.tris.resize(triStart + 24u, holeTriangle());
        nd.child_base = childBase; // local: offset when the parts are joined
        nd.tri_base = triStart;
        nd.leaf_tris = rows;
        nd.tri_stride = static_cast<uint8_t>(stride);
        nd.leaf_mask = static_cast<uint8_t>(leafMask);
        uint32_t nInternal = 0;
        for (int s = 0; s < 8; ++s) {
            const int c = childIn[s];
            if (c < 0) continue;
            const Child8& k = ch[c];
            if (k.code >= 0) {
                nd.imask |= static_cast<uint8_t>(1u << s);
                queue.push_back({ static_cast<uint32_t>(k.code), childBase + nInternal, it.depth + 1 });
                nInternal++;
            } else {
                const uint32_t code = static_cast<uint32_t>(~k.code);
                const uint32_t first = code >> kLeafCountBits, cnt = (code & (kMaxLeafSize - 1)) + 1u;
                for (uint32_t i = 0; i < cnt; ++i) out.tris[triStart + static_cast<uint32_t>(s) + stride * i] = bvh2.tris[first + i];
                out.leaf_children++;
                out.triangles += cnt;
            }
        }
        out.nodes.resize(out.nodes.size() + nInternal);
        out.nodes[it.dst] = nd;
    }
}
} // namespace

// The top levels (BVH8 depth <= kTopDepth) are collapsed first, then the subtrees below
// them in parallel, each a part with its own node and triangle-row arrays, joined in
// order: the top levels stay breadth first at the front (k_trace_shadow caches the
// first nodes in LDS), every subtree is breadth first in its block. (One sequential
// breadth-first pass took 6.2 s of a C4 build; the plan's DP is shared.)
Bvh8BuildResult collapse_bvh8(const BvhBuildResult& bvh2, uint32_t node_base, uint32_t tri_base, const Bvh8CollapseOptions& copt)
{
    Bvh8BuildResult res;
    if (bvh2.nodes.empty()) return res;
    CollapsePlan plan;
    if (copt.sah_optimal) plan = planCollapse(bvh2, copt.node_cost, copt.tri_cost, copt.area_w, copt.threads);
    constexpr uint32_t kTopDepth = 3;
    double rootArea = 0.0;
    CollapsePart top;
    top.nodes.resize(1);
    std::vector<CollapseItem> frontier;
    collapseQueue(bvh2, plan, copt, rootArea, top, { { 0u, 0u, 1u } }, kTopDepth, &frontier);
    std::vector<CollapsePart> parts(frontier.size());
    {
        const int hw = copt.threads > 0 ? copt.threads : static_cast<int>(std::thread::hardware_concurrency());
        const int T = std::max(1, std::min<int>(hw, static_cast<int>(frontier.size())));
        std::atomic<size_t> next { 0 };
        auto worker = [&] {
            for (size_t f; (f = next.fetch_add(1)) < frontier.size();) {
                parts[f].nodes.resize(1);
                double ra = rootArea;
                collapseQueue(bvh2, plan, copt, ra, parts[f], { { frontier[f].src, 0u, frontier[f].depth } }, UINT32_MAX, nullptr);
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(worker);
        worker();
        for (std::thread& th : pool) th.join();
    }
    // join: subtree f's root fills its frontier slot of the top part, its other nodes
    // follow the top part's nodes; its rows follow the top part's rows
    auto trimHoles = [](std::vector<GpuTriangle>& t) {
        while (!t.empty() && isHoleTriangle(t.back())) t.pop_back();
    };
    trimHoles(top.tris);
    size_t nodeCount = top.nodes.size(), triCount = top.tris.size();
    std::vector<size_t> nodeOff(parts.size()), triOff(parts.size());
    for (size_t f = 0; f < parts.size(); ++f) {
        trimHoles(parts[f].tris);
        nodeOff[f] = nodeCount;
        triOff[f] = triCount;
        nodeCount += parts[f].nodes.size() - 1;
        triCount += parts[f].tris.size();
    }
    res.nodes.resize(nodeCount);
    res.tris.reserve(triCount);
    auto place = [&](GpuBvh8Node nd, size_t nodeShift, size_t triShift) {
        nd.child_base = node_base + static_cast<uint32_t>(nd.child_base + nodeShift);
        nd.tri_base = tri_base + static_cast<uint32_t>(nd.leaf_tris ? nd.tri_base + triShift : 0u);
        return nd;
    };
    for (size_t k = 0; k < top.nodes.size(); ++k) res.nodes[k] = place(top.nodes[k], 0, 0);
    res.tris.insert(res.tris.end(), top.tris.begin(), top.tris.end());
    res.max_depth = top.max_depth;
    res.leaf_children = top.leaf_children;
    res.triangles = top.triangles;
    double sah = top.sah;
    for (size_t f = 0; f < parts.size(); ++f) {
        const CollapsePart& P = parts[f];
        // part-local node k >= 1 -> nodeOff + k - 1 (its children are all >= 1)
        const size_t shift = nodeOff[f] - 1;
        res.nodes[frontier[f].dst] = place(P.nodes[0], shift, triOff[f]);
        for (size_t k = 1; k < P.nodes.size(); ++k) res.nodes[shift + k] = place(P.nodes[k], shift, triOff[f]);
        res.tris.insert(res.tris.end(), P.tris.begin(), P.tris.end());
        res.max_depth = std::max(res.max_depth, P.max_depth);
        res.leaf_children += P.leaf_children;
        res.triangles += P.triangles;
        sah += P.sah;
    }
    res.sah_cost = static_cast<float>(sah);
    return res;
}

BvhBuildResult build_bvh(const std::vector<BuildTriangle>& tris, const BvhBuildOptions& opt, uint32_t node_base, uint32_t tri_base)
{
    if (tris.empty()) return {};
    Builder b(tris, opt, node_base, tri_base);
    return b.run(tris);
}

int hit_mask_class(uint32_t hit_mask) { return (hit_mask & ARK_RT_HIT_MASK_OPAQUE) ? 0 : (hit_mask & ARK_RT_HIT_MASK_MASKED) ? 1 : 2; }

bool checkBvh8Structure(const std::vector<GpuBvh8Node>& allNodes, const std::vector<GpuTriangle>& allTris, const int32_t* roots, int nRoots, std::string& why)
{
    char buf[128];
    auto bad = [&](const char* fmt, uint64_t v) {
        std::snprintf(buf, sizeof(buf), fmt, static_cast<unsigned long long>(v));
        why = buf;
        return false;
    };
    std::vector<uint8_t> seenNode(allNodes.size(), 0);
    std::vector<uint8_t> seenTri(allTris.size(), 0);
    std::vector<uint32_t> work;
    for (int c = 0; c < nRoots; ++c)
        if (roots[c] >= 0) work.push_back(static_cast<uint32_t>(roots[c]));
    while (!work.empty()) {
        const uint32_t n = work.back();
        work.pop_back();
        if (n >= allNodes.size() || seenNode[n]) return bad("BVH invalid: node %llu", n);
        seenNode[n] = 1;
        const GpuBvh8Node& nd = allNodes[n];
        uint32_t internal = 0;
        if ((nd.leaf_tris >> 24) || (nd.leaf_mask & nd.imask)) return bad("BVH invalid: node %llu leaf rows", n);
        for (int sl = 0; sl < 8; ++sl) {
            const bool isInternal = (nd.imask >> sl) & 1u;
            uint32_t slotTris[kBvh8MaxLeafSize];
            const int cnt = bvh8SlotTriangles(nd, sl, slotTris);
            if (cnt < 0) return bad("BVH invalid: node %llu slot", n);
            if (isInternal) work.push_back(nd.child_base + internal++);
            for (int i = 0; i < cnt; ++i) {
                const uint32_t t = slotTris[i];
                if (t >= allTris.size() || isHoleTriangle(allTris[t])) return bad("BVH invalid: leaf range%.0llu", 0);
                if (seenTri[t]) return bad("BVH invalid: triangle %llu in two leaves", t);
                seenTri[t] = 1;
            }
            for (int a = 0; a < 3; ++a)
                if ((isInternal || cnt > 0) && nd.qlo[a][sl] > nd.qhi[a][sl]) return bad("BVH invalid: child box%.0llu", 0);
        }
    }
    for (size_t t = 0; t < seenTri.size(); ++t)
        if (!seenTri[t] && !isHoleTriangle(allTris[t])) return bad("BVH invalid: triangle %llu unreachable", t);
    return true;
}

bool bvhLevelOrder(const GpuBvh8Node* h, uint64_t n, const int32_t* roots, int nRoots, std::vector<uint32_t>& order, std::vector<uint32_t>& offsets)
{
    std::vector<std::vector<uint32_t>> byDepth;
    std::vector<std::pair<uint32_t, uint32_t>> work; // (node, depth)
    for (int r = 0; r < nRoots; ++r)
        if (roots[r] >= 0) work.push_back({ static_cast<uint32_t>(roots[r]), 0u });
    while (!work.empty()) {
        const auto [node, d] = work.back();
        work.pop_back();
        if (node >= n) return false;
        if (byDepth.size() <= d) byDepth.resize(d + 1);
        byDepth[d].push_back(node);
        const uint32_t internal = static_cast<uint32_t>(__builtin_popcount(h[node].imask));
        for (uint32_t k = 0; k < internal; ++k) work.push_back({ h[node].child_base + k, d + 1 });
    }
    order.clear();
    order.reserve(n);
    offsets.assign(1, 0u);
    for (size_t d = byDepth.size(); d-- > 0;) {
        std::sort(byDepth[d].begin(), byDepth[d].end());
        order.insert(order.end(), byDepth[d].begin(), byDepth[d].end());
        offsets.push_back(static_cast<uint32_t>(order.size()));
    }
    return true;
}

bool build_world_bvh8(std::vector<BuildTriangle> cls[3], BvhBuildOptions opt, const Bvh8CollapseOptions& copt, WorldBvh8& out, std::string& why)
{
    out = WorldBvh8 {};
    opt.max_leaf_size = kBvh8MaxLeafSize;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int c = 0; c < 3; ++c)
        for (const BuildTriangle& t : cls[c])
            for (const float* v : { t.v0, t.v1, t.v2 })
                for (int a = 0; a < 3; ++a) {
                    lo[a] = std::min(lo[a], v[a]);
                    hi[a] = std::max(hi[a], v[a]);
                }
    out.inflateAbs = opt.inflate_abs = bvh8_inflation_box(lo, hi);
    for (int c = 0; c < 3; ++c) {
        if (cls[c].empty()) continue;
        BvhBuildResult r2 = build_bvh(cls[c], opt, 0u, 0u);
        std::vector<BuildTriangle>().swap(cls[c]);
        out.maxLeaf = std::max(out.maxLeaf, r2.max_leaf);
        if (r2.max_leaf > static_cast<uint32_t>(kBvh8MaxLeafSize)) {
            why = "BVH2 leaf of " + std::to_string(r2.max_leaf) + " triangles";
            return false;
        }
        if (c == 0) out.sah = r2.sah_cost;
        Bvh8BuildResult r = collapse_bvh8(r2, static_cast<uint32_t>(out.nodes.size()), static_cast<uint32_t>(out.tris.size()), copt);
        out.roots[c] = static_cast<int32_t>(out.nodes.size());
        if (c == 0) out.opaqueNodes = static_cast<uint32_t>(r.nodes.size());
        if (c == 0) out.opaqueRecords = static_cast<uint32_t>(r.tris.size());
        out.depth = std::max(out.depth, r.max_depth);
        out.triangles += r.triangles;
        out.nodes.insert(out.nodes.end(), r.nodes.begin(), r.nodes.end());
        out.tris.insert(out.tris.end(), r.tris.begin(), r.tris.end());
    }
    if (out.nodes.size() >= (1ull << 31) || out.tris.size() >= (1ull << 31)) {
        out.tooLarge = true;
        why = "scene too large for 31-bit BVH indices";
        return false;
    }
    return checkBvh8Structure(out.nodes, out.tris, out.roots, 3, why);
}

} // namespace ark
