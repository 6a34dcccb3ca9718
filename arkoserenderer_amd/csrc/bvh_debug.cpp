// bvh_debug.cpp — the host-only ark_ddgi_debug_* entry points of the BVH builds
// (include/ark_ddgi_debug.h): test support over triangle soups, no GPU.
#include "../../include/ark_ddgi_debug.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

#include "bvh8_check.h"
#include "bvh_builder.h"
#include "lbvh_host.h"
#include "sun_bvh.h"

static constexpr int kDebugThreads = 8; // the entry points' host builds and ray comparisons: a fixed thread count

// ark_ddgi_debug.h: host-side structural check of the BVH8 (see the header).
extern "C" int ark_ddgi_debug_bvh8_check(const float* triangles, uint64_t n, uint64_t* out)
{
    return ark_ddgi_debug_bvh8_check_opts(triangles, n, 1, 0.0f, out);
}

extern "C" int ark_ddgi_debug_bvh8_check_opts(const float* triangles, uint64_t n, int sah_optimal, float tri_cost, uint64_t* out)
{
    using namespace ark;
    const std::vector<BuildTriangle> tris = soupTriangles(triangles, n);
    BvhBuildOptions opt;
    opt.max_leaf_size = kBvh8MaxLeafSize;
    opt.inflate_abs = bvh8_inflation(triangles, n);
    const BvhBuildResult r2 = build_bvh(tris, opt, 0u, 0u);
    Bvh8CollapseOptions copt;
    copt.sah_optimal = sah_optimal != 0;
    if (tri_cost > 0.0f) copt.tri_cost = std::max(0.01f, tri_cost);
    const Bvh8BuildResult r8 = collapse_bvh8(r2, 0u, 0u, copt);
    const int32_t root = r8.nodes.empty() ? -1 : 0;
    const std::vector<int> classOf(1, 0);
    const Bvh8CheckResult c = check_bvh8_full(r8.nodes, r8.tris, &root, 1, &classOf, triangles);
    if (out) {
        out[0] = r8.nodes.size();
        out[1] = r8.leaf_children;
        out[2] = r8.max_depth;
        out[3] = c.violations;
        out[4] = r8.triangles;
        out[5] = r2.nodes.size();
        out[6] = c.internalChildren;
        out[7] = static_cast<uint64_t>(static_cast<double>(r8.sah_cost) * 1e6); // BVH8 SAH cost x 1e6
    }
    return c.violations == 0 ? 0 : 1;
}

// ark_ddgi_debug.h: the sun's light-space BVH on the host (no GPU), checked against
// brute force. Builds it as set_scene does (sun_frame, sun_add_triangles,
// build_sun_bvh), then for every origin traces a sun shadow ray (L = -normalize(sun
// dir) in fp32, [0.025, tmax]) twice: through the BVH with a host restatement of
// k_trace_shadow<SUN>'s node test (visitNodeSun: the same fp32 quantized coordinate,
// floor / ceil, integer plane compares) and against every triangle; both use the same
// Möller–Trumbore (the kernels' operation order). out[8] = {rays, occluded (brute
// force), occluded (BVH), mismatches, node visits, triangle tests, BVH8 nodes, max
// stack depth}. A mismatch would be a culled occluder: the node test must be
// conservative.
namespace {
// A sun shadow ray per origin traced through the light-space BVH (nodes, tris) by the host
// restatement of visitNodeSun and against every record of `world`: out[0..7] as
// ark_ddgi_debug_sun_bvh_check's; the mismatching rays returned
uint64_t sunRayCompare(const std::vector<ark::GpuBvh8Node>& nodes, const std::vector<ark::GpuTriangle>& tris, const std::vector<ark::GpuTriangle>& world,
                       const double frame[3][3], const float* sun_dir, const float* origins, uint64_t n_rays, float tmax, uint64_t* out)
{
    using namespace ark;
    float F[9];
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 3; ++k) F[a * 3 + k] = static_cast<float>(frame[a][k]);
    float L[3];
    sun_ray_dir(sun_dir, L);
    const float tmin = 0.025f;
    // the kernels' Möller–Trumbore (intersectTri: crossFma / dotFma3, 1 / det)
    auto mt = [&](const float o[3], const GpuTriangle& g) {
        const float v0[3] = { g.t0[0], g.t0[1], g.t0[2] }, e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
        auto cr = [](const float* a, const float* b, float* c) {
            c[0] = std::fma(a[1], b[2], -(a[2] * b[1]));
            c[1] = std::fma(a[2], b[0], -(a[0] * b[2]));
            c[2] = std::fma(a[0], b[1], -(a[1] * b[0]));
        };
        auto dt = [](const float* a, const float* b) { return std::fma(a[0], b[0], std::fma(a[1], b[1], a[2] * b[2])); };
        float p[3], q[3];
        cr(L, e2, p);
        const float det = dt(e1, p);
        const float inv = 1.0f / det;
        const float s[3] = { o[0] - v0[0], o[1] - v0[1], o[2] - v0[2] };
        const float u = dt(s, p) * inv;
        cr(s, e1, q);
        const float v = dt(L, q) * inv;
        const float t = dt(e2, q) * inv;
        return (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t >= tmin) & (t <= tmax);
    };
    std::atomic<uint64_t> occB { 0 }, occV { 0 }, mism { 0 }, visits { 0 }, tests { 0 }, maxDepth { 0 };
    auto worker = [&](uint64_t r0, uint64_t r1) {
        for (uint64_t ri = r0; ri < r1; ++ri) {
            const float* o = origins + 3 * ri;
            bool brute = false;
            for (const GpuTriangle& g : world)
                if (mt(o, g)) {
                    brute = true;
                    break;
                }
            // light-space traversal (visitNodeSun)
            const float pl[3] = { std::fma(o[0], F[0], std::fma(o[1], F[1], o[2] * F[2])), std::fma(o[0], F[3], std::fma(o[1], F[4], o[2] * F[5])),
                                  std::fma(o[0], F[6], std::fma(o[1], F[7], o[2] * F[8])) };
            std::vector<uint32_t> stack { 0u };
            bool bvh = false;
            uint64_t nv = 0, nt = 0, md = 0;
            while (!stack.empty() && !bvh) {
                const GpuBvh8Node& nd = nodes[stack.back()];
                stack.pop_back();
                nv++;
                int F_[2], C_[3];
                float Q[3];
                for (int a = 0; a < 3; ++a) {
                    const float q = std::ldexp(pl[a] - nd.p[a], 127 - static_cast<int>(nd.e[a]));
                    Q[a] = std::min(258.0f, std::max(-2.0f, q));
                }
                F_[0] = static_cast<int>(std::floor(Q[0]));
                F_[1] = static_cast<int>(std::floor(Q[1]));
                for (int a = 0; a < 3; ++a) C_[a] = static_cast<int>(std::ceil(Q[a]));
                uint32_t internalBefore = 0;
                std::vector<uint32_t> push;
                for (int sl = 0; sl < 8; ++sl) {
                    const bool internal = (nd.imask >> sl) & 1u;
                    const bool hitc = nd.qlo[0][sl] <= F_[0] && nd.qhi[0][sl] >= C_[0] && nd.qlo[1][sl] <= F_[1] && nd.qhi[1][sl] >= C_[1] &&
                                      nd.qhi[2][sl] >= C_[2];
                    if (internal) {
                        if (hitc) push.push_back(nd.child_base + internalBefore);
                        internalBefore++;
                        continue;
                    }
                    if (!hitc || !((nd.leaf_mask >> sl) & 1u)) continue;
                    uint32_t st[kBvh8MaxLeafSize];
                    const int cnt = bvh8SlotTriangles(nd, sl, st);
                    for (int i = 0; i < cnt && !bvh; ++i) {
                        nt++;
                        bvh = mt(o, tris[st[i]]);
                    }
                }
                for (size_t i = push.size(); i-- > 0;) stack.push_back(push[i]);
                md = std::max<uint64_t>(md, stack.size());
            }
            occB += brute ? 1 : 0;
            occV += bvh ? 1 : 0;
            mism += brute != bvh ? 1 : 0;
            visits += nv;
            tests += nt;
            uint64_t m = maxDepth.load();
            while (md > m && !maxDepth.compare_exchange_weak(m, md)) {}
        }
    };
    const int T = kDebugThreads;
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back(worker, n_rays * t / T, n_rays * (t + 1) / T);
    for (auto& th : pool) th.join();
    if (out) {
        out[0] = n_rays;
        out[1] = occB.load();
        out[2] = occV.load();
        out[3] = mism.load();
        out[4] = visits.load();
        out[5] = tests.load();
        out[6] = nodes.size();
        out[7] = maxDepth.load();
    }
    return mism.load();
}
} // namespace

extern "C" int ark_ddgi_debug_sun_bvh_check(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                             uint64_t* out)
{
    using namespace ark;
    SunBvhInput in;
    sun_frame(sun_dir, in.frame);
    sun_add_triangles(in, soupTriangles(triangles, n));
    std::vector<GpuTriangle> world = in.world;
    BvhBuildOptions opt;
    opt.threads = kDebugThreads;
    Bvh8CollapseOptions copt;
    Bvh8BuildResult r;
    if (n == 0 || !build_sun_bvh(in, opt, copt, r)) return 1;
    return sunRayCompare(r.nodes, r.tris, world, in.frame, sun_dir, origins, n_rays, tmax, out) == 0 ? 0 : 2;
}

// ark_ddgi_debug.h: set_scene's choice between the light-space BVH and the world BVH
// for the sun's shadow rays, on a triangle soup (one hit-mask class).
extern "C" int ark_ddgi_debug_sun_choice(const float* triangles, uint64_t n, const float* sun_dir, uint32_t n_samples, double* out)
{
    using namespace ark;
    if (n == 0 || !out) return 1;
    const std::vector<BuildTriangle> tris = soupTriangles(triangles, n);
    SunBvhInput in;
    sun_frame(sun_dir, in.frame);
    sun_add_triangles(in, tris);
    double frame[3][3];
    std::memcpy(frame, in.frame, sizeof(frame));
    BvhBuildOptions opt;
    opt.max_leaf_size = kBvh8MaxLeafSize;
    opt.inflate_abs = bvh8_inflation(triangles, n);
    opt.threads = kDebugThreads;
    Bvh8CollapseOptions copt;
    const BvhBuildResult r2 = build_bvh(tris, opt, 0u, 0u);
    if (r2.max_leaf > static_cast<uint32_t>(kBvh8MaxLeafSize)) return 1;
    const Bvh8BuildResult w8 = collapse_bvh8(r2, 0u, 0u, copt);
    Bvh8BuildResult s8;
    if (!build_sun_bvh(in, opt, copt, s8)) return 1;
    float L[3];
    sun_ray_dir(sun_dir, L);
    std::vector<float> origins;
    sun_sample_origins(w8.tris, L, n_samples, origins);
    const int32_t root = 0;
    out[0] = sun_shadow_cost(w8.nodes, w8.tris, &root, 1, nullptr, L, origins);
    out[1] = sun_shadow_cost(s8.nodes, s8.tris, &root, 1, frame, L, origins);
    out[2] = sun_bvh_pays(out[0], out[1]) ? 1.0 : 0.0;
    out[3] = static_cast<double>(origins.size() / 3);
    return 0;
}

// ark_ddgi_debug.h: what compare_bvh8_canonical notices, without a GPU
namespace {
using namespace ark;

struct HostTree {
    std::vector<GpuBvh8Node> nodes;
    std::vector<GpuTriangle> tris;
    std::vector<uint32_t> perm, order, levelOffsets;
    int32_t roots[3] = { -1, -1, -1 };
    uint32_t opaqueNodes = 0, depth = 0;
    Bvh8TreeView view() const
    {
        Bvh8TreeView v;
        v.nodes = &nodes;
        v.tris = &tris;
        v.perm = &perm;
        v.order = &order;
        v.levelOffsets = &levelOffsets;
        std::copy(roots, roots + 3, v.roots);
        v.opaqueNodes = opaqueNodes;
        v.depth = depth;
        return v;
    }
};

uint32_t rowSpan(const GpuBvh8Node& nd) { return nd.leaf_tris ? 32u - static_cast<uint32_t>(__builtin_clz(nd.leaf_tris)) : 0u; }

// What the device's atomics do to a tree: within each level of each class, the blocks of
// siblings (child_base) and the rows (tri_base) handed out in another order
HostTree shuffledTwin(const LbvhHostResult& r, uint64_t seed)
{
    HostTree t;
    const uint32_t N = static_cast<uint32_t>(r.nodes.size());
    uint64_t state = seed * 0x9e3779b97f4a7c15ull + 1u;
    auto rnd = [&](uint32_t n) { // xorshift64*
        state ^= state >> 12;
        state ^= state << 25;
        state ^= state >> 27;
        return static_cast<uint32_t>(((state * 0x2545f4914f6cdd1dull) >> 33) % n);
    };
    auto shuffle = [&](std::vector<uint32_t>& v) {
        for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd(static_cast<uint32_t>(i))]);
    };
    t.nodes.resize(N);
    t.tris.assign(r.tris.size(), holeTriangle());
    t.perm.assign(r.perm.size(), 0xffffffffu);
    uint32_t records = 0;
    for (int c = 0; c < 3; ++c) {
        t.roots[c] = r.roots[c];
        if (r.roots[c] < 0) continue;
        std::vector<uint32_t> level(1, static_cast<uint32_t>(r.roots[c])); // old indices, in new index order
        uint32_t levelBase = level[0];
        while (!level.empty()) {
            const uint32_t nextBase = levelBase + static_cast<uint32_t>(level.size());
            // the sibling blocks of the next level, parent by parent in a shuffled order
            std::vector<uint32_t> parents(level.size()), next;
            for (uint32_t i = 0; i < parents.size(); ++i) parents[i] = i;
            shuffle(parents);
            std::vector<uint32_t> childBase(level.size(), 0u);
            for (uint32_t i : parents) {
                const GpuBvh8Node& nd = r.nodes[level[i]];
                childBase[i] = nextBase + static_cast<uint32_t>(next.size());
                for (int k = 0; k < __builtin_popcount(nd.imask); ++k) {
                    next.push_back(nd.child_base + k);
                }
            }
            // this level's rows in another shuffled order
            shuffle(parents);
            for (uint32_t i : parents) {
                const GpuBvh8Node& nd = r.nodes[level[i]];
                GpuBvh8Node out = nd;
                out.child_base = childBase[i];
                out.tri_base = rowSpan(nd) ? records : 0u;
                for (uint32_t pos = 0; pos < rowSpan(nd); ++pos) {
                    t.tris[out.tri_base + pos] = r.tris[nd.tri_base + pos];
                    t.perm[out.tri_base + pos] = r.perm[nd.tri_base + pos];
                }
                records += rowSpan(nd);
                t.nodes[levelBase + i] = out;
            }
            levelBase = nextBase;
            level.swap(next);
        }
    }
    t.opaqueNodes = r.opaqueNodes;
    t.depth = r.depth;
    bvhLevelOrder(t.nodes.data(), t.nodes.size(), t.roots, 3, t.order, t.levelOffsets);
    return t;
}

void swapSlotPlanes(GpuBvh8Node& nd, int s1, int s2)
{
    for (int a = 0; a < 3; ++a) {
        std::swap(nd.qlo[a][s1], nd.qlo[a][s2]);
        std::swap(nd.qhi[a][s1], nd.qhi[a][s2]);
    }
}

// Applies mutation `which` (0 .. 5: ark_ddgi_debug.h's (a) .. (f)) to the first node that
// allows it; false when none does
bool mutateTree(HostTree& t, int which)
{
    if (which == 5) {
        for (uint32_t& p : t.perm)
            if (p != 0xffffffffu) {
                p ^= 1u;
                return true;
            }
        return false;
    }
    for (size_t k = 0; k < t.nodes.size(); ++k) {
        GpuBvh8Node& nd = t.nodes[k];
        const uint32_t occupied = nd.imask | nd.leaf_mask;
        int in[8], nIn = 0, leaf[8], nLeaf = 0, cnt[8];
        for (int s = 0; s < 8; ++s) {
            uint32_t tri[kBvh8MaxLeafSize];
            cnt[s] = std::max(0, bvh8SlotTriangles(nd, s, tri));
            if ((nd.imask >> s) & 1u) in[nIn++] = s;
            else if (cnt[s]) leaf[nLeaf++] = s;
        }
        if (which == 0) { // (a) one plane one quantum looser
            for (int s = 0; s < 8; ++s) {
                if (!((occupied >> s) & 1u)) continue;
                if (nd.qlo[0][s] > 0) {
                    nd.qlo[0][s]--;
                    return true;
                }
                if (nd.qhi[0][s] < 255) {
                    nd.qhi[0][s]++;
                    return true;
                }
            }
        } else if (which == 1) { // (b) one axis's grid one exponent coarser, the planes re-quantised outward
            // (p stays: it is a multiple of the old step, and every plane stays exact in
            // fp32 while |p / old step| + 512 < 2^24)
            const int a = 1;
            const double step = std::ldexp(1.0, static_cast<int>(nd.e[a]) - 127);
            if (nd.e[a] >= 250 || std::fabs(nd.p[a] / step) + 512.0 >= 16777216.0) continue;
            nd.e[a]++;
            for (int s = 0; s < 8; ++s) {
                if (!((occupied >> s) & 1u)) continue;
                nd.qlo[a][s] = static_cast<uint8_t>(nd.qlo[a][s] / 2);       // floor
                nd.qhi[a][s] = static_cast<uint8_t>((nd.qhi[a][s] + 1) / 2); // ceil
            }
            return true;
        } else if (which == 2) { // (c) two internal children exchanged, with their planes
            if (nIn < 2) continue;
            std::swap(t.nodes[nd.child_base], t.nodes[nd.child_base + 1]);
            swapSlotPlanes(nd, in[0], in[1]);
            return true;
        } else { // (d), (e): two leaf slots with as many triangles
            for (int i = 0; i < nLeaf; ++i)
                for (int j = i + 1; j < nLeaf; ++j) {
                    if (cnt[leaf[i]] != cnt[leaf[j]]) continue;
                    const int s1 = leaf[i], s2 = leaf[j];
                    // (d) every member, the rows rewritten and the planes with them;
                    // (e) one record each, both slots' planes widened to their union
                    const int members = which == 3 ? cnt[s1] : 1;
                    for (int m = 0; m < members; ++m) {
                        const uint32_t p1 = nd.tri_base + s1 + nd.tri_stride * m, p2 = nd.tri_base + s2 + nd.tri_stride * m;
                        std::swap(t.tris[p1], t.tris[p2]);
                        std::swap(t.perm[p1], t.perm[p2]);
                    }
                    if (which == 3) {
                        swapSlotPlanes(nd, s1, s2);
                    } else {
                        for (int a = 0; a < 3; ++a) {
                            nd.qlo[a][s1] = nd.qlo[a][s2] = std::min(nd.qlo[a][s1], nd.qlo[a][s2]);
                            nd.qhi[a][s1] = nd.qhi[a][s2] = std::max(nd.qhi[a][s1], nd.qhi[a][s2]);
                        }
                    }
                    return true;
                }
        }
    }
    return false;
}
} // namespace

extern "C" int ark_ddgi_debug_bvh8_compare_selftest(const float* triangles, uint64_t n, const float* sun_dir, uint64_t seed, uint64_t* out)
{
    using namespace ark;
    if (!triangles || n == 0 || !out) return -1;
    std::fill(out, out + 16, uint64_t(0));
    std::vector<BuildTriangle> tris = soupTriangles(triangles, n);
    std::vector<GpuTriangle> rec(n);
    for (uint64_t i = 0; i < n; ++i) {
        tris[i].instance = static_cast<uint32_t>(i % 3u); // three instances, one of each class
        rec[i] = make_gpu_triangle(tris[i]);
    }
    const std::vector<int> classOf = { 0, 1, 2 };
    LbvhSunOptions so;
    if (sun_dir) {
        double frame[3][3];
        sun_frame(sun_dir, frame);
        std::memcpy(so.frame, frame, sizeof(so.frame));
    }
    const LbvhHostResult r = build_lbvh_host(rec, classOf, lbvh::kDefaultCriterion, sun_dir ? &so : nullptr);
    HostTree ref;
    ref.nodes = r.nodes;
    ref.tris = r.tris;
    ref.perm = r.perm;
    ref.order = r.order;
    ref.levelOffsets = r.levelOffsets;
    std::copy(r.roots, r.roots + 3, ref.roots);
    ref.opaqueNodes = r.opaqueNodes;
    ref.depth = r.depth;
    const HostTree twin = shuffledTwin(r, seed);
    uint64_t moved = 0;
    for (size_t k = 0; k < ref.nodes.size(); ++k)
        if (ref.nodes[k].child_base != twin.nodes[k].child_base || ref.nodes[k].tri_base != twin.nodes[k].tri_base) moved++;
    const Bvh8CanonicalDiff same = compare_bvh8_canonical(ref.view(), twin.view());
    out[0] = ref.nodes.size();
    out[1] = moved;
    out[2] = same.total();
    out[3] = same.pairs;
    const Bvh8CheckResult twinCheck = check_bvh8_full(twin.nodes, twin.tris, twin.roots, 3, sun_dir ? nullptr : &classOf, nullptr, sun_dir ? so.frame : nullptr);
    out[4] = twinCheck.violations;
    int rc = same.total() == 0 && same.pairs == ref.nodes.size() && twinCheck.violations == 0 && moved > 0 ? 0 : 1;
    for (int which = 0; which < 6; ++which) {
        HostTree m = twin;
        if (!mutateTree(m, which)) {
            rc = 1;
            continue;
        }
        const Bvh8CanonicalDiff d = compare_bvh8_canonical(ref.view(), m.view());
        // the kind of difference each mutation has to show: (a) planes, (b) grid, (c) the
        // exchanged children's nodes or planes, (d), (e) records, (f) perm and nothing else
        const uint64_t kind[6] = { d.planes, d.grid, d.header + d.grid + d.planes + d.records, d.records, d.records, d.perm == d.total() ? d.perm : 0 };
        out[5 + which] = kind[which];
        if (kind[which] == 0 || d.firstA < 0) rc = 1;
        if (which < 2) {
            // (a) and (b) stay valid trees: what check_bvh8_full, the only check of a device
            // build's boxes before, could not tell from the tree the design describes
            const Bvh8CheckResult c = check_bvh8_full(m.nodes, m.tris, m.roots, 3, sun_dir ? nullptr : &classOf, nullptr, sun_dir ? so.frame : nullptr);
            out[11 + which] = c.violations;
            if (c.violations) rc = 1;
        }
    }
    return rc;
}

namespace {
int lbvhCheck(const float* triangles, uint64_t n, int criterion, bool sah, uint64_t* out, uint64_t* treelets, bool plan = false, uint64_t* planOut = nullptr)
{
    using namespace ark;
    std::vector<GpuTriangle> rec;
    for (const BuildTriangle& t : soupTriangles(triangles, n)) rec.push_back(make_gpu_triangle(t));
    const std::vector<int> classOf(1, 0);
    const LbvhHostResult r = build_lbvh_host(rec, classOf, criterion, nullptr, nullptr, sah, plan);
    if (treelets) *treelets = r.treelets.size();
    if (planOut) {
        planOut[0] = r.planRootCost;
        planOut[1] = r.smallInternal + (r.planStalled ? 1u : 0u);
    }
    Bvh8CheckResult c = check_bvh8_full(r.nodes, r.tris, r.roots, 3, &classOf, triangles);
    // every input triangle in exactly one leaf, bit for bit
    c.violations += recordViolations(r.tris, r.perm, rec);
    if (c.maxDepth != r.depth || c.nodes != r.nodes.size()) c.violations++;
    c.violations += c.notBreadthFirst;
    if (out) {
        out[0] = r.nodes.size();
        out[1] = c.leafChildren;
        out[2] = r.depth;
        out[3] = c.violations;
        out[4] = c.triangles;
        out[5] = n ? 2 * n - 1 : 0; // the radix tree's nodes
        out[6] = c.internalChildren;
        out[7] = static_cast<uint64_t>(r.sah * 1e6);
    }
    return c.violations == 0 ? 0 : 1;
}
} // namespace

extern "C" int ark_ddgi_debug_lbvh_check_opts(const float* triangles, uint64_t n, int criterion, uint64_t* out)
{
    return lbvhCheck(triangles, n, criterion, false, out, nullptr);
}

extern "C" int ark_ddgi_debug_lbvh_check_sah(const float* triangles, uint64_t n, int criterion, int sah, uint64_t* out)
{
    uint64_t treelets = 0;
    const int rc = lbvhCheck(triangles, n, criterion, sah != 0, out, &treelets);
    if (out) out[8] = treelets;
    return rc;
}

extern "C" int ark_ddgi_debug_lbvh_check_plan(const float* triangles, uint64_t n, int criterion, int sah, int plan, uint64_t* out)
{
    uint64_t treelets = 0, planWords[2] = { 0, 0 };
    int rc = lbvhCheck(triangles, n, criterion, sah != 0, out, &treelets, plan != 0, planWords);
    if (out) {
        out[8] = treelets;
        out[9] = planWords[0];
        out[10] = planWords[1];
    }
    if (plan && sah && planWords[1]) rc = 1;
    return rc;
}

extern "C" int ark_ddgi_debug_lbvh_check(const float* triangles, uint64_t n, uint64_t* out)
{
    return ark_ddgi_debug_lbvh_check_opts(triangles, n, ark::lbvh::kDefaultCriterion, out);
}

// ark_ddgi_debug.h: the device build of the sun's light-space BVH8 (ddgi_bvh_build.hip:
// k_lbvh_prims_light, k_lbvh_keys_light, the collapse under lbvh::kSlotsAscendingW) restated
// serially on the host with the same lbvh_build.h functions, over sun_frame's frame and
// sunAddRecords' light triangles; then ark_ddgi_debug_sun_bvh_check's ray comparison.
namespace {
int sunLbvhCheck(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax, int w_bits, bool sahPass, uint64_t* out,
                 uint64_t* treelets, bool plan = false, uint64_t* planOut = nullptr)
{
    using namespace ark;
    if (out) std::fill(out, out + 16, uint64_t(0));
    if (w_bits < 0) w_bits = lbvh::kSunKeyBitsW;
    if (n == 0 || w_bits > lbvh::kMortonBits || (w_bits & 1)) return 1;
    SunBvhInput in;
    sun_frame(sun_dir, in.frame);
    sun_add_triangles(in, soupTriangles(triangles, n));
    const std::vector<GpuTriangle> world = in.world;
    double frame[3][3];
    std::memcpy(frame, in.frame, sizeof(frame));
    // the host's tree of the same triangles: its inflation and its cost
    BvhBuildOptions opt;
    opt.threads = kDebugThreads;
    Bvh8CollapseOptions copt;
    Bvh8BuildResult sah;
    if (!build_sun_bvh(in, opt, copt, sah)) return 1;
    LbvhSunOptions so;
    std::memcpy(so.frame, frame, sizeof(so.frame));
    so.wBits = w_bits;
    const std::vector<int> classOf(1, 0);
    const LbvhHostResult r = build_lbvh_host(world, classOf, lbvh::kDefaultCriterion, &so, nullptr, sahPass, plan);
    if (treelets) *treelets = r.treelets.size();
    if (planOut) {
        planOut[0] = r.planRootCost;
        planOut[1] = r.smallInternal + (r.planStalled ? 1u : 0u);
    }
    if (r.nodes.empty() || r.roots[0] != 0) return 1;
    // structure: one tree from node 0, each depth one range behind the depth above's, every
    // record the input's bit for bit (the light-space boxes are covered by the ray comparison:
    // check_bvh8_full's containment is of world coordinates)
    uint64_t violations = r.slotOrderViolations;
    std::string why;
    const int32_t root = 0;
    if (!checkBvh8Structure(r.nodes, r.tris, &root, 1, why)) violations++;
    std::vector<uint32_t> order, offsets;
    if (!bvhLevelOrder(r.nodes.data(), r.nodes.size(), &root, 1, order, offsets) || order != r.order || offsets != r.levelOffsets) violations++;
    if (offsets.size() != static_cast<size_t>(r.depth) + 1u) violations++;
    {
        // bvhLevelOrder's levels, deepest first, must be consecutive ranges ending at the node count
        uint32_t end = static_cast<uint32_t>(r.nodes.size());
        for (size_t l = 0; l + 1 < offsets.size(); ++l) {
            const uint32_t cnt = offsets[l + 1] - offsets[l];
            for (uint32_t k = 0; k < cnt; ++k)
                if (order[offsets[l] + k] != end - cnt + k) {
                    violations++;
                    break;
                }
            end -= cnt;
        }
        if (end != 0) violations++;
    }
    uint64_t leafChildren = 0;
    for (const GpuBvh8Node& nd : r.nodes) {
        if (nd.leaf_mask & nd.imask) violations++;
        leafChildren += static_cast<uint64_t>(__builtin_popcount(nd.leaf_mask));
    }
    violations += recordViolations(r.tris, r.perm, world);
    uint32_t ia, ib;
    std::memcpy(&ia, &r.inflateAbs, 4);
    std::memcpy(&ib, &in.inflateAbs, 4);
    const uint64_t mism = sunRayCompare(r.nodes, r.tris, world, frame, sun_dir, origins, n_rays, tmax, out);
    float L[3];
    sun_ray_dir(sun_dir, L);
    const std::vector<float> o(origins, origins + 3 * n_rays);
    if (out) {
        out[6] = r.nodes.size();
        out[8] = violations;
        out[9] = ia != ib ? 1 : 0;
        out[10] = static_cast<uint64_t>(sun_shadow_cost(r.nodes, r.tris, &root, 1, frame, L, o) * 1e6);
        out[11] = static_cast<uint64_t>(sun_shadow_cost(sah.nodes, sah.tris, &root, 1, frame, L, o) * 1e6);
        // the tree's shape (_opts only)
        out[12] = leafChildren;
        out[13] = r.depth;
        out[14] = r.tris.size();
        out[15] = static_cast<uint64_t>(w_bits);
    }
    if (violations || ia != ib) return 1;
    return mism == 0 ? 0 : 2;
}
} // namespace

extern "C" int ark_ddgi_debug_sun_lbvh_check_opts(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                                   int w_bits, uint64_t* out)
{
    return sunLbvhCheck(triangles, n, sun_dir, origins, n_rays, tmax, w_bits, false, out, nullptr);
}

extern "C" int ark_ddgi_debug_sun_lbvh_check_sah(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                                  int w_bits, int sah, uint64_t* out)
{
    uint64_t treelets = 0;
    if (out) out[16] = 0;
    const int rc = sunLbvhCheck(triangles, n, sun_dir, origins, n_rays, tmax, w_bits, sah != 0, out, &treelets);
    if (out) out[16] = treelets;
    return rc;
}

extern "C" int ark_ddgi_debug_sun_lbvh_check_plan(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                                   int w_bits, int sah, int plan, uint64_t* out)
{
    uint64_t treelets = 0, planWords[2] = { 0, 0 };
    if (out) out[16] = out[17] = out[18] = 0;
    int rc = sunLbvhCheck(triangles, n, sun_dir, origins, n_rays, tmax, w_bits, sah != 0, out, &treelets, plan != 0, planWords);
    if (out) {
        out[16] = treelets;
        out[17] = planWords[0];
        out[18] = planWords[1];
    }
    if (plan && sah && planWords[1] && rc == 0) rc = 1;
    return rc;
}

extern "C" int ark_ddgi_debug_sun_lbvh_check(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax, uint64_t* out)
{
    uint64_t all[16];
    const int rc = ark_ddgi_debug_sun_lbvh_check_opts(triangles, n, sun_dir, origins, n_rays, tmax, ark::lbvh::kSunKeyBitsW, all);
    if (out) std::copy(all, all + 12, out);
    return rc;
}
