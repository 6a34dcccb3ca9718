// sun_bvh.cpp — the sun's light-space BVH8 (host build) and the sampled shadow-ray cost.
#include "sun_bvh.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <utility>

#include "lbvh_build.h"

namespace ark {

void sun_ray_dir(const float sunDir[3], float L[3])
{
    const float dd = sunDir[0] * sunDir[0] + sunDir[1] * sunDir[1] + sunDir[2] * sunDir[2];
    const float sc = 1.0f / std::sqrt(dd);
    for (int k = 0; k < 3; ++k) L[k] = -(sunDir[k] * sc);
}

// The sun's shadow rays (opaque.rchit:35-54, the sun branch :56-73) all travel along
// L = -normalize(sun direction) - the fp32 value k_shadow_gen gives them. In the
// orthonormal frame (u, v, w = L / |L|) they are rays along +w: a child box is crossed
// iff the ray's (u, v) lies in the box's u-v rectangle and the box reaches above its
// origin, a containment test in the node's quantized grid with no division and no
// per-child multiply (k_trace_shadow<SUN>, visitNodeSun). The light-space BVH holds
// every triangle of every hit-mask class (shadow rays test all three with the Opaque
// flag, no alpha test) with the world-space triangle records, so the any-hit tests and
// their results are those of the world BVHs.
void sun_frame(const float sunDir[3], double frame[3][3])
{
    float L[3];
    sun_ray_dir(sunDir, L);
    double w[3] = { L[0], L[1], L[2] };
    const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (double& x : w) x /= wl;
    const double h[3] = { std::fabs(w[0]) < 0.9 ? 1.0 : 0.0, std::fabs(w[0]) < 0.9 ? 0.0 : 1.0, 0.0 };
    double u[3] = { h[1] * w[2] - h[2] * w[1], h[2] * w[0] - h[0] * w[2], h[0] * w[1] - h[1] * w[0] };
    const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (double& x : u) x /= ul;
    const double v[3] = { w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0] };
    for (int k = 0; k < 3; ++k) {
        frame[0][k] = u[k];
        frame[1][k] = v[k];
        frame[2][k] = w[k];
    }
}

// Light-space build triangles of world-space records: rec(i) gives triangle i's record.
template<class RecordOf>
static void sunAddRecords(SunBvhInput& in, size_t n, RecordOf rec, int threads)
{
    const size_t base = in.world.size();
    in.tris.resize(base + n);
    in.world.resize(base + n);
    // independent per triangle: in chunks on `threads` threads, the largest |coordinate|
    // reduced at the end (a max does not depend on the order)
    const int T = std::max(1, std::min<int>(threads > 0 ? threads : static_cast<int>(std::thread::hardware_concurrency()), static_cast<int>(n >> 16) + 1));
    std::vector<float> maxAbs(T, 0.0f);
    auto work = [&](int t) {
        const size_t b = n * t / T, e = n * (t + 1) / T;
        for (size_t i = b; i < e; ++i) {
            const GpuTriangle rc = rec(i);
            // the triangle Möller–Trumbore tests: v0, v0 + e1, v0 + e2 (exact, from the record)
            // (lbvh_build.h: the refit and the device build box the same light coordinates)
            const float e1[3] = { rc.t0[3], rc.t1[0], rc.t1[1] }, e2[3] = { rc.t1[2], rc.t1[3], rc.t2[0] };
            float Lv[3][3], m;
            lbvh::lightVertices(rc.t0, e1, e2, &in.frame[0][0], Lv, m);
            maxAbs[t] = std::max(maxAbs[t], m);
            BuildTriangle& l = in.tris[base + i];
            float* dst[3] = { l.v0, l.v1, l.v2 };
            for (int k = 0; k < 3; ++k)
                for (int r = 0; r < 3; ++r) dst[k][r] = Lv[k][r];
            l.instance = 0;
            l.primitive = static_cast<uint32_t>(base + i);
            l.flip_facing = 0;
            in.world[base + i] = rc;
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back(work, t);
    work(0);
    for (std::thread& th : pool) th.join();
    for (float m : maxAbs) in.maxAbs = std::max(in.maxAbs, m);
}

void sun_add_triangles(SunBvhInput& in, const std::vector<BuildTriangle>& tris, int threads)
{
    sunAddRecords(in, tris.size(), [&](size_t i) { return make_gpu_triangle(tris[i]); }, threads);
}

void sun_add_records(SunBvhInput& in, const std::vector<GpuTriangle>& records, int threads)
{
    std::vector<uint32_t> live;
    live.reserve(records.size());
    for (size_t i = 0; i < records.size(); ++i)
        if (!isHoleTriangle(records[i])) live.push_back(static_cast<uint32_t>(i));
    sunAddRecords(in, live.size(), [&](size_t i) { return records[live[i]]; }, threads);
}

bool build_sun_bvh(SunBvhInput& in, const BvhBuildOptions& opt, const Bvh8CollapseOptions& copt, Bvh8BuildResult& out)
{
    // light-space box inflation: the rounding of the light coordinates to fp32 here and
    // of the origin's (u, v, w) in the kernel (a 3-term fp32 dot product, about 3 ulp of
    // |P|), Möller–Trumbore's acceptance margin (as the world BVHs: bvh8_inflation_box,
    // 1e-6 of the diagonal) - each covered twice over
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (const BuildTriangle& t : in.tris)
        for (const float* v : { t.v0, t.v1, t.v2 })
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], v[a]);
                hi[a] = std::max(hi[a], v[a]);
            }
    BvhBuildOptions lopt = opt;
    lopt.max_leaf_size = kBvh8MaxLeafSize;
    lopt.inflate_abs = 2.0f * bvh8_inflation_box(lo, hi) + 2e-6f * in.maxAbs;
    in.inflateAbs = lopt.inflate_abs;
    BvhBuildResult r2 = build_bvh(in.tris, lopt, 0u, 0u);
    std::vector<BuildTriangle>().swap(in.tris);
    if (r2.max_leaf > static_cast<uint32_t>(kBvh8MaxLeafSize)) return false;
    Bvh8CollapseOptions lc = copt;
    lc.slot_sort_axis = 2; // every ray goes along +w
    out = collapse_bvh8(r2, 0u, 0u, lc);
    // the leaves' records become the world-space ones (primitive = world index)
    for (GpuTriangle& g : out.tris) {
        if (isHoleTriangle(g)) continue;
        uint32_t idx;
        std::memcpy(&idx, &g.t2[2], 4);
        g = in.world[idx];
    }
    std::vector<GpuTriangle>().swap(in.world);
    return true;
}

void sun_sample_origins(const std::vector<GpuTriangle>& tris, const float L[3], uint32_t n, std::vector<float>& out)
{
    out.clear();
    if (tris.empty() || n == 0) return;
    uint64_t x = 0x9E3779B97F4A7C15ull; // xorshift64: the same samples every build
    auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    for (uint64_t tries = 0; out.size() < 3ull * n && tries < 32ull * n; ++tries) {
        const GpuTriangle& g = tris[next() % tris.size()];
        if (isHoleTriangle(g)) continue;
        const double e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
        const double nrm[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
        uint32_t flip;
        std::memcpy(&flip, &g.t2[3], 4);
        const double dn = (nrm[0] * L[0] + nrm[1] * L[1] + nrm[2] * L[2]) * (flip ? -1.0 : 1.0);
        if (!(dn > 0.0)) continue; // the front face (CCW, mirrored instances flipped) must face the sun
        const double r1 = static_cast<double>(next() >> 11) * 0x1p-53, r2 = static_cast<double>(next() >> 11) * 0x1p-53;
        const double sq = std::sqrt(r1), b1 = sq * (1.0 - r2), b2 = sq * r2;
        for (int a = 0; a < 3; ++a) out.push_back(static_cast<float>(g.t0[a] + b1 * e1[a] + b2 * e2[a]));
    }
}

double sun_shadow_cost(const std::vector<GpuBvh8Node>& nodes, const std::vector<GpuTriangle>& tris, const int32_t* roots, int nRoots,
                       const double (*frame)[3], const float L[3], const std::vector<float>& origins)
{
    const size_t n = origins.size() / 3;
    if (n == 0) return 0.0;
    const float tmin = 0.025f, tmax = 1e30f;
    uint64_t steps = 0;
    std::vector<uint32_t> stack;
    for (size_t r = 0; r < n; ++r) {
        const float* P = &origins[3 * r];
        float ob[3], db[3];
        for (int a = 0; a < 3; ++a) {
            ob[a] = frame ? static_cast<float>(frame[a][0] * P[0] + frame[a][1] * P[1] + frame[a][2] * P[2]) : P[a];
            db[a] = frame ? (a == 2 ? 1.0f : 0.0f) : L[a];
        }
        float idir[3];
        for (int a = 0; a < 3; ++a) idir[a] = 1.0f / (std::fabs(db[a]) < 1e-20f ? std::copysign(1e-20f, db[a]) : db[a]);
        bool hit = false;
        for (int k = 0; k < nRoots && !hit; ++k) {
            if (roots[k] < 0) continue;
            stack.assign(1, static_cast<uint32_t>(roots[k]));
            while (!stack.empty() && !hit) {
                const GpuBvh8Node& nd = nodes[stack.back()];
                stack.pop_back();
                steps++;
                struct Cand { float tn; int s; } hc[8];
                int nh = 0;
                uint32_t before[8], cnt = 0;
                for (int s = 0; s < 8; ++s) {
                    before[s] = cnt;
                    if ((nd.imask >> s) & 1u) cnt++;
                    if (!((nd.imask >> s) & 1u) && !((nd.leaf_mask >> s) & 1u)) continue;
                    float tn = tmin, tf = tmax, lo[3], hi[3];
                    decodeSlotBox(nd, s, lo, hi);
                    for (int a = 0; a < 3; ++a) {
                        float t0 = (lo[a] - ob[a]) * idir[a];
                        float t1 = (hi[a] - ob[a]) * idir[a];
                        if (t0 > t1) std::swap(t0, t1);
                        tn = std::max(tn, t0);
                        tf = std::min(tf, t1);
                    }
                    if (tn <= tf * 1.00001f + 1e-7f) hc[nh++] = { tn, s };
                }
                std::sort(hc, hc + nh, [](const Cand& p, const Cand& q) { return p.tn < q.tn; });
                // the node's leaf triangles first (the dual step), nearest leaf first
                for (int i = 0; i < nh && !hit; ++i) {
                    if ((nd.imask >> hc[i].s) & 1u) continue;
                    uint32_t t[kBvh8MaxLeafSize];
                    const int c = bvh8SlotTriangles(nd, hc[i].s, t);
                    for (int j = 0; j < c && !hit; ++j) {
                        steps++;
                        const GpuTriangle& g = tris[t[j]];
                        const float v0[3] = { g.t0[0], g.t0[1], g.t0[2] }, e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
                        const float pv[3] = { L[1] * e2[2] - L[2] * e2[1], L[2] * e2[0] - L[0] * e2[2], L[0] * e2[1] - L[1] * e2[0] };
                        const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
                        if (det == 0.0f) continue;
                        const float inv = 1.0f / det;
                        const float sv[3] = { P[0] - v0[0], P[1] - v0[1], P[2] - v0[2] };
                        const float u = (sv[0] * pv[0] + sv[1] * pv[1] + sv[2] * pv[2]) * inv;
                        if (!(u >= 0.0f && u <= 1.0f)) continue;
                        const float q[3] = { sv[1] * e1[2] - sv[2] * e1[1], sv[2] * e1[0] - sv[0] * e1[2], sv[0] * e1[1] - sv[1] * e1[0] };
                        const float v = (L[0] * q[0] + L[1] * q[1] + L[2] * q[2]) * inv;
                        if (!(v >= 0.0f && u + v <= 1.0f)) continue;
                        const float tt = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv;
                        hit = tt >= tmin && tt <= tmax;
                    }
                }
                for (int i = nh - 1; i >= 0 && !hit; --i)
                    if ((nd.imask >> hc[i].s) & 1u) stack.push_back(nd.child_base + before[hc[i].s]);
            }
        }
    }
    return static_cast<double>(steps) / static_cast<double>(n);
}

} // namespace ark
