// sun_cover_map.cpp — the sun's cover map (sun_cover_map.h): the host restatement of its
// build, the device build's sequence, and the checks of ark_ddgi_debug.h.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <thread>

#include "../../include/ark_ddgi.h"
#include "../../include/ark_ddgi_debug.h"
#include "sun_bvh.h"
#include "sun_cover_build.h"

namespace ark {

void sunRayDirection(const float sunDir[3], float L[3])
{
    sun_ray_dir(sunDir, L); // normalize() of the kernels, as sun_frame's w
}

bool hostBuildCoverMap(const GpuTriangle* rec, uint64_t records, const double* frame, const float* dir, uint64_t budgetBytes, cover::Grid& grid,
                       std::vector<float>& map)
{
    auto hdr = std::make_unique<cover::Header>();
    cover::initHeader(*hdr);
    for (uint64_t i = 0; i < records; ++i) {
        float L[3][3], maxAbs;
        if (!cover::recordLight(rec[i], frame, L, maxAbs)) continue;
        hdr->prims++;
        for (int a = 0; a < 3; ++a) {
            hdr->lo[a] = std::min(hdr->lo[a], lbvh::ordered(std::min(L[0][a], std::min(L[1][a], L[2][a]))));
            hdr->hi[a] = std::max(hdr->hi[a], lbvh::ordered(std::max(L[0][a], std::max(L[1][a], L[2][a]))));
        }
        hdr->maxAbs = std::max(hdr->maxAbs, cover::floatBits(maxAbs));
        hdr->hist[cover::extentBin(L)]++;
    }
    if (!cover::chooseGrid(*hdr, budgetBytes, grid)) return false;
    std::vector<uint32_t> words(static_cast<size_t>(grid.nx) * grid.ny * 2u, lbvh::ordered(-INFINITY));
    for (uint64_t i = 0; i < records; ++i) {
        float L[3][3], maxAbs;
        if (!cover::recordLight(rec[i], frame, L, maxAbs)) continue;
        cover::TriSetup t;
        const int kind = cover::setupTriangle(rec[i], L, dir, grid, t);
        if (kind == cover::kTriSkip) continue;
        if (kind == cover::kTriPoison) return false;
        for (int32_t cy = t.y0; cy <= t.y1; ++cy)
            for (int32_t cx = t.x0; cx <= t.x1; ++cx) {
                uint32_t* texel = words.data() + 2u * (static_cast<size_t>(cy) * grid.nx + static_cast<uint32_t>(cx));
                float top, wc;
                const bool covers = cover::cellValues(t, grid, cx, cy, top, wc);
                texel[1] = std::max(texel[1], lbvh::ordered(top));
                if (covers) texel[0] = std::max(texel[0], lbvh::ordered(wc));
            }
    }
    map.resize(words.size());
    for (size_t i = 0; i < words.size(); ++i) map[i] = lbvh::orderedFloat(words[i]);
    return true;
}

hipError_t deviceBuildCoverMap(const GpuTriangle* devRec, uint64_t records, const double* frame, const float* dir, uint64_t budgetBytes, hipStream_t s,
                               cover::Grid& grid, DeviceBuffer& map, bool& ok)
{
    ok = false;
    if (records == 0 || records > 0xffffffffull) return hipSuccess;
    const uint32_t n = static_cast<uint32_t>(records);
    auto hdr = std::make_unique<cover::Header>();
    cover::initHeader(*hdr);
    DeviceBuffer dHdr, big;
    hipError_t e = dHdr.alloc(sizeof(cover::Header));
    auto done = [&](hipError_t r) {
        dHdr.release();
        big.release();
        if (r != hipSuccess || !ok) map.release();
        return r;
    };
    if (e != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(dHdr.ptr, hdr.get(), sizeof(cover::Header), hipMemcpyHostToDevice, s)) != hipSuccess) return done(e);
    if ((e = launch_cover_prims(devRec, n, frame, dHdr.as<cover::Header>(), s)) != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(hdr.get(), dHdr.ptr, sizeof(cover::Header), hipMemcpyDeviceToHost, s)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return done(e);
    if (!cover::chooseGrid(*hdr, budgetBytes, grid)) return done(hipSuccess);
    const size_t words = static_cast<size_t>(grid.nx) * grid.ny * 2u;
    if ((e = map.alloc(words * 4u)) != hipSuccess) return done(e);
    if ((e = big.alloc(static_cast<size_t>(n) * 4u)) != hipSuccess) return done(e);
    if ((e = launch_cover_raster(devRec, n, frame, dir, grid, map.as<uint32_t>(), big.as<uint32_t>(), dHdr.as<cover::Header>(), s)) != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(hdr.get(), dHdr.ptr, sizeof(cover::Header), hipMemcpyDeviceToHost, s)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return done(e);
    if (hdr->poison != 0u) return done(hipSuccess);
    if ((e = launch_cover_big(devRec, frame, dir, grid, map.as<uint32_t>(), big.as<uint32_t>(), hdr->big, s)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return done(e);
    ok = true;
    return done(hipSuccess);
}

} // namespace ark

namespace {

void recordsOf(const float* triangles, uint64_t n, std::vector<ark::GpuTriangle>& rec)
{
    rec.clear();
    for (const ark::BuildTriangle& t : ark::soupTriangles(triangles, n)) rec.push_back(ark::make_gpu_triangle(t));
}

} // namespace

// ark_ddgi_debug.h: the host map's verdicts against a brute-force any-hit over every
// triangle with the kernels' fp32 Möller–Trumbore (intersectTri's operation order).
extern "C" int ark_ddgi_debug_cover_map_check(const float* triangles, uint64_t n, const float* sun_dir, const float* origins, uint64_t n_rays, float tmax,
                                              uint64_t budget_bytes, uint64_t* out)
{
    using namespace ark;
    if (!triangles || !sun_dir || !origins || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    std::vector<GpuTriangle> rec;
    recordsOf(triangles, n, rec);
    double frame[3][3];
    sun_frame(sun_dir, frame);
    float L[3];
    sunRayDirection(sun_dir, L);
    cover::Grid grid {};
    std::vector<float> map;
    const bool ok = hostBuildCoverMap(rec.data(), n, &frame[0][0], L, budget_bytes ? budget_bytes : cover::kDefaultBudget, grid, map) && tmax >= grid.wExtent;
    float F[9];
    for (int k = 0; k < 9; ++k) F[k] = static_cast<float>((&frame[0][0])[k]);
    const float tmin = cover::kTmin, lift = tmin + grid.margin, reach = tmin - grid.margin;
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
    std::atomic<uint64_t> occB { 0 }, occM { 0 }, litM { 0 }, wrong { 0 };
    auto worker = [&](uint64_t r0, uint64_t r1) {
        uint64_t b = 0, mo = 0, ml = 0, w = 0;
        for (uint64_t ri = r0; ri < r1; ++ri) {
            const float* o = origins + 3 * ri;
            bool brute = false;
            for (const GpuTriangle& g : rec)
                if (mt(o, g)) {
                    brute = true;
                    break;
                }
            int vd = cover::kUndecided;
            if (ok) {
                // sunCoords
                const float pl[3] = { std::fma(o[0], F[0], std::fma(o[1], F[1], o[2] * F[2])), std::fma(o[0], F[3], std::fma(o[1], F[4], o[2] * F[5])),
                                      std::fma(o[0], F[6], std::fma(o[1], F[7], o[2] * F[8])) };
                const int64_t c = cover::cellIndex(grid, pl[0], pl[1]);
                if (c >= 0) vd = cover::verdict(pl[2], lift, reach, map[2 * c], map[2 * c + 1]);
            }
            b += brute;
            mo += vd == cover::kOccluded;
            ml += vd == cover::kLit;
            w += (vd == cover::kOccluded && !brute) || (vd == cover::kLit && brute);
        }
        occB += b;
        occM += mo;
        litM += ml;
        wrong += w;
    };
    const int T = static_cast<int>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back(worker, n_rays * t / T, n_rays * (t + 1) / T);
    for (auto& th : pool) th.join();
    uint64_t covered = 0;
    for (size_t i = 0; i < map.size(); i += 2) covered += map[i] > -INFINITY;
    out[0] = n_rays;
    out[1] = occB.load();
    out[2] = occM.load();
    out[3] = litM.load();
    out[4] = wrong.load();
    out[5] = ok ? grid.nx : 0;
    out[6] = ok ? grid.ny : 0;
    out[7] = ok ? 1 : 0;
    out[8] = covered;
    out[9] = n_rays - occM.load() - litM.load();
    out[10] = cover::floatBits(grid.u0);
    out[11] = cover::floatBits(grid.v0);
    out[12] = cover::floatBits(grid.invCell);
    return ARK_DDGI_OK;
}

// ark_ddgi_debug.h: the device build against the host restatement, word for word
extern "C" int ark_ddgi_debug_cover_map_device(int device, const float* triangles, uint64_t n, const float* sun_dir, uint64_t budget_bytes, uint64_t* out)
{
    using namespace ark;
    if (!triangles || !sun_dir || !out) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (hipSetDevice(device) != hipSuccess) return ARK_DDGI_E_DEVICE;
    std::vector<GpuTriangle> rec;
    recordsOf(triangles, n, rec);
    double frame[3][3];
    sun_frame(sun_dir, frame);
    float L[3];
    sunRayDirection(sun_dir, L);
    const uint64_t budget = budget_bytes ? budget_bytes : cover::kDefaultBudget;
    cover::Grid hg {}, dg {};
    std::vector<float> hmap;
    const bool hok = hostBuildCoverMap(rec.data(), n, &frame[0][0], L, budget, hg, hmap);
    DeviceBuffer dRec, dMap;
    if (dRec.alloc((n + 1) * sizeof(GpuTriangle)) != hipSuccess) return ARK_DDGI_E_DEVICE;
    bool dok = false;
    hipError_t e = hipMemcpy(dRec.ptr, rec.data(), n * sizeof(GpuTriangle), hipMemcpyHostToDevice);
    const auto t0 = std::chrono::steady_clock::now();
    if (e == hipSuccess) e = deviceBuildCoverMap(dRec.as<GpuTriangle>(), n, &frame[0][0], L, budget, nullptr, dg, dMap, dok);
    const auto t1 = std::chrono::steady_clock::now();
    uint64_t diff = 0;
    if (e == hipSuccess && hok && dok) {
        if (std::memcmp(&hg, &dg, sizeof(hg)) != 0) {
            diff = ~0ull;
        } else {
            std::vector<float> dmap(hmap.size());
            e = hipMemcpy(dmap.data(), dMap.ptr, dmap.size() * 4u, hipMemcpyDeviceToHost);
            for (size_t i = 0; i < hmap.size(); ++i) diff += cover::floatBits(hmap[i]) != cover::floatBits(dmap[i]);
        }
    }
    dRec.release();
    dMap.release();
    if (e != hipSuccess) return ARK_DDGI_E_DEVICE;
    out[0] = diff;
    out[1] = hg.nx;
    out[2] = hg.ny;
    out[3] = hok ? 1 : 0;
    out[4] = dok ? 1 : 0;
    out[5] = static_cast<uint64_t>(std::chrono::duration<double, std::micro>(t1 - t0).count());
    return ARK_DDGI_OK;
}
