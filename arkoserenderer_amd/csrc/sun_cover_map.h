// sun_cover_map.h — the sun's cover map: a conservative light-space depth map that
// resolves most sun shadow rays in k_shadow_gen, before they are listed.
// What the device build (ddgi_cover_map.hip) and its host restatement (sun_cover_map.cpp)
// share, in the manner of lbvh_build.h: every value of the map is computed by the functions
// below, in double, and combined by maxima of ordered words, so both give the same bits.
//
// The map is a 2-D grid over the scene's extent in the sun frame's (u, v) (sunCoords). A
// cell holds
//   wCover  the largest, over the triangles that cover the cell, of the lowest w of the
//           triangle's plane over the cell, less the triangle's w margin (-inf: none)
//   wTop    the largest, over the triangles whose (u, v) box touches the cell, of the highest
//           w at which a ray of the cell can meet the triangle - its plane's highest w
//           over the cell, no higher than its highest vertex - plus its w margin (-inf: none)
// and a sun ray from light-space point pl in that cell is
//   occluded  when pl.w + tmin + M0 < wCover  (the covering triangle is hit)
//   lit       when pl.w + tmin - M0 > wTop    (nothing reaches up to where hits are accepted:
//             the triangle the ray starts on stays below tmin across a cell unless it is steep)
// Which triangles count: the sun's any-hit traversal (k_trace_shadow) tests the three
// hit-mask classes in turn with the Opaque flag - no alpha test, cull mask 0xff - so every
// record of the world BVHs that is not a hole is accepted unconditionally, for both values.
//
// Margins. M0 = kMarginScale x (light-space diagonal + largest |world coordinate|), the
// builder's rule (bvh8_inflation_box: 1e-6 of the diagonal = 2 ulp x 4; build_sun_bvh adds
// 2e-6 max |coordinate| for the light coordinates) with one scale for both terms. It bounds,
// with a factor of about 4: the rounding of sunCoords for the origin (a 3-term fp32 dot,
// 3 ulp of |P| sqrt 3), of the frame's rows to fp32 and of the vertices' light coordinates
// (1 ulp each), the ray direction's fp32 length and angle to the frame's w (1e-7 t), and
// the fp32 adds of the consumer's two comparisons - about 7e-7 max |coordinate| together.
// The band along an edge in which the fp32 Möller–Trumbore (intersectTri: no determinant
// epsilon, both faces) can disagree with exact arithmetic is not uniform: the sign of
// u = (s . p) / det with p = d x e2 is that of s . p, whose error is 3 ulp |s| |p| from the
// dot and |s| times p's own rounding, 2 ulp |d| |e2| - as a distance from the projected
// edge, divided by |p| = |e2 projected|: 3 ulp |s| + 2 ulp |s| |e2| / |e2 projected|. With
// |s| at most the diagonal that is below 1e-6 diagonal x A for the triangle's slant
// A = max(|e1| / |e1'|, |e2| / |e2'|, (|e1| + |e2|) / |e3'|) >= 1 (' = projected along the
// sun; the third edge tests u + v, the sum of both errors). Likewise t = (e2 . q) / det
// carries about 12 ulp diagonal x Aw, Aw = |e1| |e2| / |det| (a sliver or a triangle near
// edge-on has a large one). So a triangle's (u, v) margin is M0 x A and its w margin
// M0 x Aw: a triangle near edge-on covers no grown cell and drops out by itself, a
// triangle whose Aw exceeds kMaxSlantW never covers and tops its cells with +inf, and one
// whose A exceeds kMaxSlant poisons the map (no map is installed: rare, an edge within
// 2.4e-4 rad of the sun's direction). A triangle whose fp32 determinant is exactly 0 is
// never hit (intersectTri) and is skipped. The consumer's cell index (an fp32 subtract and
// multiply, at most kMaxDim cells) is off by less than kCellSlack cells, which every cell
// is grown by as well.
#pragma once

#include <stdint.h>

#include "ddgi_types.h"
#include "lbvh_build.h"

namespace ark {
namespace cover {

constexpr double kMarginScale = 4e-6;
constexpr double kMaxSlant = 4096.0;
constexpr double kMaxSlantW = 1024.0;
constexpr double kCellSlack = 4e-3;  // cells: 2 x 2^-23 x kMaxDim, doubled
constexpr uint32_t kMaxDim = 8192;   // cells per side at most
constexpr float kTmin = 0.025f;      // the shadow rays' tmin (k_trace_shadow)
constexpr uint32_t kExtentBins = 1024; // histogram of projected extents: fp32 bits >> 21
constexpr uint32_t kBigCells = 256;  // a triangle over more cells is rastered by a workgroup
// Cells per median projected triangle extent. A cell resolves rays only where a triangle
// covers all of it: on the 20 k-triangle soup at the flagship's density, 6 cells per extent
// resolve 50 % of surface origins, 10 cells 69 %, 16 cells 79 % (EXPERIMENTS.md).
constexpr double kCellsPerExtent = 12.0;
#ifndef ARK_COVER_BUDGET_MB
#define ARK_COVER_BUDGET_MB 64 // the map's byte budget (EXPERIMENTS.md: 16 and 256 measured)
#endif
constexpr uint64_t kDefaultBudget = static_cast<uint64_t>(ARK_COVER_BUDGET_MB) << 20;

// what the first pass reduces over the records (ordered words: lbvh::ordered)
struct Header {
    uint32_t prims;
    uint32_t lo[3], hi[3]; // light-space box
    uint32_t maxAbs;       // largest |world coordinate|, fp32 bits
    uint32_t poison;       // a triangle's slant exceeded kMaxSlant
    uint32_t big;          // triangles handed to the workgroup raster
    uint32_t hist[kExtentBins];
};

// the grid, chosen on the host from the header (chooseGrid) - what the consumer reads
struct Grid {
    float u0, v0;    // the lower corner
    float invCell;   // cells per unit length
    uint32_t nx, ny;
    float margin;    // M0
    float wExtent;   // the scene's w extent plus the largest w margin: the map is valid for tmax above it
};

ARK_LBVH_FN void initHeader(Header& h)
{
    h.prims = h.maxAbs = h.poison = h.big = 0u;
    for (int a = 0; a < 3; ++a) {
        h.lo[a] = 0xffffffffu;
        h.hi[a] = 0u;
    }
    for (uint32_t i = 0; i < kExtentBins; ++i) h.hist[i] = 0u;
}

ARK_LBVH_FN uint32_t floatBits(float f)
{
    union {
        float f;
        uint32_t u;
    } s;
    s.f = f;
    return s.u;
}

// a record's light coordinates; false: a hole
ARK_LBVH_FN bool recordLight(const GpuTriangle& g, const double* F, float L[3][3], float& maxAbs)
{
    if (floatBits(g.t2[1]) == kHoleInstance) return false;
    const float e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
    lbvh::lightVertices(g.t0, e1, e2, F, L, maxAbs);
    return true;
}

ARK_LBVH_FN uint32_t extentBin(const float L[3][3])
{
    float lo[2], hi[2];
    for (int a = 0; a < 2; ++a) {
        lo[a] = L[0][a] < L[1][a] ? (L[0][a] < L[2][a] ? L[0][a] : L[2][a]) : (L[1][a] < L[2][a] ? L[1][a] : L[2][a]);
        hi[a] = L[0][a] > L[1][a] ? (L[0][a] > L[2][a] ? L[0][a] : L[2][a]) : (L[1][a] > L[2][a] ? L[1][a] : L[2][a]);
    }
    const float eu = hi[0] - lo[0], ev = hi[1] - lo[1];
    const float e = eu > ev ? eu : ev;
    return (floatBits(e) >> 21) & (kExtentBins - 1u); // e >= 0: sign bit clear
}

// The grid for a reduced header: kCellsPerExtent cells per median projected extent, no
// smaller than the byte budget (8 B per cell) and kMaxDim allow. False: no map (no
// triangles, a poisoned header, a degenerate extent).
inline bool chooseGrid(const Header& h, uint64_t budgetBytes, Grid& g)
{
    if (h.prims == 0u || h.poison != 0u) return false;
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = lbvh::orderedFloat(h.lo[a]);
        hi[a] = lbvh::orderedFloat(h.hi[a]);
    }
    union {
        uint32_t u;
        float f;
    } s;
    s.u = h.maxAbs;
    const double maxAbs = s.f;
    const double diag = __builtin_sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    const double M0 = kMarginScale * (diag + maxAbs);
    if (!(M0 > 0.0) || !(diag < 1e30)) return false;
    // the median extent: the lower end of the bin that holds the middle triangle
    uint64_t run = 0;
    uint32_t bin = 0;
    for (; bin < kExtentBins; ++bin) {
        run += h.hist[bin];
        if (2 * run >= h.prims) break;
    }
    s.u = bin << 21;
    const double median = s.f;
    // the map's extent: the scene's (u, v) box and a border of two margins
    const double eu = (hi[0] - lo[0]) + 4.0 * M0, ev = (hi[1] - lo[1]) + 4.0 * M0;
    double cell = median / kCellsPerExtent;
    const double cells = static_cast<double>(budgetBytes / 8u);
    const double byBudget = __builtin_sqrt(eu * ev / cells) * 1.001;
    const double byDim = (eu > ev ? eu : ev) / (kMaxDim - 2.0);
    if (!(cell > byBudget)) cell = byBudget;
    if (cell < byDim) cell = byDim;
    if (!(cell > 0.0)) return false;
    g.invCell = static_cast<float>(1.0 / cell);
    const double c = 1.0 / static_cast<double>(g.invCell); // the cell every side computes with
    g.u0 = static_cast<float>(lo[0] - 2.0 * M0);
    g.v0 = static_cast<float>(lo[1] - 2.0 * M0);
    g.nx = static_cast<uint32_t>((hi[0] + 2.0 * M0 - g.u0) / c) + 2u;
    g.ny = static_cast<uint32_t>((hi[1] + 2.0 * M0 - g.v0) / c) + 2u;
    if (g.nx > kMaxDim || g.ny > kMaxDim || static_cast<uint64_t>(g.nx) * g.ny * 8u > budgetBytes + (budgetBytes >> 4)) return false;
    g.margin = static_cast<float>(M0);
    g.wExtent = static_cast<float>((hi[2] - lo[2]) + M0 * (kMaxSlantW + 4.0) + kTmin);
    return true;
}

// One triangle set up for the raster: its light coordinates, margins and cell range.
struct TriSetup {
    double U[3], V[3], W[3];
    double grow;     // its (u, v) margin M0 x A
    double padW;     // its w margin M0 x Aw (covering only)
    float top;       // what it tops its cells with
    int32_t x0, x1, y0, y1; // inclusive cell range of its grown box
    bool covers;     // may cover cells (Aw within kMaxSlantW)
    double gu, gv;   // the plane's w gradient
};

enum : int { kTriSkip = 0, kTriOk = 1, kTriPoison = 2 };

// The fp32 determinant of intersectTri for direction d (crossFma / dotFma3's order)
ARK_LBVH_FN float mtDet(const float d[3], const float e1[3], const float e2[3])
{
    const float p[3] = { __builtin_fmaf(d[1], e2[2], -(d[2] * e2[1])), __builtin_fmaf(d[2], e2[0], -(d[0] * e2[2])),
                         __builtin_fmaf(d[0], e2[1], -(d[1] * e2[0])) };
    return __builtin_fmaf(e1[0], p[0], __builtin_fmaf(e1[1], p[1], e1[2] * p[2]));
}

ARK_LBVH_FN double len3(double x, double y, double z) { return __builtin_sqrt(x * x + y * y + z * z); }

// L: the record's light coordinates (recordLight); d: the rays' fp32 direction
ARK_LBVH_FN int setupTriangle(const GpuTriangle& g, const float L[3][3], const float d[3], const Grid& grid, TriSetup& t)
{
    const float e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
    const float det = mtDet(d, e1, e2);
    if (!(det != 0.0f)) return kTriSkip; // 0 or NaN: intersectTri never accepts it
    for (int k = 0; k < 3; ++k) {
        t.U[k] = L[k][0];
        t.V[k] = L[k][1];
        t.W[k] = L[k][2];
    }
    const double M0 = grid.margin;
    const double l1 = len3(e1[0], e1[1], e1[2]), l2 = len3(e2[0], e2[1], e2[2]);
    const double p1 = len3(t.U[1] - t.U[0], t.V[1] - t.V[0], 0.0), p2 = len3(t.U[2] - t.U[0], t.V[2] - t.V[0], 0.0),
                 p3 = len3(t.U[2] - t.U[1], t.V[2] - t.V[1], 0.0);
    double A = 1.0;
    const double a1 = l1 / p1, a2 = l2 / p2, a3 = (l1 + l2) / p3;
    // (a NaN or infinite ratio - a projected edge of length 0 - fails the comparison below)
    A = a1 > A ? a1 : A;
    A = a2 > A ? a2 : A;
    A = a3 > A ? a3 : A;
    if (!(a1 <= kMaxSlant) || !(a2 <= kMaxSlant) || !(a3 <= kMaxSlant)) return kTriPoison;
    const double adet = det < 0.0f ? -static_cast<double>(det) : static_cast<double>(det);
    double Aw = l1 * l2 / adet;
    Aw = Aw > 1.0 ? Aw : 1.0;
    t.covers = Aw <= kMaxSlantW;
    t.grow = M0 * A;
    t.padW = M0 * Aw;
    double wmax = t.W[0] > t.W[1] ? t.W[0] : t.W[1];
    wmax = wmax > t.W[2] ? wmax : t.W[2];
    t.top = t.covers ? static_cast<float>(wmax + t.padW + M0) : __builtin_inff();
    // the plane w(u, v) = W0 + gu (u - U0) + gv (v - V0) through the light vertices
    const double au = t.U[1] - t.U[0], av = t.V[1] - t.V[0], aw = t.W[1] - t.W[0];
    const double bu = t.U[2] - t.U[0], bv = t.V[2] - t.V[0], bw = t.W[2] - t.W[0];
    const double area2 = au * bv - av * bu;
    t.gu = (aw * bv - av * bw) / area2;
    t.gv = (au * bw - aw * bu) / area2;
    if (!(area2 != 0.0)) t.covers = false;
    // cells its box, grown by its margin and the index slack, touches
    double ulo = t.U[0] < t.U[1] ? t.U[0] : t.U[1], uhi = t.U[0] > t.U[1] ? t.U[0] : t.U[1];
    double vlo = t.V[0] < t.V[1] ? t.V[0] : t.V[1], vhi = t.V[0] > t.V[1] ? t.V[0] : t.V[1];
    ulo = ulo < t.U[2] ? ulo : t.U[2];
    uhi = uhi > t.U[2] ? uhi : t.U[2];
    vlo = vlo < t.V[2] ? vlo : t.V[2];
    vhi = vhi > t.V[2] ? vhi : t.V[2];
    const double inv = grid.invCell;
    auto cellOf = [&](double c, double org, double n) {
        double q = __builtin_floor((c - org) * inv);
        q = q < 0.0 ? 0.0 : q;
        q = q > n - 1.0 ? n - 1.0 : q;
        return static_cast<int32_t>(q);
    };
    t.x0 = cellOf(ulo - t.grow - kCellSlack / inv, grid.u0, grid.nx);
    t.x1 = cellOf(uhi + t.grow + kCellSlack / inv, grid.u0, grid.nx);
    t.y0 = cellOf(vlo - t.grow - kCellSlack / inv, grid.v0, grid.ny);
    t.y1 = cellOf(vhi + t.grow + kCellSlack / inv, grid.v0, grid.ny);
    return kTriOk;
}

ARK_LBVH_FN uint64_t cellCount(const TriSetup& t) { return static_cast<uint64_t>(t.x1 - t.x0 + 1) * static_cast<uint64_t>(t.y1 - t.y0 + 1); }

// What the triangle gives cell (cx, cy), grown by its margin and the index slack. top: the
// highest w at which a ray of the cell can hit it, plus its w margin - its plane's highest w
// over the grown cell, no higher than its highest vertex (+inf when its w margin is beyond
// kMaxSlantW). Returns whether it covers the grown cell; then wCover is the plane's lowest w
// over it, less the w margin.
ARK_LBVH_FN bool cellValues(const TriSetup& t, const Grid& grid, int32_t cx, int32_t cy, float& top, float& wCover)
{
    top = t.top;
    if (!t.covers) return false;
    const double c = 1.0 / static_cast<double>(grid.invCell);
    const double xa = static_cast<double>(grid.u0) + (cx - kCellSlack) * c - t.grow, xb = static_cast<double>(grid.u0) + (cx + 1.0 + kCellSlack) * c + t.grow;
    const double ya = static_cast<double>(grid.v0) + (cy - kCellSlack) * c - t.grow, yb = static_cast<double>(grid.v0) + (cy + 1.0 + kCellSlack) * c + t.grow;
    const double X[4] = { xa, xb, xa, xb }, Y[4] = { ya, ya, yb, yb };
    const double au = t.U[1] - t.U[0], av = t.V[1] - t.V[0], bu = t.U[2] - t.U[0], bv = t.V[2] - t.V[0];
    const double sgn = au * bv - av * bu > 0.0 ? 1.0 : -1.0;
    double wlow = __builtin_inf(), whigh = -__builtin_inf();
    bool inside = true;
    for (int k = 0; k < 4; ++k) {
        // the three edge functions, positive inside
        for (int e = 0; e < 3; ++e) {
            const int i = e, j = (e + 1) % 3;
            const double f = ((t.U[j] - t.U[i]) * (Y[k] - t.V[i]) - (t.V[j] - t.V[i]) * (X[k] - t.U[i])) * sgn;
            inside = inside && f > 0.0;
        }
        const double w = t.W[0] + t.gu * (X[k] - t.U[0]) + t.gv * (Y[k] - t.V[0]);
        wlow = w < wlow ? w : wlow;
        whigh = w > whigh ? w : whigh;
    }
    const float planeTop = static_cast<float>(whigh + t.padW + static_cast<double>(grid.margin));
    if (planeTop < top) top = planeTop; // (false for a NaN: the vertex bound stays)
    wCover = static_cast<float>(wlow - t.padW - static_cast<double>(grid.margin));
    return inside;
}

// The consumer's side (k_shadow_gen, the host's verdicts): the cell of light-space (u, v)
// in fp32, -1 outside the map
ARK_LBVH_FN int64_t cellIndex(const Grid& g, float u, float v)
{
    const float fx = (u - g.u0) * g.invCell, fy = (v - g.v0) * g.invCell;
    if (!(fx >= 0.0f) || !(fy >= 0.0f) || !(fx < static_cast<float>(g.nx)) || !(fy < static_cast<float>(g.ny))) return -1;
    return static_cast<int64_t>(static_cast<uint32_t>(fy)) * g.nx + static_cast<uint32_t>(fx);
}
enum : int { kUndecided = 0, kOccluded = 1, kLit = 2 };
// lift = tmin + M0, reach = tmin - M0: a hit is accepted only from tmin on
ARK_LBVH_FN int verdict(float w, float lift, float reach, float wCover, float wTop)
{
    if (w + lift < wCover) return kOccluded;
    if (w + reach > wTop) return kLit;
    return kUndecided;
}

} // namespace cover
} // namespace ark
