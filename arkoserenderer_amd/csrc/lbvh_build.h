// lbvh_build.h — the build logic of the device-side LBVH of the world BVH8s
// (ddgi_bvh_build.hip), shared with its serial host restatement
// (ark_ddgi_debug_lbvh_check, lbvh_host.cpp). Plain inline functions over plain
// arrays, no HIP types: the host check and the kernels run the same code.
//
//   mortonKey      class << 60 | 60-bit Morton code (20 bits per axis, x highest) of a
//                  record's centroid inside the all-class scene box
//   delta / nodeRange / findSplit   the radix tree of Karras 2012 ("Maximizing
//                  parallelism in the construction of BVHs, octrees, and k-d trees")
//                  over one class's range [lo, hi) of the sorted keys. Equal keys are
//                  told apart by their sorted index. Internal node i covers a contiguous
//                  range whose first or last primitive is i, so a child is known by its
//                  range alone: the left child [first, split] is internal node `split`,
//                  the right one [split + 1, last] internal node `split + 1`, a range of
//                  one primitive a leaf. Only split[] is stored.
//   selectCut      the members of one BVH8 node: the BVH2 node's two children, then one
//                  member of more than kBvh8MaxLeafSize triangles opened at a time until
//                  there are 8 or none can be opened
//   assignSlots    internal children into the octant slot of their Morton cell's centre
//                  relative to the node's cell, leaf members into the slots left over
//   placeRows      the leaf slots' triangle rows of one node (GpuBvh8Node)
//
// The sun's light-space BVH8 (ARK_DDGI_FLAG_GPU_REBUILD_SUN) is built by the same functions
// over one range [0, n): lightVertices (a record's vertices in the sun's frame, shared with
// build_sun_bvh and the refit), lightKey (a Morton code of the light-space box's centre,
// class bits 0, w given wBits of the 60 and u, v the rest: KeyLayout) and the slot rule
// kSlotsAscendingW (every ray goes along +w and visits a node's children in slot order).
//
// The SAH pass (ARK_DDGI_FLAG_GPU_REBUILD_SAH, k_lbvh_treelet_sah and its host restatement):
// every maximal range of the radix tree of at most kTreeletPrims primitives (a treelet) gets a
// binary tree of its own by a full three-axis sweep SAH, its primitives reordered inside the
// range. sorted[] is permuted inside a treelet; keys[] is NOT: it stays sorted and from then
// on only describes the Morton cells of ranges that are unions of whole treelets. Inside a
// treelet split[] keeps the numbering (left child [f, s]: node s, right child: node s + 1),
// which is collision-free for any tree over contiguous ranges, so selectCut reads it as it
// is. What the pass shares between the kernel and the host: ordered / orderedFloat (boxes are
// min / max unions of ordered words: the same bits in any order, -0 below +0), sweepKey,
// halfArea, splitKey; what the collapse reads of it: SahBoxes, kOpenLargestBox, rangeCentre,
// memberLowW.
//
// The collapse plan (ARK_DDGI_FLAG_GPU_REBUILD_PLAN, with the SAH pass): the treelets go down
// to single primitives (treeletsOf lists ranges of 2 and 3 too, so only single primitives lie
// outside a treelet), and every BVH2 node n gets cost[n][i], i = 1 .. 8 - the least SAH cost
// of the subtree below n held in at most i slots of a BVH8 node (Ylitie, Karras, Laine 2017,
// the host collapse's planNode) - and the picks that reach it (planCosts; one packed word per
// node, kPlanDone set once it is final). Bottom-up: inside a treelet by its workgroup, above
// the treelets by k_lbvh_upper_plan, which also boxes those nodes. The collapse then walks the
// picks (planCut) where it chose greedily (selectCut); a range of at most kBvh8MaxLeafSize
// primitives is never an internal member, so assignSlots, the rows and the scatter see what
// they saw before.
#pragma once

#include <stdint.h>

#include "ddgi_types.h"

#if defined(__HIPCC__)
#define ARK_LBVH_FN __host__ __device__ inline
#else
#define ARK_LBVH_FN inline
#endif

namespace ark {
namespace lbvh {

constexpr int kMortonBits = 20;         // per axis
constexpr int kKeyBits = 62;            // 60 Morton bits + 2 class bits: the sort's end bit
constexpr uint32_t kNoSlot = 0xffu;
constexpr uint32_t kTreeletPrims = 256; // the SAH pass's subtree size: one workgroup, one primitive per thread

// How the 60 Morton bits are split across the axes: w bits for axis 2, (60 - w) / 2 for
// axes 0 and 1 each. From the top the key interleaves pairs of axes 0 and 1 (axis 0
// higher) - the bits they have more than axis 2 - then w triples (axis 0 highest).
// w = kMortonBits is the world's 20 / 20 / 20.
struct KeyLayout {
    int w;
};
constexpr KeyLayout kWorldLayout = { kMortonBits };
// The light-space key's split (EXPERIMENTS.md "Device LBVH build": the cheapest of the
// candidates by sun_shadow_cost on the soup and the city block)
constexpr int kSunKeyBitsW = 18;

ARK_LBVH_FN int axisBits(const KeyLayout& L, int a) { return a == 2 ? L.w : (60 - L.w) / 2; }

// Of the top p Morton bits of a key, the number that belong to each axis
ARK_LBVH_FN void prefixBits(const KeyLayout& L, int p, int n[3])
{
    const int pairs = (60 - L.w) / 2 - L.w; // top bits of axes 0 and 1 that stand in pairs
    if (p <= 2 * pairs) {
        n[0] = (p + 1) / 2;
        n[1] = p / 2;
        n[2] = 0;
    } else {
        const int q = p - 2 * pairs;
        n[0] = pairs + (q + 2) / 3;
        n[1] = pairs + (q + 1) / 3;
        n[2] = q / 3;
    }
}

// The key's bit that holds bit b (0: the lowest) of axis a's cell
ARK_LBVH_FN int keyBit(const KeyLayout& L, int a, int b)
{
    if (a == 2) return 3 * b;
    if (b < L.w) return 3 * b + (2 - a);
    return 3 * L.w + 2 * (b - L.w) + (1 - a);
}

// Which slots the members of a node take (assignSlots)
enum SlotRule : int {
    kSlotsOctant = 0,     // the world BVHs: rays of every direction, visited in slot ^ ray octant order
    kSlotsAscendingW = 1, // the sun's BVH: every ray along +w, visited in slot order
};

// A member of a cut: the sorted primitives [first, last] (global indices)
struct Range {
    uint32_t first, last;
};
ARK_LBVH_FN uint32_t count(const Range& r) { return r.last - r.first + 1u; }

// Which member of a cut is opened next
enum Criterion : int {
    kOpenLargestCount = 0, // most triangles
    kOpenLargestCell = 1,  // largest surface area of the range's Morton cell
    kOpenLargestBox = 2,   // (the SAH pass) a member of at most kTreeletPrims by its stored box's half-area, a larger one by its cell
};
// The default (EXPERIMENTS.md "Device LBVH build"): the cell area, the nearest an LBVH
// has to the host collapse's largest-box-area opening; by the host check's BVH8 SAH cost
// on the 20,000-triangle soup it beats the count.
constexpr int kDefaultCriterion = kOpenLargestCell;

ARK_LBVH_FN int clz64(uint64_t x)
{
    return x ? __builtin_clzll(x) : 64;
}

// fp32 as a word whose unsigned order is the numbers' (-0 below +0, a NaN above or below
// everything by its sign), and back
ARK_LBVH_FN uint32_t ordered(float f)
{
    union {
        float f;
        uint32_t u;
    } s;
    s.f = f;
    return (s.u & 0x80000000u) ? ~s.u : (s.u | 0x80000000u);
}
ARK_LBVH_FN float orderedFloat(uint32_t u)
{
    union {
        uint32_t u;
        float f;
    } s;
    // the top bit cleared when it is set, every bit flipped otherwise
    s.u = u ^ (0xffffffffu ^ (static_cast<uint32_t>(static_cast<int32_t>(u) >> 31) & 0x7fffffffu));
    return s.f;
}

// The SAH pass -----------------------------------------------------------------------
// What the pass leaves to the collapse: a box per BVH2 node of more than kBvh8MaxLeafSize
// and at most kTreeletPrims primitives (nbox, 6 floats per node index: lo, hi), a box per
// sorted primitive (pbox, 6 floats), and the scene box the keys were taken in
struct SahBoxes {
    const float* nbox;
    const float* pbox;
    float lo[3], hi[3];
};

// The word the primitives of a treelet are sorted by along one axis (ties: the lower
// position in the Morton order): lo + hi of the primitive's box, in fp32
ARK_LBVH_FN uint32_t sweepKey(float lo, float hi)
{
    const float s = lo + hi;
    return s == s ? ordered(s) : 0xffffffffu; // (a NaN's sign and payload differ between host and device)
}

// Half the surface area of a box given as ordered words (lo xyz, hi xyz)
ARK_LBVH_FN float halfArea(const uint32_t b[6])
{
    const float dx = orderedFloat(b[3]) - orderedFloat(b[0]), dy = orderedFloat(b[4]) - orderedFloat(b[1]), dz = orderedFloat(b[5]) - orderedFloat(b[2]);
    return dx * dy + dy * dz + dz * dx;
}
ARK_LBVH_FN float halfArea(const float lo[3], const float hi[3])
{
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return dx * dy + dy * dz + dz * dx;
}

// A candidate split of a segment of n primitives (the first k of `axis`'s order to the
// left), as a word whose minimum is the chosen one: the least cost areaL k + areaR (n - k)
// (fp32, no contraction), ties to the k nearest n / 2, then the lower k, then the lower
// axis. A cost that is not a finite number is no candidate (kNoSplit's upper word); a
// segment without one splits at the middle of axis 0's order (chosenSplit). The tie rule
// keeps coincident triangles from peeling 1 | n - 1, level after level.
constexpr uint64_t kNoSplit = ~uint64_t(0);
ARK_LBVH_FN uint64_t splitKey(float areaL, float areaR, uint32_t k, uint32_t n, uint32_t axis)
{
    const float c = areaL * static_cast<float>(k) + areaR * static_cast<float>(n - k);
    if (!(c >= 0.0f && c < __builtin_inff())) return kNoSplit;
    union {
        float f;
        uint32_t u;
    } s;
    s.f = c;
    const uint32_t off = 2u * k > n ? 2u * k - n : n - 2u * k;
    return static_cast<uint64_t>(s.u & 0x7fffffffu) << 32 | static_cast<uint64_t>(off) << 20 | static_cast<uint64_t>(k) << 8 | axis;
}
ARK_LBVH_FN void chosenSplit(uint64_t best, uint32_t n, uint32_t& axis, uint32_t& k)
{
    if ((best >> 32) == 0xffffffffu) {
        axis = 0;
        k = n / 2u;
    } else {
        axis = static_cast<uint32_t>(best & 0xffu);
        k = static_cast<uint32_t>(best >> 8) & 0xfffu;
    }
}

ARK_LBVH_FN uint64_t spread20(uint32_t v)
{
    // bit k of v to bit 3 k
    uint64_t x = v & 0xfffffu;
    x = (x | x << 32) & 0x001f00000000ffffull;
    x = (x | x << 16) & 0x001f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// The 20-bit cell of coordinate c in [lo, lo + extent]: scale = 2^20 / extent (0 for a flat box)
ARK_LBVH_FN uint32_t mortonCell(float c, float lo, float scale)
{
    float q = (c - lo) * scale;
    q = q > 0.0f ? q : 0.0f; // NaN to 0
    q = q < 1048575.0f ? q : 1048575.0f;
    return static_cast<uint32_t>(q);
}

ARK_LBVH_FN float mortonScale(float lo, float hi)
{
    const float ext = hi - lo;
    return ext > 0.0f ? 1048576.0f / ext : 0.0f;
}

ARK_LBVH_FN uint64_t mortonKey(const float c[3], const float lo[3], const float scale[3], uint32_t cls)
{
    const uint64_t m = spread20(mortonCell(c[0], lo[0], scale[0])) << 2 | spread20(mortonCell(c[1], lo[1], scale[1])) << 1 |
                       spread20(mortonCell(c[2], lo[2], scale[2]));
    return static_cast<uint64_t>(cls) << 60 | m;
}

// The light coordinates of a record's three vertices (v0, v0 + e1, v0 + e2 in double, each
// rotated into the frame F - rows u, v, w - in double and rounded to fp32) and the largest
// |world coordinate|: what build_sun_bvh boxes, the refit of the light-space BVH boxes
// again (k_refit_nodes) and the device build's keys and scene box are taken from.
ARK_LBVH_FN void lightVertices(const float v0[3], const float e1[3], const float e2[3], const double* F, float L[3][3], float& maxAbs)
{
    double V[3][3];
    maxAbs = 0.0f;
    for (int a = 0; a < 3; ++a) {
        V[0][a] = v0[a];
        V[1][a] = V[0][a] + static_cast<double>(e1[a]);
        V[2][a] = V[0][a] + static_cast<double>(e2[a]);
        double m = __builtin_fabs(V[0][a]);
        for (int k = 1; k < 3; ++k) m = m < __builtin_fabs(V[k][a]) ? __builtin_fabs(V[k][a]) : m;
        const float mf = static_cast<float>(m);
        maxAbs = maxAbs < mf ? mf : maxAbs;
    }
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r) L[k][r] = static_cast<float>(F[3 * r + 0] * V[k][0] + F[3 * r + 1] * V[k][1] + F[3 * r + 2] * V[k][2]);
}

// The cell of coordinate c in [lo, lo + extent] on a grid of 2^bits cells: scale = 2^bits / extent
ARK_LBVH_FN float layoutScale(float lo, float hi, int bits)
{
    const float ext = hi - lo;
    union {
        uint32_t u;
        float f;
    } s;
    s.u = static_cast<uint32_t>(127 + bits) << 23;
    return ext > 0.0f ? s.f / ext : 0.0f;
}

ARK_LBVH_FN uint32_t layoutCell(float c, float lo, float scale, int bits)
{
    float q = (c - lo) * scale;
    q = q > 0.0f ? q : 0.0f; // NaN to 0
    const uint32_t last = (1u << bits) - 1u;
    return q < static_cast<float>(last) ? static_cast<uint32_t>(q) : last;
}

// The light-space key: the Morton code (layout L) of the centre c of a record's light-space
// box inside the scene's light-space box; the class bits are 0 (one tree for all classes)
ARK_LBVH_FN uint64_t lightKey(const float c[3], const float lo[3], const float hi[3], const KeyLayout& L)
{
    uint64_t key = 0;
    for (int a = 0; a < 3; ++a) {
        const int bits = axisBits(L, a);
        const uint32_t cell = layoutCell(c[a], lo[a], layoutScale(lo[a], hi[a], bits), bits);
        for (int b = 0; b < bits; ++b) key |= static_cast<uint64_t>((cell >> b) & 1u) << keyBit(L, a, b);
    }
    return key;
}

// Length of the common prefix of the (key, index) pairs i and j of the class range
// [lo, hi); -1 when j lies outside it
ARK_LBVH_FN int delta(const uint64_t* keys, uint32_t lo, uint32_t hi, uint32_t i, int64_t j)
{
    if (j < static_cast<int64_t>(lo) || j >= static_cast<int64_t>(hi)) return -1;
    const uint64_t a = keys[i], b = keys[j];
    if (a != b) return clz64(a ^ b);
    return 64 + (clz64(static_cast<uint64_t>(i ^ static_cast<uint32_t>(j))) - 32);
}

// The range of internal node i of the class range [lo, hi) (hi - lo >= 2, lo <= i < hi - 1)
ARK_LBVH_FN Range nodeRange(const uint64_t* keys, uint32_t lo, uint32_t hi, uint32_t i)
{
    const int64_t I = i;
    const int d = delta(keys, lo, hi, i, I + 1) - delta(keys, lo, hi, i, I - 1) >= 0 ? 1 : -1;
    const int dmin = delta(keys, lo, hi, i, I - d);
    int64_t lmax = 2;
    while (delta(keys, lo, hi, i, I + lmax * d) > dmin) lmax <<= 1;
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, lo, hi, i, I + (l + t) * d) > dmin) l += t;
    const int64_t j = I + l * d;
    Range r;
    r.first = static_cast<uint32_t>(d > 0 ? I : j);
    r.last = static_cast<uint32_t>(d > 0 ? j : I);
    return r;
}

// The last primitive of the left child of the node covering r (r.first < r.last)
ARK_LBVH_FN uint32_t findSplit(const uint64_t* keys, uint32_t lo, uint32_t hi, const Range& r)
{
    const int dnode = delta(keys, lo, hi, r.first, r.last);
    uint32_t split = r.first, step = r.last - r.first;
    do {
        step = (step + 1u) >> 1;
        const uint32_t m = split + step;
        if (m < r.last && delta(keys, lo, hi, r.first, m) > dnode) split = m;
    } while (step > 1u);
    return split;
}

// The BVH2 internal node of a range of more than one primitive that is not a class's
// root: a left child ends at its own index, a right child starts at it
ARK_LBVH_FN uint32_t leftNode(const Range& r) { return r.last; }
ARK_LBVH_FN uint32_t rightNode(const Range& r) { return r.first; }

// A cut member while the cut is chosen: its range and its BVH2 internal node
struct Member {
    Range r;
    uint32_t node;
};

// The Morton cell of a range: the axis-wise cell counts (log2) the common prefix of its
// first and last key leaves free, as a relative surface area (extent: the scene box's)
ARK_LBVH_FN float cellArea(const uint64_t* keys, const Range& r, const float extent[3], const KeyLayout& L = kWorldLayout)
{
    const uint64_t x = (keys[r.first] ^ keys[r.last]) << 4; // the class bits are equal
    const int p = x ? clz64(x) : 60;                         // common Morton bits, x first
    int n[3];
    prefixBits(L, p, n);
    float d[3];
    for (int a = 0; a < 3; ++a) {
        // extent * 2^-n, exactly
        union {
            uint32_t u;
            float f;
        } s;
        s.u = static_cast<uint32_t>(127 - n[a]) << 23;
        d[a] = extent[a] * s.f;
    }
    return d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
}

// The SAH pass's box of a range of at most kTreeletPrims primitives: its node's stored box,
// or the union of a leaf member's primitive boxes
ARK_LBVH_FN void memberBox(const SahBoxes& S, const Member& m, float lo[3], float hi[3])
{
    if (count(m.r) > static_cast<uint32_t>(kBvh8MaxLeafSize)) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = S.nbox[6ull * m.node + a];
            hi[a] = S.nbox[6ull * m.node + 3 + a];
        }
        return;
    }
    uint32_t l[3], h[3];
    for (int a = 0; a < 3; ++a) {
        l[a] = 0xffffffffu;
        h[a] = 0u;
    }
    for (uint32_t j = m.r.first; j <= m.r.last; ++j)
        for (int a = 0; a < 3; ++a) {
            const uint32_t pl = ordered(S.pbox[6ull * j + a]), ph = ordered(S.pbox[6ull * j + 3 + a]);
            l[a] = pl < l[a] ? pl : l[a];
            h[a] = ph > h[a] ? ph : h[a];
        }
    for (int a = 0; a < 3; ++a) {
        lo[a] = orderedFloat(l[a]);
        hi[a] = orderedFloat(h[a]);
    }
}

// A primitive's box from its three vertices, as ordered words (lo xyz, hi xyz)
ARK_LBVH_FN void primBox(const float v[3][3], uint32_t b[6])
{
    for (int a = 0; a < 3; ++a) {
        uint32_t l = ordered(v[0][a]), h = l;
        for (int k = 1; k < 3; ++k) {
            const uint32_t o = ordered(v[k][a]);
            l = o < l ? o : l;
            h = o > h ? o : h;
        }
        b[a] = l;
        b[3 + a] = h;
    }
}

// The treelets that the BVH2 node over r with split s adds to the SAH pass's work list
// (out[0 .. return)): each child of at most kTreeletPrims primitives of a node of more, and
// a class's root of at most kTreeletPrims; none of kBvh8MaxLeafSize or fewer, which the
// collapse never opens. Treelets are disjoint ranges of at least 4 primitives. plan (the
// collapse plan): ranges of 2 and 3 too - then only single primitives lie outside a treelet.
ARK_LBVH_FN int treeletsOf(const Range& r, uint32_t s, bool isRoot, Member out[2], bool plan = false)
{
    const uint32_t least = plan ? 1u : static_cast<uint32_t>(kBvh8MaxLeafSize);
    int n = 0;
    if (count(r) > kTreeletPrims) {
        Member a, b;
        a.r.first = r.first;
        a.r.last = s;
        a.node = leftNode(a.r);
        b.r.first = s + 1u;
        b.r.last = r.last;
        b.node = rightNode(b.r);
        if (count(a.r) <= kTreeletPrims && count(a.r) > least) out[n++] = a;
        if (count(b.r) <= kTreeletPrims && count(b.r) > least) out[n++] = b;
    } else if (isRoot && count(r) > least) {
        out[0].r = r;
        out[0].node = r.first;
        n = 1;
    }
    return n;
}

// A range of n primitives holds n - 1 nodes of its own under the numbering, its root
// included: the index at the end its root's is not at belongs to an ancestor (a class's
// root, whose index is its first, has none there: its last is no node's). The SAH pass
// rewrites split[] at every index of a treelet but this one.
ARK_LBVH_FN uint32_t treeletSpareIndex(const Member& T) { return T.node == T.r.first ? T.r.last : T.r.first; }

// The members of the BVH8 node over `top` (top.node: its BVH2 node when it holds more
// than one primitive): out[0 .. return). A node of at most kBvh8MaxLeafSize triangles
// (only a class's root) is one leaf member. S: the SAH pass's boxes (kOpenLargestBox).
ARK_LBVH_FN int selectCut(const uint64_t* keys, const uint32_t* split, const Member& top, int criterion, const float extent[3], Member out[8],
                          const KeyLayout& L = kWorldLayout, const SahBoxes* S = nullptr)
{
    if (count(top.r) <= static_cast<uint32_t>(kBvh8MaxLeafSize)) {
        out[0] = top;
        return 1;
    }
    int n = 0;
    int open = -1;
    Member cur = top;
    for (;;) {
        // open `cur` into its two children (at position `open`, the second appended)
        const uint32_t sp = split[cur.node];
        Member a, b;
        a.r.first = cur.r.first;
        a.r.last = sp;
        a.node = leftNode(a.r);
        b.r.first = sp + 1u;
        b.r.last = cur.r.last;
        b.node = rightNode(b.r);
        if (open < 0) {
            out[n++] = a;
        } else {
            out[open] = a;
        }
        out[n++] = b;
        if (n == 8) break;
        open = -1;
        float best = -1.0f;
        for (int k = 0; k < n; ++k) {
            if (count(out[k].r) <= static_cast<uint32_t>(kBvh8MaxLeafSize)) continue;
            float v;
            if (criterion == kOpenLargestBox && S && count(out[k].r) <= kTreeletPrims) {
                float lo[3], hi[3];
                memberBox(*S, out[k], lo, hi);
                v = halfArea(lo, hi);
            } else {
                v = criterion == kOpenLargestCell || (criterion == kOpenLargestBox && S) ? cellArea(keys, out[k].r, extent, L) : static_cast<float>(count(out[k].r));
            }
            if (v > best) {
                best = v;
                open = k;
            }
        }
        if (open < 0) break;
        cur = out[open];
    }
    return n;
}

// The collapse plan -----------------------------------------------------------------
// cost[n][i] (C[i - 1]) of a BVH2 node n over cnt primitives with box half-area `area`, from
// its children's (L, R; a single primitive: planLeafCosts): with dist(j) the least
// L[k] + R[j - k] over k = 1 .. j - 1 (the lowest k wins ties), cost[n][1] is
// area kPlanNodeCost + dist(8) - n as a BVH8 node of its own - for more than kBvh8MaxLeafSize
// primitives and area kPlanTriCost cnt - one leaf slot - otherwise (such a range is never an
// internal member), cost[n][i] = min(dist(i), cost[n][i - 1]). fp32, no contraction, left
// then right. Returns the picks, packed: the slots given to the left child at i = 2, 3 (two
// bits each, from bit 0) and i = 4 .. 8 (three bits each, from bit 4), 0: as i - 1; from bit
// 19 those of the node's own 8 (more than kBvh8MaxLeafSize primitives). 22 bits.
constexpr float kPlanNodeCost = 1.0f, kPlanTriCost = 1.0f; // Bvh8CollapseOptions' defaults
constexpr uint32_t kPlanPickBits = 0x3fffffu;
constexpr uint32_t kPlanDone = 0x80000000u;     // the node's word is final
constexpr uint32_t kPlanComputed = 0x40000000u; // (k_lbvh_upper_plan: written this round, final from the next)
ARK_LBVH_FN uint32_t planPickShift(int i) { return i < 4 ? 2u * static_cast<uint32_t>(i - 2) : 4u + 3u * static_cast<uint32_t>(i - 4); }
ARK_LBVH_FN uint32_t planPick(uint32_t word, int i) { return (word >> planPickShift(i)) & (i < 4 ? 3u : 7u); }
ARK_LBVH_FN uint32_t planOwnPick(uint32_t word) { return (word >> 19) & 7u; }

ARK_LBVH_FN void planLeafCosts(const uint32_t box[6], float C[8])
{
    const float c = halfArea(box) * kPlanTriCost;
    for (int i = 0; i < 8; ++i) C[i] = c;
}

template <int J>
ARK_LBVH_FN float planDist(const float L[8], const float R[8], uint32_t& bestK)
{
    float best = L[0] + R[J - 2];
    bestK = 1u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 2; k < J; ++k) {
        const float v = L[k - 1] + R[J - k - 1];
        if (v < best) {
            best = v;
            bestK = static_cast<uint32_t>(k);
        }
    }
    return best;
}

template <int I>
ARK_LBVH_FN void planStep(const float L[8], const float R[8], float C[8], uint32_t& word)
{
    uint32_t k;
    const float d = planDist<I>(L, R, k);
    if (d < C[I - 2]) {
        C[I - 1] = d;
        word |= k << planPickShift(I);
    } else {
        C[I - 1] = C[I - 2];
    }
}

ARK_LBVH_FN uint32_t planCosts(float area, uint32_t cnt, const float L[8], const float R[8], float C[8])
{
    uint32_t word = 0;
    if (cnt > static_cast<uint32_t>(kBvh8MaxLeafSize)) {
        uint32_t k8;
        const float d = planDist<8>(L, R, k8);
        C[0] = area * kPlanNodeCost + d;
        word = k8 << 19;
    } else {
        C[0] = area * kPlanTriCost * static_cast<float>(cnt);
    }
    planStep<2>(L, R, C, word);
    planStep<3>(L, R, C, word);
    planStep<4>(L, R, C, word);
    planStep<5>(L, R, C, word);
    planStep<6>(L, R, C, word);
    planStep<7>(L, R, C, word);
    planStep<8>(L, R, C, word);
    return word;
}

// A node above the treelets: its box (ordered words) the union of its children's, its plan
// from theirs
ARK_LBVH_FN uint32_t planUpperNode(const uint32_t lb[6], const float L[8], const uint32_t rb[6], const float R[8], uint32_t cnt, uint32_t box[6], float C[8])
{
    for (int a = 0; a < 3; ++a) {
        box[a] = lb[a] < rb[a] ? lb[a] : rb[a];
        box[3 + a] = lb[3 + a] > rb[3 + a] ? lb[3 + a] : rb[3 + a];
    }
    return planCosts(halfArea(box), cnt, L, R, C);
}

// The two children of the BVH2 node of m (more than one primitive) under the numbering
ARK_LBVH_FN void childrenOf(const uint32_t* split, const Member& m, Member& a, Member& b)
{
    const uint32_t sp = split[m.node];
    a.r.first = m.r.first;
    a.r.last = sp;
    a.node = leftNode(a.r);
    b.r.first = sp + 1u;
    b.r.last = m.r.last;
    b.node = rightNode(b.r);
}

// selectCut by the plan: the members of the BVH8 node over `top`, in left-to-right range
// order. From top's own 8-way distribution down, with a stack of at most 8 (the slots on it
// sum to at most 8): a range that reaches i = 1, or a single primitive, is a member - an
// internal one if it holds more than kBvh8MaxLeafSize primitives; a pick of 0 is "as i - 1".
// A pick outside 1 .. i - 1 (never: planCosts writes none) is taken as the nearest inside.
ARK_LBVH_FN int planCut(const uint32_t* split, const uint32_t* picks, const Member& top, Member out[8])
{
    if (count(top.r) <= static_cast<uint32_t>(kBvh8MaxLeafSize)) {
        out[0] = top;
        return 1;
    }
    Member stack[8];
    uint32_t slots[8];
    int sp = 0, n = 0;
    Member cur = top;
    uint32_t i = 8u, k = planOwnPick(picks[top.node]);
    for (;;) {
        // `cur` shares its i slots between its children: k to the left one
        k = k < 1u ? 1u : k > i - 1u ? i - 1u : k;
        Member a, b;
        childrenOf(split, cur, a, b);
        stack[sp] = b;
        slots[sp++] = i - k;
        stack[sp] = a;
        slots[sp++] = k;
        bool opened = false;
        while (sp > 0 && !opened) {
            cur = stack[--sp];
            i = slots[sp];
            k = 0u;
            if (count(cur.r) > 1u) {
                const uint32_t word = picks[cur.node];
                while (i >= 2u && (k = planPick(word, static_cast<int>(i))) == 0u) --i;
            }
            if (count(cur.r) > 1u && i >= 2u) {
                opened = true;
            } else if (n < 8) {
                out[n++] = cur;
            }
        }
        if (!opened) break;
    }
    return n;
}

// The Morton cell of a range per axis: its low edge in cells of the axis's finest grid and
// the log2 of its width in them
ARK_LBVH_FN void cellBounds(const uint64_t* keys, const Range& r, const KeyLayout& L, int64_t lo[3], int free[3])
{
    const uint64_t k = keys[r.first];
    const uint64_t x = (k ^ keys[r.last]) << 4;
    const int p = x ? clz64(x) : 60;
    int n[3];
    prefixBits(L, p, n);
    for (int a = 0; a < 3; ++a) {
        // the axis's bits of the first key, its low (bits - n) ones cleared
        const int bits = axisBits(L, a);
        uint32_t v = 0;
        for (int b = 0; b < bits; ++b) v |= static_cast<uint32_t>((k >> keyBit(L, a, b)) & 1u) << b;
        free[a] = bits - n[a];
        lo[a] = static_cast<int64_t>(v >> free[a]) << free[a];
    }
}

// The centre of a range's Morton cell in half cells of the finest grid, per axis
ARK_LBVH_FN void cellCentre(const uint64_t* keys, const Range& r, int64_t c[3], const KeyLayout& L = kWorldLayout)
{
    int64_t lo[3];
    int free[3];
    cellBounds(keys, r, L, lo, free);
    for (int a = 0; a < 3; ++a) c[a] = 2 * lo[a] + (int64_t(1) << free[a]);
}

// Slots of a node's members. Internal members (more than kBvh8MaxLeafSize triangles) take
// the octant slot of their cell's centre relative to the node's cell's centre (bit a of
// the slot: the + side along axis a), a taken one the nearest free slot (fewest differing
// axes, then the lowest). Leaf members decide only which triangles a hit slot adds, so
// they fill the free slots in ascending order, most triangles first, which keeps the
// node's rows compact (as the host collapse does). slotOf[k]: the slot of member k.
// kSlotsAscendingW (the sun's BVH, whose rays all go along +w and visit a node's children
// in slot order, as the host collapse's slot_sort_axis = 2): internal and leaf members
// alike take slots 0, 1, ... in ascending order of the low w edge of their Morton cell,
// ties to the lower first key; placeRows finds rows for any such assignment (stride 8).
// Under the SAH pass (S, with parentNode the BVH2 node of `node`) a member or parent of at
// most kTreeletPrims primitives is no whole Morton cell any more: its centre is that of its
// stored box (rangeCentre), its low w edge that of its box (memberLowW; a leaf member's box
// the union of its primitives'). Larger ranges keep their cells; all else is unchanged.
ARK_LBVH_FN void rangeCentre(const uint64_t* keys, const Member& m, int64_t c[3], const SahBoxes* S)
{
    if (!S || count(m.r) > kTreeletPrims) return cellCentre(keys, m.r, c);
    float lo[3], hi[3];
    memberBox(*S, m, lo, hi);
    for (int a = 0; a < 3; ++a) c[a] = 2 * static_cast<int64_t>(mortonCell(0.5f * lo[a] + 0.5f * hi[a], S->lo[a], mortonScale(S->lo[a], S->hi[a]))) + 1;
}

ARK_LBVH_FN int64_t memberLowW(const uint64_t* keys, const Member& m, const KeyLayout& L, const SahBoxes* S)
{
    if (!S || count(m.r) > kTreeletPrims) {
        int64_t lo[3];
        int free[3];
        cellBounds(keys, m.r, L, lo, free);
        return lo[2];
    }
    float lo[3], hi[3];
    memberBox(*S, m, lo, hi);
    const int bits = axisBits(L, 2);
    return static_cast<int64_t>(layoutCell(lo[2], S->lo[2], layoutScale(S->lo[2], S->hi[2], bits), bits));
}

ARK_LBVH_FN void assignSlots(const uint64_t* keys, const Range& node, const Member* m, int n, uint32_t slotOf[8], int rule = kSlotsOctant,
                             const KeyLayout& L = kWorldLayout, const SahBoxes* S = nullptr, uint32_t parentNode = 0)
{
    if (rule == kSlotsAscendingW) {
        int64_t low[8];
        for (int k = 0; k < n; ++k) low[k] = memberLowW(keys, m[k], L, S);
        for (int k = 0; k < n; ++k) {
            uint32_t rank = 0;
            for (int j = 0; j < n; ++j)
                if (low[j] < low[k] || (low[j] == low[k] && m[j].r.first < m[k].r.first)) ++rank;
            slotOf[k] = rank;
        }
        return;
    }
    uint32_t taken = 0;
    int64_t pc[3];
    Member parent;
    parent.r = node;
    parent.node = parentNode;
    rangeCentre(keys, parent, pc, S);
    for (int k = 0; k < n; ++k) {
        slotOf[k] = kNoSlot;
        if (count(m[k].r) <= static_cast<uint32_t>(kBvh8MaxLeafSize)) continue;
        int64_t c[3];
        rangeCentre(keys, m[k], c, S);
        const uint32_t want = (c[0] > pc[0] ? 1u : 0u) | (c[1] > pc[1] ? 2u : 0u) | (c[2] > pc[2] ? 4u : 0u);
        uint32_t bestSlot = 0, bestDist = 99;
        for (uint32_t s = 0; s < 8u; ++s) {
            if ((taken >> s) & 1u) continue;
            const uint32_t x = s ^ want;
            const uint32_t dist = (x & 1u) + ((x >> 1) & 1u) + ((x >> 2) & 1u);
            if (dist < bestDist) {
                bestDist = dist;
                bestSlot = s;
            }
        }
        slotOf[k] = bestSlot;
        taken |= 1u << bestSlot;
    }
    for (uint32_t c = static_cast<uint32_t>(kBvh8MaxLeafSize); c >= 1u; --c)
        for (int k = 0; k < n; ++k) {
            if (slotOf[k] != kNoSlot || count(m[k].r) != c) continue;
            uint32_t s = 0;
            while ((taken >> s) & 1u) ++s;
            slotOf[k] = s;
            taken |= 1u << s;
        }
}

// The rows of one node's leaf slots (cnt[s] triangles in slot s, 0: not a leaf slot)
struct Rows {
    uint32_t stride;    // tri_stride
    uint32_t leaf_tris; // bit s + stride i: triangle i of slot s
    uint32_t leaf_mask;
    uint32_t span;      // highest used position + 1 (0: no leaf slot)
};

// The smallest stride in 1..8 under which every position s + stride i (i < 3) of a leaf
// slot s is free or s's own triangle i, and the rows fit in 24 positions (GpuBvh8Node;
// bvh_builder.cpp leafRowStride). The node's rows are private: positions 0 .. span - 1
// from its tri_base belong to it alone.
ARK_LBVH_FN Rows placeRows(const uint32_t cnt[8])
{
    Rows r;
    r.leaf_mask = 0;
    for (uint32_t s = 0; s < 8u; ++s)
        if (cnt[s]) r.leaf_mask |= 1u << s;
    for (uint32_t st = 1u; st <= 8u; ++st) {
        uint32_t used = 0;
        bool ok = true;
        for (uint32_t s = 0; s < 8u && ok; ++s)
            for (uint32_t i = 0; i < cnt[s] && ok; ++i) {
                const uint32_t p = s + st * i;
                ok = p < 24u && !((used >> p) & 1u);
                used |= ok ? 1u << p : 0u;
            }
        for (uint32_t s = 0; s < 8u && ok; ++s) {
            if (!cnt[s]) continue;
            uint32_t own = 0;
            for (uint32_t i = 0; i < cnt[s]; ++i) own |= 1u << (s + st * i);
            const uint32_t spread = bvh8SlotRow(st, static_cast<int>(s)) & 0xffffffu;
            ok = ((spread & used) & ~own) == 0u;
        }
        if (ok || st == 8u) {
            r.stride = st;
            r.leaf_tris = used;
            break;
        }
    }
    r.span = 0;
    for (uint32_t p = 0; p < 24u; ++p)
        if ((r.leaf_tris >> p) & 1u) r.span = p + 1u;
    return r;
}

// One BVH8 node of the collapse: what selectCut, assignSlots and placeRows decide
struct WideNode {
    Member member[8];
    uint32_t slotOf[8];
    int members;
    uint32_t imask;     // slots of internal members
    uint32_t internal;  // popcount(imask)
    Rows rows;
};

ARK_LBVH_FN void planNode(const uint64_t* keys, const uint32_t* split, const Member& top, int criterion, const float extent[3], WideNode& w,
                          int slotRule = kSlotsOctant, const KeyLayout& L = kWorldLayout, const SahBoxes* S = nullptr, const uint32_t* picks = nullptr)
{
    w.members = picks ? planCut(split, picks, top, w.member) : selectCut(keys, split, top, criterion, extent, w.member, L, S);
    assignSlots(keys, top.r, w.member, w.members, w.slotOf, slotRule, L, S, top.node);
    uint32_t cnt[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    w.imask = 0;
    w.internal = 0;
    for (int k = 0; k < w.members; ++k) {
        const uint32_t c = count(w.member[k].r);
        if (c <= static_cast<uint32_t>(kBvh8MaxLeafSize)) {
            cnt[w.slotOf[k]] = c;
        } else {
            w.imask |= 1u << w.slotOf[k];
            w.internal++;
        }
    }
    w.rows = placeRows(cnt);
}

// The member in slot s (-1: none)
ARK_LBVH_FN int memberInSlot(const WideNode& w, uint32_t s)
{
    for (int k = 0; k < w.members; ++k)
        if (w.slotOf[k] == s) return k;
    return -1;
}

} // namespace lbvh
} // namespace ark
