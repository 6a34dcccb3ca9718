// ddgi_bvh_build.hip — the world BVH8s' topology built on the device from a snapshot of
// the triangle records (lbvh_device_build.cpp buildLbvhGpu, ARK_DDGI_FLAG_GPU_REBUILD): an
// LBVH (Karras 2012) per hit-mask class, collapsed into 8-wide nodes level by level.
// The decisions are lbvh_build.h's (shared with the host check
// ark_ddgi_debug_lbvh_check); the boxes, grids and planes are k_refit_nodes'
// (ddgi_scene_update.hip), run over every level afterwards.
//
//   k_lbvh_prims      one thread per snapshot record: holes skipped, the survivors'
//                     record indices compacted, the per-class counts, the all-class
//                     scene box of the vertices (wave reduction, then atomics)
//   k_lbvh_keys       class << 60 | Morton code of each survivor's centroid
//   k_lbvh_prims_light / k_lbvh_keys_light   the same for the sun's light-space BVH8
//                     (ARK_DDGI_FLAG_GPU_REBUILD_SUN): one tree over every class, the box
//                     and the keys of the records' light coordinates, the largest |world
//                     coordinate|; the survivors compacted by one ballot and one atomic add
//                     per wave
//   (rocPRIM radix_sort_pairs over the 62 key bits)
//   k_lbvh_hierarchy  one thread per BVH2 internal node of a class range: its split; under
//                     ARK_DDGI_FLAG_GPU_REBUILD_SAH also the treelets it is the parent of,
//                     appended to the SAH pass's work list (one atomic add each)
//   k_lbvh_treelet_sah  (that flag only) one workgroup per treelet of at most
//                     lbvh::kTreeletPrims primitives: its binary tree rebuilt by a
//                     three-axis sweep SAH in LDS, its primitives reordered, a box per node
//                     and primitive for the collapse's decisions (lbvh_build.h)
//   k_lbvh_upper_plan  (ARK_DDGI_FLAG_GPU_REBUILD_PLAN, with the SAH pass, whose plan instance
//                     splits down to single primitives and plans the treelets' nodes) one
//                     workgroup: boxes and collapse plans of the nodes above the treelets, in
//                     rounds with a barrier between them; the collapse then cuts by the picks
//   k_lbvh_collapse   one level of one class, one thread per BVH8 node of the work
//                     list: cut, slots and rows; the internal children's node indices
//                     from one atomic add on the next level's counter, the rows' span
//                     from one on the record counter; the next level's work list
//   k_lbvh_fill / k_lbvh_scatter   hole records everywhere, then every record copied
//                     bit for bit from the snapshot to its row position, perm
//
// No kernel here waits on, polls or spins on another workgroup: all ordering between
// workgroups is by kernel boundaries on the job's stream. Atomics only allocate and
// reduce, and a returned value is consumed by the thread that got it.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "ddgi_kernels.h"
#include "lbvh_build.h"

namespace ark {
namespace dev {

// fp32 in an unsigned order (for integer atomic min / max)
__device__ __forceinline__ uint32_t orderedBits(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void recordVertices(const GpuTriangle* __restrict__ rec, float v[3][3], uint32_t& instance)
{
    const float4* q = reinterpret_cast<const float4*>(rec);
    const float4 a = q[0], b = q[1], c = q[2];
    instance = __float_as_uint(c.y);
    const float v0[3] = { a.x, a.y, a.z }, e1[3] = { a.w, b.x, b.y }, e2[3] = { b.z, b.w, c.x };
    for (int k = 0; k < 3; ++k) {
        v[0][k] = v0[k];
        v[1][k] = v0[k] + e1[k];
        v[2][k] = v0[k] + e2[k];
    }
}

__global__ void __launch_bounds__(256) k_lbvh_prims(const GpuTriangle* __restrict__ snap, uint32_t records, const uint32_t* __restrict__ classOf,
                                                    uint32_t instances, uint32_t* __restrict__ idx, LbvhHeader* __restrict__ hdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (i < records) {
        float v[3][3];
        uint32_t inst;
        recordVertices(snap + i, v, inst);
        if (inst != kHoleInstance) {
            if (inst >= instances) {
                atomicOr(&hdr->error, kLbvhErrorInstance);
            } else {
                idx[atomicAdd(&hdr->prims, 1u)] = i; // at most `records` survivors: in bounds
                atomicAdd(&hdr->classCount[classOf[inst]], 1u);
                for (int a = 0; a < 3; ++a) {
                    lo[a] = fminf(v[0][a], fminf(v[1][a], v[2][a]));
                    hi[a] = fmaxf(v[0][a], fmaxf(v[1][a], v[2][a]));
                }
            }
        }
    }
    for (int m = 1; m < 64; m <<= 1)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], m, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m, 64));
        }
    if ((threadIdx.x & 63u) == 0u && lo[0] <= hi[0])
        for (int a = 0; a < 3; ++a) {
            atomicMin(&hdr->lo[a], orderedBits(lo[a]));
            atomicMax(&hdr->hi[a], orderedBits(hi[a]));
        }
}

__device__ __forceinline__ float fromOrdered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__global__ void __launch_bounds__(256) k_lbvh_keys(const GpuTriangle* __restrict__ snap, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ classOf,
                                                   const LbvhHeader* __restrict__ hdr, uint64_t* __restrict__ keys)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= hdr->prims) return;
    float v[3][3];
    uint32_t inst;
    recordVertices(snap + idx[j], v, inst);
    float lo[3], scale[3], c[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = fromOrdered(hdr->lo[a]);
        scale[a] = lbvh::mortonScale(lo[a], fromOrdered(hdr->hi[a]));
        // the centre of the triangle's box
        c[a] = 0.5f * fminf(v[0][a], fminf(v[1][a], v[2][a])) + 0.5f * fmaxf(v[0][a], fmaxf(v[1][a], v[2][a]));
    }
    keys[j] = lbvh::mortonKey(c, lo, scale, classOf[inst]);
}

// A record's light-space box (lbvh::lightVertices: the coordinates build_sun_bvh and the
// refit box) and its largest |world coordinate|
__device__ __forceinline__ void recordLightBox(const GpuTriangle* __restrict__ rec, const double* F, float lo[3], float hi[3], float& maxAbs, uint32_t& instance)
{
    const float4* q = reinterpret_cast<const float4*>(rec);
    const float4 a = q[0], b = q[1], c = q[2];
    instance = __float_as_uint(c.y);
    const float v0[3] = { a.x, a.y, a.z }, e1[3] = { a.w, b.x, b.y }, e2[3] = { b.z, b.w, c.x };
    float L[3][3];
    lbvh::lightVertices(v0, e1, e2, F, L, maxAbs);
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(L[0][k], fminf(L[1][k], L[2][k]));
        hi[k] = fmaxf(L[0][k], fmaxf(L[1][k], L[2][k]));
    }
}

__global__ void __launch_bounds__(256) k_lbvh_prims_light(const GpuTriangle* __restrict__ snap, uint32_t records, uint32_t instances, LbvhFrame frame,
                                                          uint32_t* __restrict__ idx, LbvhHeader* __restrict__ hdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    float maxAbs = 0.0f;
    bool live = false;
    if (i < records) {
        const uint32_t inst = __float_as_uint(reinterpret_cast<const float4*>(snap + i)[2].y);
        if (inst != kHoleInstance) {
            if (inst >= instances) {
                atomicOr(&hdr->error, kLbvhErrorInstance);
            } else {
                uint32_t unused;
                recordLightBox(snap + i, frame.m, lo, hi, maxAbs, unused);
                live = true;
            }
        }
    }
    // the survivors' record indices: a rank within the wave, one atomic add per wave
    const uint64_t alive = __ballot(live);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(alive >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(alive), 0u));
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0u && alive) base = atomicAdd(&hdr->prims, static_cast<uint32_t>(__popcll(alive)));
    base = __shfl(base, 0, 64);
    if (live) idx[base + rank] = i; // at most `records` survivors: in bounds
    for (int m = 1; m < 64; m <<= 1) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], m, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m, 64));
        }
        maxAbs = fmaxf(maxAbs, __shfl_xor(maxAbs, m, 64));
    }
    if ((threadIdx.x & 63u) == 0u && alive) {
        for (int a = 0; a < 3; ++a) {
            atomicMin(&hdr->lo[a], orderedBits(lo[a]));
            atomicMax(&hdr->hi[a], orderedBits(hi[a]));
        }
        atomicMax(&hdr->maxAbs, __float_as_uint(maxAbs));
    }
}

__global__ void __launch_bounds__(256) k_lbvh_keys_light(const GpuTriangle* __restrict__ snap, const uint32_t* __restrict__ idx, const LbvhHeader* __restrict__ hdr,
                                                         LbvhFrame frame, int wBits, uint64_t* __restrict__ keys)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= hdr->prims) return;
    float blo[3], bhi[3], m, lo[3], hi[3], c[3];
    uint32_t inst;
    recordLightBox(snap + idx[j], frame.m, blo, bhi, m, inst);
    for (int a = 0; a < 3; ++a) {
        lo[a] = fromOrdered(hdr->lo[a]);
        hi[a] = fromOrdered(hdr->hi[a]);
        c[a] = 0.5f * blo[a] + 0.5f * bhi[a]; // the centre of the triangle's light-space box
    }
    const lbvh::KeyLayout layout = { wBits };
    keys[j] = lbvh::lightKey(c, lo, hi, layout);
}

// kPlan (the collapse plan): ranges of 2 and 3 primitives are treelets too, and a node of more
// than lbvh::kTreeletPrims is appended to the list of the nodes above the treelets
template <bool kPlan>
__global__ void __launch_bounds__(256) k_lbvh_hierarchy(const uint64_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint32_t* __restrict__ split,
                                                        lbvh::Member* __restrict__ treelets, uint32_t treeletCapacity, uint32_t* __restrict__ counters,
                                                        lbvh::Member* __restrict__ upper, uint32_t upperCapacity)
{
    const uint32_t i = lo + blockIdx.x * 256u + threadIdx.x;
    if (i + 1u >= hi) return; // internal nodes lo .. hi - 2
    const lbvh::Range r = lbvh::nodeRange(keys, lo, hi, i);
    const uint32_t s = lbvh::findSplit(keys, lo, hi, r);
    split[i] = s;
    if (!treelets) return;
    // the SAH pass's work list (its order does not matter: treelets are disjoint ranges)
    lbvh::Member m[2];
    const int n = lbvh::treeletsOf(r, s, i == lo, m, kPlan);
    for (int k = 0; k < n; ++k) {
        const uint32_t at = atomicAdd(&counters[kLbvhTreelets], 1u);
        if (at < treeletCapacity) treelets[at] = m[k];
        else atomicOr(&counters[kLbvhOverflow], 1u); // (never: at most prims / 4 treelets, prims / 2 under the plan)
    }
    if (kPlan && lbvh::count(r) > lbvh::kTreeletPrims) {
        const uint32_t at = atomicAdd(&counters[kLbvhUpper], 1u);
        if (at < upperCapacity) {
            lbvh::Member u;
            u.r = r;
            u.node = i;
            upper[at] = u;
        } else {
            atomicOr(&counters[kLbvhOverflow], 1u); // (never: fewer than prims such nodes)
        }
    }
}

// What the plan instance of k_lbvh_treelet_sah keeps in LDS beside the pass's own: per node
// of the treelet (by its index in the treelet) the eight costs, its box's half-area, its
// range and its done flag
struct PlanLds {
    float cost[8][256];
    float area[256];
    uint8_t first[256], last[256], done[256];
};
__device__ __forceinline__ PlanLds& planLds()
{
    __shared__ PlanLds lds;
    return lds;
}

// The SAH pass: one workgroup per treelet (4 .. 256 primitives), one primitive per thread,
// the treelet's binary tree built top-down in LDS, every level inside the workgroup. The
// primitives stand in three orders (by lo + hi of their boxes along each axis, ties to the
// Morton order); the segments of a level are the same position ranges in all three.
// Per level and axis: segmented prefix and suffix unions of the boxes in that axis's order
// (shuffle scans within a wave, joined across the waves through LDS; unions of ordered
// words, so exact in any order), every candidate's lbvh::splitKey, the segment's least by
// one LDS atomic min; then all three orders stably partitioned by side (ballot ranks).
// Out: sorted[] permuted inside the treelet (axis 0's final order), split[] of the
// treelet's nodes under the radix tree's numbering (entries no node owns: the first of
// their final segment; lbvh::treeletSpareIndex is an ancestor's and left alone), nbox[] of every node of more than kBvh8MaxLeafSize primitives,
// pbox[] of every primitive at its new position. Nothing is read of or written to another
// treelet's range, and no workgroup waits for another.
// kPlan (the collapse plan; treelets of 2 primitives or more): the instance that keeps
// splitting until every segment is one primitive - the same sweep, split key, tie rule and
// numbering - writes nbox of every node, and then plans the treelet's nodes bottom-up inside
// the workgroup (lbvh::planCosts): one thread per node, the costs and the done flags in LDS, a
// barrier between rounds, until the root is done. A node's flag is raised in the round after
// its costs were written, behind a barrier, so a parent never reads half a plan. Out: the
// packed picks of every node (picks, lbvh::kPlanDone set), the root's eight costs (pcost).
template <bool kPlan>
__global__ void __launch_bounds__(256) k_lbvh_treelet_sah(LbvhTreeletArgs a)
{
    constexpr uint32_t kLeafMost = kPlan ? 1u : static_cast<uint32_t>(kBvh8MaxLeafSize);
    __shared__ uint32_t sBox[6][256];          // by primitive (Morton position in the treelet): lo xyz, hi xyz, ordered
    __shared__ uint32_t sP[6][256], sS[6][256]; // a wave's prefix / suffix unions by position (hi complemented: all minima)
    __shared__ unsigned long long sBest[256];  // at a segment's first position
    __shared__ uint32_t sSrc[256];
    __shared__ uint32_t sWave[4];
    __shared__ uint16_t sCnt[256], sSplit[256];
    __shared__ uint8_t sOrd[3][256], sF[256], sL[256], sN[256], sSide[256];

    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const lbvh::Member T = a.list[blockIdx.x];
    const uint32_t first = T.r.first, n = lbvh::count(T.r);
    if (T.r.last < first || T.r.last >= a.prims || n > lbvh::kTreeletPrims || T.node < first || T.node > T.r.last) return; // (never: the list holds treelets only)
    uint32_t box[6] = { ~0u, ~0u, ~0u, 0u, 0u, 0u };
    if (t < n) {
        const uint32_t src = a.sorted[first + t];
        sSrc[t] = src;
        const float4* q = reinterpret_cast<const float4*>(a.snap + src);
        const float4 r0 = q[0], r1 = q[1], r2 = q[2];
        const float v0[3] = { r0.x, r0.y, r0.z }, e1[3] = { r0.w, r1.x, r1.y }, e2[3] = { r1.z, r1.w, r2.x };
        float v[3][3];
        if (a.light) {
            float unused;
            lbvh::lightVertices(v0, e1, e2, a.frame.m, v, unused);
        } else {
            for (int k = 0; k < 3; ++k) {
                v[0][k] = v0[k];
                v[1][k] = v0[k] + e1[k];
                v[2][k] = v0[k] + e2[k];
            }
        }
        lbvh::primBox(v, box);
    }
    for (int c = 0; c < 6; ++c) sBox[c][t] = box[c];
    // one segment, the treelet; the threads past it one segment each, never live
    sF[t] = static_cast<uint8_t>(t < n ? 0u : t);
    sL[t] = static_cast<uint8_t>(t < n ? n - 1u : t);
    sN[t] = static_cast<uint8_t>(t < n ? T.node - first : t);
    sSplit[t] = 0xffffu;
    sSide[t] = 0;
    if constexpr (kPlan) planLds().done[t] = 0;
    for (int ax = 0; ax < 3; ++ax) sP[ax][t] = lbvh::sweepKey(lbvh::orderedFloat(box[ax]), lbvh::orderedFloat(box[3 + ax]));
    __syncthreads();
    for (int ax = 0; ax < 3; ++ax) {
        uint32_t rank = t;
        if (t < n) {
            const uint32_t key = sP[ax][t];
            rank = 0;
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t kq = sP[ax][q];
                rank += (kq < key || (kq == key && q < t)) ? 1u : 0u;
            }
        }
        sOrd[ax][rank] = static_cast<uint8_t>(t);
    }
    __syncthreads();
    const uint32_t w0 = t & ~63u, w1 = w0 + 63u;
    for (;;) {
        const uint32_t f = sF[t], l = sL[t], cnt = l - f + 1u;
        const bool live = cnt > kLeafMost;
        if (!__syncthreads_or(live ? 1 : 0)) break;
        if (t == f) sBest[t] = lbvh::kNoSplit;
        unsigned long long mine = lbvh::kNoSplit;
        const uint32_t pLim = f > w0 ? f : w0, sLim = l < w1 ? l : w1;
        for (int ax = 0; ax < 3; ++ax) {
            const uint32_t prim = sOrd[ax][t];
            uint32_t P[6], S[6];
            for (int c = 0; c < 6; ++c) P[c] = S[c] = c < 3 ? sBox[c][prim] : ~sBox[c][prim];
            for (uint32_t j = 1; j < 64u; j <<= 1)
                for (int c = 0; c < 6; ++c) {
                    const uint32_t up = __shfl_up(P[c], j, 64), dn = __shfl_down(S[c], j, 64);
                    if (t >= pLim + j) P[c] = up < P[c] ? up : P[c];
                    if (t + j <= sLim) S[c] = dn < S[c] ? dn : S[c];
                }
            for (int c = 0; c < 6; ++c) {
                sP[c][t] = P[c];
                sS[c][t] = S[c];
            }
            __syncthreads();
            if (live) {
                // the union of [f, t]: this wave's part, the first wave's from f on, whole waves between
                if (f < w0) {
                    for (int c = 0; c < 6; ++c) {
                        const uint32_t o = sS[c][f];
                        P[c] = o < P[c] ? o : P[c];
                    }
                    for (uint32_t w = (f >> 6) + 1u; w < wave; ++w)
                        for (int c = 0; c < 6; ++c) {
                            const uint32_t o = sP[c][64u * w + 63u];
                            P[c] = o < P[c] ? o : P[c];
                        }
                }
                for (int c = 3; c < 6; ++c) P[c] = ~P[c];
                if (ax == 0 && t == l) {
                    float* nb = a.nbox + 6ull * (first + sN[t]);
                    for (int c = 0; c < 6; ++c) nb[c] = lbvh::orderedFloat(P[c]);
                    if constexpr (kPlan) {
                        PlanLds& pl = planLds();
                        pl.area[sN[t]] = lbvh::halfArea(P);
                        pl.first[sN[t]] = static_cast<uint8_t>(f);
                        pl.last[sN[t]] = static_cast<uint8_t>(l);
                    }
                }
                if (t < l) {
                    // the union of [t + 1, l] the same way
                    const uint32_t u = t + 1u, uw1 = (u & ~63u) + 63u;
                    uint32_t R[6];
                    for (int c = 0; c < 6; ++c) R[c] = sS[c][u];
                    if (l > uw1) {
                        for (int c = 0; c < 6; ++c) {
                            const uint32_t o = sP[c][l];
                            R[c] = o < R[c] ? o : R[c];
                        }
                        for (uint32_t w = (u >> 6) + 1u; w < (l >> 6); ++w)
                            for (int c = 0; c < 6; ++c) {
                                const uint32_t o = sP[c][64u * w + 63u];
                                R[c] = o < R[c] ? o : R[c];
                            }
                    }
                    for (int c = 3; c < 6; ++c) R[c] = ~R[c];
                    const unsigned long long key = lbvh::splitKey(lbvh::halfArea(P), lbvh::halfArea(R), t - f + 1u, cnt, static_cast<uint32_t>(ax));
                    mine = key < mine ? key : mine;
                }
            }
            __syncthreads(); // sP / sS are the next axis's
        }
        if (live && t < l) atomicMin(&sBest[f], mine);
        __syncthreads();
        uint32_t axis = 0, k = cnt;
        if (live) lbvh::chosenSplit(sBest[f], cnt, axis, k);
        sSide[sOrd[axis][t]] = t - f >= k ? 1 : 0;
        __syncthreads();
        for (int b = 0; b < 3; ++b) {
            const uint32_t prim = sOrd[b][t];
            const bool right = sSide[prim] != 0;
            const uint64_t lefts = __ballot(!right);
            if (lane == 0u) sWave[wave] = static_cast<uint32_t>(__popcll(lefts));
            __syncthreads();
            uint32_t c = static_cast<uint32_t>(__popcll(lefts & ((uint64_t(1) << lane) - 1u)));
            for (uint32_t w = 0; w < wave; ++w) c += sWave[w];
            sCnt[t] = static_cast<uint16_t>(c); // lefts before position t
            __syncthreads();
            const uint32_t leftBefore = c - sCnt[f];
            const uint32_t pos = right ? f + k + (t - f - leftBefore) : f + leftBefore;
            sOrd[b][pos] = static_cast<uint8_t>(prim);
            __syncthreads();
        }
        if (live) {
            if (t == f) sSplit[sN[t]] = static_cast<uint16_t>(f + k - 1u);
            if (t - f < k) {
                sL[t] = static_cast<uint8_t>(f + k - 1u);
                sN[t] = static_cast<uint8_t>(f + k - 1u);
            } else {
                sF[t] = static_cast<uint8_t>(f + k);
                sN[t] = static_cast<uint8_t>(f + k);
            }
        }
    }
    if (t < n) {
        const uint32_t prim = sOrd[0][t];
        a.sorted[first + t] = sSrc[prim];
        for (int c = 0; c < 6; ++c) a.pbox[6ull * (first + t) + c] = lbvh::orderedFloat(sBox[c][prim]);
        const uint32_t sp = sSplit[t];
        if (first + t != lbvh::treeletSpareIndex(T)) a.split[first + t] = first + (sp != 0xffffu ? sp : sF[t]);
    }
    if constexpr (kPlan) {
        // node t of the treelet (every index but the spare one): its range and split, relative
        PlanLds& pl = planLds();
        // (0 to do, 1 costs written, 2 flag raised; an index without a split - never: n - 1 nodes on n - 1 indices - is none)
        int state = t < n && first + t != lbvh::treeletSpareIndex(T) && sSplit[t] != 0xffffu ? 0 : 2;
        const uint32_t nf = pl.first[t], nl = pl.last[t], ns = sSplit[t];
        for (uint32_t round = 0; round <= n; ++round) { // (a tree of n - 1 nodes is done within n - 1 rounds)
            if (state == 1) {
                pl.done[t] = 1;
                state = 2;
            }
            if (!__syncthreads_or(state == 0 ? 1 : 0)) break;
            if (state != 0) continue;
            const bool leftSingle = ns == nf, rightSingle = ns + 1u == nl;
            if (!(leftSingle || pl.done[ns]) || !(rightSingle || pl.done[ns + 1u])) continue;
            float L[8], R[8], C[8];
            if (leftSingle) {
                uint32_t b[6];
                for (int c = 0; c < 6; ++c) b[c] = sBox[c][sOrd[0][nf]];
                lbvh::planLeafCosts(b, L);
            } else {
                for (int i = 0; i < 8; ++i) L[i] = pl.cost[i][ns];
            }
            if (rightSingle) {
                uint32_t b[6];
                for (int c = 0; c < 6; ++c) b[c] = sBox[c][sOrd[0][nl]];
                lbvh::planLeafCosts(b, R);
            } else {
                for (int i = 0; i < 8; ++i) R[i] = pl.cost[i][ns + 1u];
            }
            const uint32_t word = lbvh::planCosts(pl.area[t], nl - nf + 1u, L, R, C);
            for (int i = 0; i < 8; ++i) pl.cost[i][t] = C[i];
            a.picks[first + t] = word | lbvh::kPlanDone;
            if (first + t == T.node)
                for (int i = 0; i < 8; ++i) a.pcost[8ull * T.node + i] = C[i];
            state = 1;
        }
    }
}

// The collapse plan above the treelets: one workgroup per build, in rounds. In a round every
// thread strides over the list of the nodes of more than lbvh::kTreeletPrims primitives; a
// node that is not done and whose two children are - a treelet's root (planned by the kernel
// before), a single primitive outside every treelet (boxed here from its snapshot record, its
// pbox written for the collapse), or an upper node marked done in an earlier round - gets its
// box (nbox, the union of its children's ordered words), its costs (pcost) and its word
// (picks) with lbvh::kPlanComputed; behind a barrier the words computed in this round get
// lbvh::kPlanDone, and a second barrier ends the round. Nothing is read that this workgroup
// wrote in the same phase, no other workgroup exists, and the result does not depend on the
// schedule: unions of ordered words are exact in any order and a plan reads finished children
// only. The tree's height bounds the rounds by the list's length; a round that computes
// nothing while nodes are left sets counters[kLbvhPlanStalled] and ends the kernel.
__device__ __forceinline__ bool upperChild(const LbvhUpperArgs& a, const lbvh::Member& m, uint32_t b[6], float C[8])
{
    const uint32_t cnt = lbvh::count(m.r);
    if (cnt == 1u) {
        const uint32_t src = a.sorted[m.r.first];
        const float4* q = reinterpret_cast<const float4*>(a.snap + src);
        const float4 r0 = q[0], r1 = q[1], r2 = q[2];
        const float v0[3] = { r0.x, r0.y, r0.z }, e1[3] = { r0.w, r1.x, r1.y }, e2[3] = { r1.z, r1.w, r2.x };
        float v[3][3];
        if (a.light) {
            float unused;
            lbvh::lightVertices(v0, e1, e2, a.frame.m, v, unused);
        } else {
            for (int k = 0; k < 3; ++k) {
                v[0][k] = v0[k];
                v[1][k] = v0[k] + e1[k];
                v[2][k] = v0[k] + e2[k];
            }
        }
        lbvh::primBox(v, b);
        for (int c = 0; c < 6; ++c) a.pbox[6ull * m.r.first + c] = lbvh::orderedFloat(b[c]);
        lbvh::planLeafCosts(b, C);
        return true;
    }
    if (cnt > lbvh::kTreeletPrims && !(a.picks[m.node] & lbvh::kPlanDone)) return false;
    for (int c = 0; c < 6; ++c) b[c] = lbvh::ordered(a.nbox[6ull * m.node + c]);
    for (int i = 0; i < 8; ++i) C[i] = a.pcost[8ull * m.node + i];
    return true;
}

__global__ void __launch_bounds__(1024) k_lbvh_upper_plan(LbvhUpperArgs a)
{
    for (uint32_t round = 0; round < a.count; ++round) {
        int left = 0, computed = 0;
        for (uint32_t j = threadIdx.x; j < a.count; j += 1024u) {
            const lbvh::Member m = a.list[j];
            // (never: the list holds nodes of this build's ranges only)
            if (m.r.last >= a.prims || m.r.first > m.r.last || m.node < m.r.first || m.node > m.r.last) continue;
            if (a.picks[m.node] & lbvh::kPlanDone) continue;
            left = 1;
            lbvh::Member l, r;
            lbvh::childrenOf(a.split, m, l, r);
            if (l.r.last < m.r.first || l.r.last >= m.r.last) continue; // (never: a split inside the range)
            uint32_t lb[6], rb[6], box[6];
            float L[8], R[8], C[8];
            if (!upperChild(a, l, lb, L) || !upperChild(a, r, rb, R)) continue;
            const uint32_t word = lbvh::planUpperNode(lb, L, rb, R, lbvh::count(m.r), box, C);
            for (int c = 0; c < 6; ++c) a.nbox[6ull * m.node + c] = lbvh::orderedFloat(box[c]);
            for (int i = 0; i < 8; ++i) a.pcost[8ull * m.node + i] = C[i];
            a.picks[m.node] = word | lbvh::kPlanComputed;
            computed = 1;
        }
        const int anyLeft = __syncthreads_or(left);
        const int anyComputed = __syncthreads_or(computed);
        if (!anyLeft) return;
        if (!anyComputed) {
            if (threadIdx.x == 0u) atomicOr(&a.counters[kLbvhPlanStalled], 1u);
            return;
        }
        // this round's words become final: from the next round on their nodes count as done
        for (uint32_t j = threadIdx.x; j < a.count; j += 1024u) {
            const lbvh::Member m = a.list[j];
            if (m.node >= a.prims) continue;
            const uint32_t word = a.picks[m.node];
            if ((word & lbvh::kPlanComputed) && !(word & lbvh::kPlanDone)) a.picks[m.node] = word | lbvh::kPlanDone;
        }
        __syncthreads();
    }
}

template <bool kPlan>
__global__ void __launch_bounds__(128) k_lbvh_collapse(LbvhCollapseArgs a, const uint32_t* __restrict__ picks)
{
    const uint32_t i = blockIdx.x * 128u + threadIdx.x;
    if (i >= a.count) return;
    const lbvh::Member top = a.items ? a.items[i] : a.root;
    lbvh::WideNode w;
    const lbvh::KeyLayout layout = { a.wBits };
    lbvh::planNode(a.keys, a.split, top, a.criterion, a.extent, w, a.slotRule, layout, a.useSah ? &a.sah : nullptr, kPlan ? picks : nullptr);
    uint32_t slot0 = 0;
    if (w.internal) {
        slot0 = atomicAdd(&a.counters[kLbvhNextCount], w.internal);
        if (slot0 + w.internal > a.nextCapacity) {
            // more nodes than the scratch holds: nothing written past it, the job falls back
            atomicOr(&a.counters[kLbvhOverflow], 1u);
            return;
        }
    }
    const uint32_t triBase = w.rows.span ? atomicAdd(&a.counters[kLbvhRecords], w.rows.span) : 0u;
    GpuBvh8Node nd;
    uint4* words = reinterpret_cast<uint4*>(&nd);
    for (int k = 0; k < 5; ++k) words[k] = make_uint4(0u, 0u, 0u, 0u);
    nd.imask = static_cast<uint8_t>(w.imask);
    nd.child_base = a.nextBase + slot0;
    nd.tri_base = triBase;
    nd.leaf_tris = w.rows.leaf_tris;
    nd.tri_stride = static_cast<uint8_t>(w.rows.stride);
    nd.leaf_mask = static_cast<uint8_t>(w.rows.leaf_mask);
    uint4* dst = reinterpret_cast<uint4*>(a.nodes + a.levelBase + i);
    for (int k = 0; k < 5; ++k) dst[k] = words[k];
    // children in slot order: internal ones consecutive from child_base
    uint32_t nInternal = 0;
    for (uint32_t s = 0; s < 8u; ++s) {
        const int k = lbvh::memberInSlot(w, s);
        if (k < 0) continue;
        const lbvh::Member& m = w.member[k];
        if ((w.imask >> s) & 1u) {
            a.next[slot0 + nInternal++] = m;
        } else {
            for (uint32_t t = 0; t < lbvh::count(m.r); ++t) a.position[m.r.first + t] = triBase + s + w.rows.stride * t;
        }
    }
}

__global__ void __launch_bounds__(256) k_lbvh_fill(float4* __restrict__ tris, uint32_t* __restrict__ perm, uint32_t records)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > records) return; // records + 1 entries: the padding record last, all zero
    float4* q = tris + 3ull * r;
    q[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    q[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    q[2] = make_float4(0.0f, r < records ? __uint_as_float(kHoleInstance) : 0.0f, 0.0f, 0.0f);
    if (r < records && perm) perm[r] = 0xffffffffu; // (the sun's BVH needs no perm)
}

__global__ void __launch_bounds__(256) k_lbvh_scatter(const float4* __restrict__ snap, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ position,
                                                      float4* __restrict__ tris, uint32_t* __restrict__ perm, uint32_t prims, uint32_t records)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= prims) return;
    const uint32_t src = sorted[j], pos = position[j];
    if (pos >= records) return; // (never: positions come from the record counter)
    const float4* q = snap + 3ull * src;
    float4* d = tris + 3ull * pos;
    d[0] = q[0];
    d[1] = q[1];
    d[2] = q[2];
    if (perm) perm[pos] = src;
}

} // namespace dev

hipError_t launch_lbvh_prims(const GpuTriangle* snap, uint32_t records, const uint32_t* classOf, uint32_t instances, uint32_t* idx, uint64_t* keys,
                             LbvhHeader* hdr, hipStream_t s)
{
    // counts and flags 0, the box empty (lo the largest, hi the smallest ordered value)
    hipError_t e = hipMemsetAsync(hdr, 0, sizeof(LbvhHeader), s);
    if (e == hipSuccess) e = hipMemsetAsync(hdr->lo, 0xff, sizeof(hdr->lo), s);
    if (e != hipSuccess || records == 0) return e;
    const dim3 grid((records + 255u) / 256u);
    hipLaunchKernelGGL(dev::k_lbvh_prims, grid, dim3(256), 0, s, snap, records, classOf, instances, idx, hdr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dev::k_lbvh_keys, grid, dim3(256), 0, s, snap, idx, classOf, hdr, keys);
    return hipGetLastError();
}

hipError_t launch_lbvh_prims_light(const GpuTriangle* snap, uint32_t records, uint32_t instances, const LbvhFrame& frame, int wBits, uint32_t* idx, uint64_t* keys,
                                   LbvhHeader* hdr, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(hdr, 0, sizeof(LbvhHeader), s);
    if (e == hipSuccess) e = hipMemsetAsync(hdr->lo, 0xff, sizeof(hdr->lo), s);
    if (e != hipSuccess || records == 0) return e;
    const dim3 grid((records + 255u) / 256u);
    hipLaunchKernelGGL(dev::k_lbvh_prims_light, grid, dim3(256), 0, s, snap, records, instances, frame, idx, hdr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dev::k_lbvh_keys_light, grid, dim3(256), 0, s, snap, idx, hdr, frame, wBits, keys);
    return hipGetLastError();
}

hipError_t launch_lbvh_sort(void* temp, size_t& tempBytes, const uint64_t* keysIn, uint64_t* keysOut, const uint32_t* valuesIn, uint32_t* valuesOut, uint32_t count,
                            hipStream_t s)
{
    return rocprim::radix_sort_pairs(temp, tempBytes, keysIn, keysOut, valuesIn, valuesOut, count, 0u, static_cast<unsigned int>(lbvh::kKeyBits), s);
}

hipError_t launch_lbvh_hierarchy(const uint64_t* keys, uint32_t lo, uint32_t hi, uint32_t* split, hipStream_t s, lbvh::Member* treelets, uint32_t treeletCapacity,
                                 uint32_t* counters, lbvh::Member* upper, uint32_t upperCapacity)
{
    if (hi - lo < 2u) return hipSuccess;
    const dim3 grid((hi - lo - 1u + 255u) / 256u);
    if (treelets && upper)
        hipLaunchKernelGGL(dev::k_lbvh_hierarchy<true>, grid, dim3(256), 0, s, keys, lo, hi, split, treelets, treeletCapacity, counters, upper, upperCapacity);
    else
        hipLaunchKernelGGL(dev::k_lbvh_hierarchy<false>, grid, dim3(256), 0, s, keys, lo, hi, split, treelets, treeletCapacity, counters, nullptr, 0u);
    return hipGetLastError();
}

hipError_t launch_lbvh_treelet_sah(const LbvhTreeletArgs& a, uint32_t treelets, hipStream_t s, bool plan)
{
    if (treelets == 0) return hipSuccess;
    if (plan && (!a.picks || !a.pcost)) return hipErrorInvalidValue;
    if (plan)
        hipLaunchKernelGGL(dev::k_lbvh_treelet_sah<true>, dim3(treelets), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(dev::k_lbvh_treelet_sah<false>, dim3(treelets), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lbvh_upper_plan(const LbvhUpperArgs& a, hipStream_t s)
{
    if (a.count == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_lbvh_upper_plan, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lbvh_collapse(const LbvhCollapseArgs& a, hipStream_t s, const uint32_t* picks)
{
    if (a.count == 0) return hipSuccess;
    const dim3 grid((a.count + 127u) / 128u);
    if (picks)
        hipLaunchKernelGGL(dev::k_lbvh_collapse<true>, grid, dim3(128), 0, s, a, picks);
    else
        hipLaunchKernelGGL(dev::k_lbvh_collapse<false>, grid, dim3(128), 0, s, a, picks);
    return hipGetLastError();
}

hipError_t launch_lbvh_scatter(const GpuTriangle* snap, const uint32_t* sorted, const uint32_t* position, GpuTriangle* tris, uint32_t* perm, uint32_t prims,
                               uint32_t records, hipStream_t s)
{
    hipLaunchKernelGGL(dev::k_lbvh_fill, dim3(records / 256u + 1u), dim3(256), 0, s, reinterpret_cast<float4*>(tris), perm, records);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || prims == 0) return e;
    hipLaunchKernelGGL(dev::k_lbvh_scatter, dim3((prims + 255u) / 256u), dim3(256), 0, s, reinterpret_cast<const float4*>(snap), sorted, position,
                       reinterpret_cast<float4*>(tris), perm, prims, records);
    return hipGetLastError();
}

} // namespace ark
