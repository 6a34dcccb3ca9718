// ddgi_traversal.h — the software BVH8 traversal core of the device code: the per-lane
// stack, the node and triangle steps (world space and the sun's light space) and the
// XCD-aware work distribution. Nothing here is a kernel: the persistent kernel templates
// are ddgi_trace_kernels.h's, the AO bake (ddgi_bake.hip) steps with travFetch /
// travCompute directly. A consumer adds a ray source or a shadow mode by instantiating
// those templates in its own unit, not by editing this file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddgi_device.h"
#include "ddgi_kernels.h"

namespace ark {

__device__ __forceinline__ float4 SceneArgs::sample(int idx, float u, float v) const
{
    return dev::sampleOrWhite(tex_infos, texels, texture_count, white_texture, idx, u, v);
}

namespace dev {

// ---------------------------------------------------------------------------
// 1. BVH traversal
// ---------------------------------------------------------------------------
// Per-lane traversal stack of node groups {child_base, hits | imask << 8}: the top
// kStackLds entries live in an LDS ring (slot-major, so the 64 lanes of a wave hit
// distinct banks), deeper entries spill to a per-lane HBM area
// [entry][word][lane] that only deep descents touch.
template<int BLOCK>
struct Stack {
    uint32_t* lds;
    uint32_t* spill;
    uint32_t spillStride;
    int depth;
    __device__ __forceinline__ void push(uint32_t a, uint32_t b)
    {
        const int slot = depth & (kStackLds - 1);
        uint32_t* l = lds + slot * 2 * BLOCK;
        if (depth >= kStackLds) {
            uint32_t* sp = spill + static_cast<size_t>(depth - kStackLds) * 2 * spillStride;
            sp[0] = l[0];
            sp[spillStride] = l[BLOCK];
        }
        l[0] = a;
        l[BLOCK] = b;
        depth++;
    }
    __device__ __forceinline__ void pop(uint32_t& a, uint32_t& b)
    {
        depth--;
        const int slot = depth & (kStackLds - 1);
        uint32_t* l = lds + slot * 2 * BLOCK;
        a = l[0];
        b = l[BLOCK];
        if (depth >= kStackLds) {
            const uint32_t* sp = spill + static_cast<size_t>(depth - kStackLds) * 2 * spillStride;
            l[0] = sp[0];
            l[BLOCK] = sp[spillStride];
        }
    }
};

struct RayHit {
    float t;      // best t so far (tmax of the query)
    float u, v;
    uint32_t tri; // leaf-order triangle index, kNoHit = none
    uint32_t inst, prim;
    bool backface;
};

// Inverse ray direction for the box tests only (triangle tests use d): v_rcp_f32
// (1 ulp) instead of an IEEE divide (~10 VALU each). Every slab distance of an axis
// then carries the same relative factor 1 +- 6e-8, far inside the box test's 1e-5
// relative margin (visitNode8), so culling stays conservative; the sign, and with
// it the ray octant, is exact.
__device__ __forceinline__ V3 safeInv(V3 d)
{
    auto f = [](float x) { return __builtin_amdgcn_rcpf(fabsf_(x) < 1e-20f ? (x < 0.0f ? -1e-20f : 1e-20f) : x); };
    return { f(d.x), f(d.y), f(d.z) };
}

// crossFma, dotFma3 and intersectTri (Möller–Trumbore) are shading_math.h's: the host restatements call the same function.

__device__ __forceinline__ GpuTriangle loadTri(const GpuTriangle* __restrict__ tris, uint32_t i)
{
    const float4* p = reinterpret_cast<const float4*>(tris + i);
    float4 a = p[0], b = p[1], c = p[2];
    GpuTriangle t;
    t.t0[0] = a.x; t.t0[1] = a.y; t.t0[2] = a.z; t.t0[3] = a.w;
    t.t1[0] = b.x; t.t1[1] = b.y; t.t1[2] = b.z; t.t1[3] = b.w;
    t.t2[0] = c.x; t.t2[1] = c.y; t.t2[2] = c.z; t.t2[3] = c.w;
    return t;
}

// masked.rahit:16-37 — any-hit alpha test of a masked candidate.
static __device__ bool alphaAccept(const SceneArgs& sc, uint32_t inst, uint32_t prim, float u, float v)
{
    const GpuInstance& gi = sc.instances[inst];
    const ArkRTTriangleMesh mesh = sc.meshes[gi.rt_mesh_index];
    const ArkShaderMaterial& mat = sc.materials[mesh.material_index];
    float bx = 1.0f - u - v, by = u, bz = v;
    float uv[2][3];
    for (int k = 0; k < 3; ++k) {
        uint32_t idx = sc.indices[static_cast<size_t>(mesh.first_index) + 3u * prim + k];
        const float* vx = sc.vertices + (static_cast<size_t>(mesh.first_vertex) + idx) * 9;
        uv[0][k] = vx[0];
        uv[1][k] = vx[1];
    }
    float uvx = uv[0][0] * bx + uv[0][1] * by + uv[0][2] * bz;
    float uvy = uv[1][0] * bx + uv[1][1] * by + uv[1][2] * bz;
    float4 c = sc.sample(mat.base_color, uvx, uvy);
    return !(c.w < mat.mask_cutoff);
}

// anyhit.rahit of the path tracer: only BLEND_MODE_MASKED materials are tested. Declared here for
// travStepDual<.., PATH = true>; the unit that instantiates the path source (ddgi_path_tracer.hip)
// defines it, no other unit's kernels refer to it.
__device__ bool alphaAcceptPath(const SceneArgs& sc, uint32_t inst, uint32_t prim, float u, float v);

// Ray octant (bit a: idir[a] < 0); slots are visited in increasing (slot ^ oct).
__device__ __forceinline__ uint32_t rayOctant(V3 idir)
{
    return (idir.x < 0.0f ? 1u : 0u) | (idir.y < 0.0f ? 2u : 0u) | (idir.z < 0.0f ? 4u : 0u);
}

// Node group holding only the root: one hit child (k = 0) of a virtual parent with no
// internal-children mask, so nextChild returns the group base (the root) whatever the
// ray octant - a fresh lane can fetch the root before its ray direction is known.
__device__ __forceinline__ uint32_t rootGroupBits() { return 1u; }

// Next child of a non-empty node group; removes it from the group. Group bits:
// 0-7 hit internal children in visiting order (k = slot ^ oct), 8-15 imask (slot
// order). (An "origin inside" set that went first was measured and removed in round 3;
// its bits 16-23 stayed zero and their test ran in every node step until round 5.)
__device__ __forceinline__ uint32_t nextChild(uint32_t base, uint32_t& bits, uint32_t oct)
{
    const uint32_t k = static_cast<uint32_t>(__builtin_ctz(bits & 0xffu));
    const uint32_t slot = k ^ oct;
    bits &= ~(1u << k);
    return base + static_cast<uint32_t>(__builtin_popcount((bits >> 8) & ((1u << slot) - 1u)));
}

// Tests the 8 children of one BVH8 node against [tmin, tmax]. A slab distance is
// one fma of the 8-bit plane index q:  t = q * (step * idir) + (p - o) * idir,
// where step * idir is exact (a power of two) and (p - o) * idir carries at most
// about 2 ulp of |p - o| * |idir| (idir itself within 1 ulp of 1/d, safeInv); the
// build inflates every box by 1e-6 of the
// scene diagonal on top of its own relative margin (bvh_builder.cpp inflateChildBox), which
// covers that error, and the comparison keeps a relative margin for far boxes,
// so a box holding an exact triangle hit is never culled. The near/far plane of
// each axis is chosen by the ray octant. Scalar fp32, one slot at a time: a packed
// v_pk_fma_f32 pair issues in two slots on gfx950 and needs moves to pair its
// operands (measured 3.02 vs 2.72 ms traversal at C4 in round 1).
// Returns the hit internal children as a node group and the hit leaf children's
// triangles as a bit mask over [tBase, tBase + 24) (2 VALU: triangle rows).
// Node-visit instruction budget (tools/isa_budget.py). Dual steps of
// k_trace (travStepDual<.., GF = true>) fetch every node from global memory, with both
// sides' loads outside any branch (see travStepDual): its LDS node cache is then not
// allocated (22.3 -> 18.4 KB of LDS per workgroup); C4 step 3.66 / 3.68 -> 3.57 / 3.54
// ms, K = 4096 windows 0.606 -> 0.591 / 0.585 ms, Z-slab proxy P = 8 0.578 -> 0.570 ms
// (profiles/r03_an, r03_ao). k_trace_shadow keeps its top nodes in LDS (GF = false):
// its any-hit rays gain from them (0.704 -> 0.730 ms with global fetches).
constexpr int kShadowLdsNodes = kLdsNodes - 8; // top nodes k_trace_shadow keeps in LDS
// LDS octant permutation table of the node visit (loadNodeCache fills it; every
// kernel that visits nodes calls loadNodeCache first)
static __shared__ uint8_t g_octPerm[8 * 256];

// Rejected node-test forms (measured slower, removed in round 5): packed
// fp16 child tests with error bounds or directed rounding (C4 traversal 1.95 -> 20-30
// ms from near-axis-parallel rays), origin-containing children first (+40 VALU per node
// for 0.8 % fewer visits), v_cndmask plane selects and v_max/v_min interval tests.
__device__ __forceinline__ void visitNode8(uint4 w0, uint4 w1, uint4 w2, uint4 w3, uint4 w4, V3 o, V3 idir, uint32_t oct, float tmin,
                                           float tmax, uint32_t& gBase, uint32_t& gBits, uint32_t& tBase, uint32_t& tBits)
{
    // exponent byte e: the step is 2^(e - 127) (e = 0 never occurs for a used axis:
    // the builder's steps are normal numbers); step * idir as one v_ldexp_f32
    const float ax = __builtin_amdgcn_ldexpf(idir.x, static_cast<int>(w0.w & 0xffu) - 127);
    const float ay = __builtin_amdgcn_ldexpf(idir.y, static_cast<int>((w0.w >> 8) & 0xffu) - 127);
    const float az = __builtin_amdgcn_ldexpf(idir.z, static_cast<int>((w0.w >> 16) & 0xffu) - 127);
    const float bx = (__uint_as_float(w0.x) - o.x) * idir.x;
    const float by = (__uint_as_float(w0.y) - o.y) * idir.y;
    const float bz = (__uint_as_float(w0.z) - o.z) * idir.z;
    const uint32_t imask = w0.w >> 24;
    // gfx950 issues v_bitop3_b32 and v_ashrrev_i32 in about half the cycles of a
    // v_cndmask_b32 (tools/probe/valu_table*.hip): the near/far plane words of each axis
    // are selected bitwise under the lane mask of its direction sign (all ones when the
    // component is negative - the octant bit; idir is never -0, safeInv)
    auto signMask = [](float v) { return static_cast<uint32_t>(static_cast<int32_t>(__float_as_uint(v)) >> 31); };
    auto pick = [](uint32_t m, uint32_t a, uint32_t b) {
        uint32_t r;
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xca" : "=v"(r) : "v"(m), "v"(a), "v"(b)); // m ? a : b, bitwise
        return r;
    };
    const uint32_t mx = signMask(idir.x), my = signMask(idir.y), mz = signMask(idir.z);
    const uint32_t nX0 = pick(mx, w3.z, w2.x), nX1 = pick(mx, w3.w, w2.y), fX0 = pick(mx, w2.x, w3.z), fX1 = pick(mx, w2.y, w3.w);
    const uint32_t nY0 = pick(my, w4.x, w2.z), nY1 = pick(my, w4.y, w2.w), fY0 = pick(my, w2.z, w4.x), fY1 = pick(my, w2.w, w4.y);
    const uint32_t nZ0 = pick(mz, w4.z, w3.x), nZ1 = pick(mz, w4.w, w3.y), fZ0 = pick(mz, w3.x, w4.z), fZ1 = pick(mz, w3.y, w4.w);
    // max(tn, tmin) <= f(min(tf, tmax)) with the monotone f(x) = fma(x, 1.00001, 1e-7) is
    // tn <= f(tf) && tn <= f(tmax) && tmin <= f(tf) (tmin <= f(tmax) holds for any ray
    // the traversal runs): the same accepted set as the max/min form (no NaN reaches
    // it: A, B and q are finite), three 2-cycle compares instead of two 4-cycle v_max /
    // v_min (tmin is an SGPR operand: every caller passes a wave-uniform constant)
    const float limT = fmaf(tmax, 1.00001f, 1e-7f);
    uint32_t hitSlots = 0;
    // slots 7 .. 0, each compare shifted into the mask as v_addc's carry (m = 2m + hit)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = 7 - k;
        const uint32_t sh = static_cast<uint32_t>(s & 3) * 8u;
        const bool hiWord = s >= 4;
        auto q = [&](uint32_t w0_, uint32_t w1_) { return static_cast<float>(((hiWord ? w1_ : w0_) >> sh) & 0xffu); };
        const float tnx = fmaf(q(nX0, nX1), ax, bx), tny = fmaf(q(nY0, nY1), ay, by), tnz = fmaf(q(nZ0, nZ1), az, bz);
        const float tfx = fmaf(q(fX0, fX1), ax, bx), tfy = fmaf(q(fY0, fY1), ay, by), tfz = fmaf(q(fZ0, fZ1), az, bz);
        const float tn = fmaxf(fmaxf(tnx, tny), tnz);
        const float lim = fmaf(fminf(fminf(tfx, tfy), tfz), 1.00001f, 1e-7f);
        uint64_t c0, c1;
        asm("v_cmp_le_f32_e64 %[c0], %[tn], %[lim]\n\t"
            "v_cmp_le_f32_e64 %[c1], %[tn], %[lt]\n\t"
            "s_and_b64 %[c0], %[c0], %[c1]\n\t"
            "v_cmp_le_f32_e64 %[c1], %[tmin], %[lim]\n\t"
            "s_and_b64 vcc, %[c0], %[c1]\n\t"
            "v_addc_co_u32_e32 %[acc], vcc, %[acc], %[acc], vcc"
            : [acc] "+v"(hitSlots), [c0] "=&s"(c0), [c1] "=&s"(c1)
            : [tn] "v"(tn), [lim] "v"(lim), [lt] "v"(limT), [tmin] "s"(tmin)
            : "vcc");
    }
    // internal children: slot bits -> visiting order bits (k = slot ^ oct), one LDS byte
    // (g_octPerm, filled by loadNodeCache) instead of three conditional swap stages
    const uint32_t m = g_octPerm[(oct << 8) | (hitSlots & imask & 0xffu)];
    // leaf children: their triangle rows (GpuBvh8Node: bit s + stride i = triangle
    // i of leaf slot s), the hit leaf slots spread over the three rows and masked
    gBase = w1.x;
    gBits = m | (imask << 8);
    tBase = w1.y;
    const uint32_t stride = w1.w & 31u, leafHits = hitSlots & (w1.w >> 8) & 0xffu;
    const uint32_t x = (leafHits << stride) | leafHits;
    tBits = ((x << stride) | x) & w1.z;
}

__device__ __forceinline__ GpuTriangle triFromWords(uint4 a, uint4 b, uint4 c)
{
    GpuTriangle t;
    t.t0[0] = __uint_as_float(a.x); t.t0[1] = __uint_as_float(a.y); t.t0[2] = __uint_as_float(a.z); t.t0[3] = __uint_as_float(a.w);
    t.t1[0] = __uint_as_float(b.x); t.t1[1] = __uint_as_float(b.y); t.t1[2] = __uint_as_float(b.z); t.t1[3] = __uint_as_float(b.w);
    t.t2[0] = __uint_as_float(c.x); t.t2[1] = __uint_as_float(c.y); t.t2[2] = __uint_as_float(c.z); t.t2[3] = __uint_as_float(c.w);
    return t;
}

// One traversal step of one lane: a pending triangle of the current leaf group is
// tested, otherwise the next child of the current node group is visited (popping
// a group when it is empty). Triangles and nodes are fetched by the same five
// 16-B loads, so a wave whose lanes mix both kinds of step waits for memory
// once per step instead of once per node plus once per triangle.
struct TravState {
    uint32_t gBase, gBits; // node group: hits (k-space) | imask << 8
    uint32_t tBase, tBits; // triangle group
};

template<int BLOCK>
__device__ __forceinline__ bool travDone(const TravState& ts, const Stack<BLOCK>& st)
{
    return ts.tBits == 0 && (ts.gBits & 0xffu) == 0 && st.depth == 0;
}

// A traversal step is split in two so that the fetch can be issued before a
// freshly refilled lane has its ray set up: travFetch picks the work item (a
// pending leaf triangle, else the next child of the current node group, popping
// a group when it is empty) and issues its five 16-B loads; travCompute tests it.
struct Fetch {
    uint4 w0, w1, w2, w3, w4;
    uint32_t i; // triangle index (triangle steps)
    bool isTri;
};

// The first kLdsNodes nodes of the opaque BVH (its top levels: nodes are laid out
// breadth first) copied into LDS once per workgroup: every ray starts there, so
// those fetches skip the vector-memory path.
struct NodeCache {
    const uint4* lds; // [count][5]
    uint32_t base;    // node index of lds[0]
    uint32_t count;
};

template<int BLOCK, int NODES = kLdsNodes>
__device__ __forceinline__ NodeCache loadNodeCache(const SceneArgs& sc, uint4* lds)
{
    NodeCache nc { lds, sc.root_opaque >= 0 ? static_cast<uint32_t>(sc.root_opaque) : 0u, 0u };
    if (sc.root_opaque >= 0) {
        nc.count = min(static_cast<uint32_t>(NODES), sc.opaque_nodes);
        const uint4* src = reinterpret_cast<const uint4*>(sc.nodes + nc.base);
        for (uint32_t i = threadIdx.x; i < nc.count * 5u; i += BLOCK) lds[i] = src[i];
    }
    // octant permutation table of visitNode8: entry (oct << 8 | m) has bit k set iff
    // bit k ^ oct of m is set
    for (uint32_t i = threadIdx.x; i < 8u * 256u; i += BLOCK) {
        const uint32_t oct = i >> 8, m = i & 0xffu;
        uint32_t r = 0;
        for (uint32_t k = 0; k < 8u; ++k) r |= ((m >> (k ^ oct)) & 1u) << k;
        g_octPerm[i] = static_cast<uint8_t>(r);
    }
    __syncthreads();
    return nc;
}

template<int BLOCK>
__device__ __forceinline__ void travFetch(const SceneArgs& sc, const NodeCache& nc, TravState& ts, Stack<BLOCK>& st, uint32_t oct, Fetch& fx)
{
    fx.isTri = ts.tBits != 0;
    const uint4* src;
    if (fx.isTri) {
        fx.i = ts.tBase + static_cast<uint32_t>(__builtin_ctz(ts.tBits));
        ts.tBits &= ts.tBits - 1u;
        src = reinterpret_cast<const uint4*>(sc.tris + fx.i);
    } else {
        if ((ts.gBits & 0xffu) == 0) st.pop(ts.gBase, ts.gBits);
        const uint32_t child = nextChild(ts.gBase, ts.gBits, oct);
        if (ts.gBits & 0xffu) st.push(ts.gBase, ts.gBits);
        src = reinterpret_cast<const uint4*>(sc.nodes + child);
    }
    const uint32_t rel = static_cast<uint32_t>(reinterpret_cast<const GpuBvh8Node*>(src) - sc.nodes) - nc.base;
    if (!fx.isTri && rel < nc.count) {
        const uint4* l = nc.lds + rel * 5u;
        fx.w0 = l[0];
        fx.w1 = l[1];
        fx.w2 = l[2];
        fx.w3 = l[3];
        fx.w4 = l[4];
        return;
    }
    fx.w0 = src[0];
    fx.w1 = src[1];
    fx.w2 = src[2];
    // five loads whatever the step: a triangle step reads 32 B of the next record
    // (the triangle array is padded), no branch around the node's last two loads
    fx.w3 = src[3];
    fx.w4 = src[4];
}

// Returns true when a triangle step produced a candidate (tt, uu, vv, backface
// with the instance's handedness applied, inst, prim) in [tmin, tmax]; node steps
// update the group state and return false.
__device__ __forceinline__ bool travCompute(const Fetch& fx, TravState& ts, V3 o, V3 d, V3 idir, uint32_t oct, float tmin, float tmax, float& tt,
                                            float& uu, float& vv, bool& backface, uint32_t& inst, uint32_t& prim, uint32_t& cNodes, uint32_t& cTris)
{
    if (fx.isTri) {
        cTris++;
        const GpuTriangle tr = triFromWords(fx.w0, fx.w1, fx.w2);
        bool bf;
        if (!intersectTri(o, d, tmin, tmax, tr, &tt, &uu, &vv, &bf)) return false;
        inst = fx.w2.y;
        prim = fx.w2.z;
        backface = bf != (fx.w2.w != 0u); // GpuTriangle t2.w: instance flips facing
        return true;
    }
    cNodes++;
    visitNode8(fx.w0, fx.w1, fx.w2, fx.w3, fx.w4, o, idir, oct, tmin, tmax, ts.gBase, ts.gBits, ts.tBase, ts.tBits);
    return false;
}

// Dual step (k_trace): one lane tests a pending leaf triangle AND visits the next
// node in the same iteration. A divergent wave runs the node and the triangle code
// every iteration anyway (28 % of the steps are triangle steps, spread over its
// lanes), so letting each lane do both roughly turns nodes + triangles iterations
// per ray into max(nodes, triangles) + a short tail. Leaf hits of a node visited
// while the lane's triangle group is still pending wait in a second group (nBase,
// nBits); the node side pauses while that one is full. The closest hit does not
// depend on the order (equal t: smaller (instance, primitive) wins). ANY (shadow
// rays): the step reports a triangle hit in [tmin, h.t] instead of recording it.
template<int BLOCK>
__device__ __forceinline__ bool travDoneDual(const TravState& ts, uint32_t nBits, const Stack<BLOCK>& st)
{
    return ts.tBits == 0 && nBits == 0 && (ts.gBits & 0xffu) == 0 && st.depth == 0;
}

template<int BLOCK, bool ANY, bool GF = false, bool PATH = false>
__device__ __forceinline__ bool travStepDual(const SceneArgs& sc, const NodeCache& nc, TravState& ts, uint32_t& nBase, uint32_t& nBits, Stack<BLOCK>& st,
                                             V3 o, V3 d, V3 idir, uint32_t oct, float tmin, RayHit& h, int pass, uint32_t& cNodes, uint32_t& cTris)
{
    bool anyHit = false;
    const bool doTri = ts.tBits != 0;
    const bool doNode = nBits == 0 && ((ts.gBits & 0xffu) != 0 || st.depth != 0);
    // fetch registers are left undefined on lanes that skip a side: zero-filling
    // them cost ~34 VALU per iteration (the compiler materialised the zeros)
    uint4 a, b, c;
    uint32_t ti = 0;
    uint4 w0, w1, w2, w3, w4;
    if constexpr (GF) {
    // Both sides' loads are issued by every lane outside any branch (a skipped side
    // reads a resident dummy record: triangle 0, the root node), triangle loads first:
    // the wait before the triangle test then covers only the triangle loads, and the
    // test runs while the node loads are in flight (the branch-local loads of the
    // other form make the compiler wait for both: vmcnt(0)). Nodes come from global
    // memory only (the LDS node cache would make these generic flat loads).
    (void)nc;
    if (doTri) {
        ti = ts.tBase + static_cast<uint32_t>(__builtin_ctz(ts.tBits));
        ts.tBits &= ts.tBits - 1u;
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(sc.tris + ti);
        a = src[0];
        b = src[1];
        c = src[2];
    }
    uint32_t child = static_cast<uint32_t>(sc.root_opaque >= 0 ? sc.root_opaque : 0);
    if (doNode) {
        if ((ts.gBits & 0xffu) == 0) st.pop(ts.gBase, ts.gBits);
        child = nextChild(ts.gBase, ts.gBits, oct);
        if (ts.gBits & 0xffu) st.push(ts.gBase, ts.gBits);
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(sc.nodes + child);
        w0 = src[0];
        w1 = src[1];
        w2 = src[2];
        w3 = src[3];
        w4 = src[4];
    }
    } else {
    if (doTri) {
        ti = ts.tBase + static_cast<uint32_t>(__builtin_ctz(ts.tBits));
        ts.tBits &= ts.tBits - 1u;
        const uint4* src = reinterpret_cast<const uint4*>(sc.tris + ti);
        a = src[0];
        b = src[1];
        c = src[2];
    }
    if (doNode) {
        if ((ts.gBits & 0xffu) == 0) st.pop(ts.gBase, ts.gBits);
        const uint32_t child = nextChild(ts.gBase, ts.gBits, oct);
        if (ts.gBits & 0xffu) st.push(ts.gBase, ts.gBits);
        const uint32_t rel = child - nc.base;
        const uint4* src = rel < nc.count ? nc.lds + rel * 5u : reinterpret_cast<const uint4*>(sc.nodes + child);
        w0 = src[0];
        w1 = src[1];
        w2 = src[2];
        w3 = src[3];
        w4 = src[4];
    }
    }
    if (doTri) {
        cTris++;
        const GpuTriangle tr = triFromWords(a, b, c);
        bool bf;
        float tt, uu, vv;
        if (intersectTri(o, d, tmin, h.t, tr, &tt, &uu, &vv, &bf)) {
            const uint32_t inst = c.y, prim = c.z;
            if (ANY) anyHit = true;
            else if (!(h.tri != kNoHit && tt == h.t && (inst > h.inst || (inst == h.inst && prim > h.prim))) &&
                !(pass == 1 && !(PATH ? alphaAcceptPath(sc, inst, prim, uu, vv) : alphaAccept(sc, inst, prim, uu, vv)))) {
                h.t = tt;
                h.u = uu;
                h.v = vv;
                h.tri = ti;
                h.inst = inst;
                h.prim = prim;
                h.backface = bf != (c.w != 0u); // GpuTriangle t2.w: instance flips facing
            }
        }
    }
    if (doNode) {
        cNodes++;
        uint32_t lb, lbits;
        visitNode8(w0, w1, w2, w3, w4, o, idir, oct, tmin, h.t, ts.gBase, ts.gBits, lb, lbits);
        if (lbits) {
            if (ts.tBits == 0) {
                ts.tBase = lb;
                ts.tBits = lbits;
            } else {
                nBase = lb;
                nBits = lbits;
            }
        }
    }
    if (ts.tBits == 0 && nBits != 0) {
        ts.tBase = nBase;
        ts.tBits = nBits;
        nBits = 0;
    }
    return anyHit;
}

// ---------------------------------------------------------------------------
// 2. The sun's shadow rays in light space (SceneArgs::sun_root, ark_ddgi.cpp sunFrame)
// ---------------------------------------------------------------------------
// Light-space coordinates (u, v, w) of a world point: three fp32 dot products (the
// BVH's box inflation covers their rounding, ark_ddgi.cpp).
__device__ __forceinline__ V3 sunCoords(const SceneArgs& sc, V3 p)
{
    const float* F = sc.sun_frame;
    return { fmaf(p.x, F[0], fmaf(p.y, F[1], p.z * F[2])), fmaf(p.x, F[3], fmaf(p.y, F[4], p.z * F[5])), fmaf(p.x, F[6], fmaf(p.y, F[7], p.z * F[8])) };
}

// Bytewise unsigned x >= y of four packed bytes, the result in bit 7 of each byte, from
// xh = x | 0x80808080 and yl = y & 0x7f7f7f7f: d = xh - yl borrows within no byte
// (each byte of xh is >= 0x80 > each of yl), so bit 7 of a byte of d says x_lo7 >= y_lo7;
// with the top bits, x >= y = (x7 & ~y7) | (~(x7 ^ y7) & d7) - one v_bitop3.
__device__ __forceinline__ uint32_t geBytes(uint32_t x, uint32_t y, uint32_t xh, uint32_t yl)
{
    const uint32_t d = xh - yl;
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xb2" : "=v"(r) : "v"(x), "v"(y), "v"(d));
    return r;
}

// Node visit of a ray along +w from light-space point pl (k_trace_shadow<SUN>). With
// the direction exactly +w the slab test of u and v degenerates to "pl's coordinate
// lies in the child's interval" and that of w to "the box reaches above pl": in the
// node's quantized grid, qlo <= floor(Q) and qhi >= ceil(Q) for Q = (pl - anchor) /
// step - no reciprocal, no per-child multiply (the world test: 8 x 19 VALU). The ray's
// tmin is not used (a box between pl and pl + tmin is visited, conservatively). The
// children are visited in slot order: the builder sorted them by their lower w bound
// (Bvh8CollapseOptions::slot_sort_axis), the order the ray meets them.
// The five conditions are tested on four children at once, bytewise within the plane
// words (geBytes), with no lane-mask compares (the per-child form: 40 SDWA v_cmp, 32
// s_and and 8 v_addc). Q is clamped to [0, 255]
// so that floor and ceil are bytes: that can only accept more children (qlo <= 0 for a
// point below the node's anchor, qhi >= 255 above its far side), never fewer, and an
// any-hit result does not depend on extra visits.
__device__ __forceinline__ void visitNodeSun(uint4 w0, uint4 w1, uint4 w2, uint4 w3, uint4 w4, V3 pl, uint32_t& gBase, uint32_t& gBits, uint32_t& tBase,
                                             uint32_t& tBits)
{
    auto quant = [](float c, uint32_t p, uint32_t ebyte) {
        return __builtin_amdgcn_fmed3f(__builtin_amdgcn_ldexpf(c - __uint_as_float(p), 127 - static_cast<int>(ebyte)), 0.0f, 255.0f);
    };
    const float qu = quant(pl.x, w0.x, w0.w & 0xffu), qv = quant(pl.y, w0.y, (w0.w >> 8) & 0xffu), qw = quant(pl.z, w0.z, (w0.w >> 16) & 0xffu);
    constexpr uint32_t kH = 0x80808080u;
    // floor (the truncating conversion: Q >= 0) and ceil of Q, in every byte (v_perm_b32
    // with selector 0: byte 0 of the second operand four times)
    auto bcast = [](float q) { return __builtin_amdgcn_perm(0u, static_cast<uint32_t>(q), 0u); };
    const uint32_t Fu = bcast(qu), Cu = bcast(ceilf(qu)), Fv = bcast(qv), Cv = bcast(ceilf(qv)), Cw = bcast(ceilf(qw));
    const uint32_t FuH = Fu | kH, FvH = Fv | kH, CuL = Cu & ~kH, CvL = Cv & ~kH, CwL = Cw & ~kH;
    // planes (GpuBvh8Node): qlo u = w2.x|y, qlo v = w2.z|w, qhi u = w3.z|w, qhi v = w4.x|y,
    // qhi w = w4.z|w (children 0-3 | 4-7, child k in byte k & 3)
    auto crossed = [&](uint32_t lu, uint32_t hu, uint32_t lv, uint32_t hv, uint32_t hw) {
        return geBytes(Fu, lu, FuH, lu & ~kH) & geBytes(hu, Cu, hu | kH, CuL) & geBytes(Fv, lv, FvH, lv & ~kH) & geBytes(hv, Cv, hv | kH, CvL) &
               geBytes(hw, Cw, hw | kH, CwL) & kH;
    };
    const uint32_t r0 = crossed(w2.x, w3.z, w2.z, w4.x, w4.z), r1 = crossed(w2.y, w3.w, w2.w, w4.y, w4.w);
    // bit 7 of byte k of r0 / r1 -> bit k / k + 4 of the slot mask: the bits of x =
    // (r0 >> 4) | r1 sit at 8k + 3 (child k) and 8k + 7 (child k + 4), and the high word
    // of x * (2^29 + 2^22 + 2^15 + 2^8) holds them at bits k and k + 4 (no two partial
    // products share a bit position, so nothing carries); its bits above 7 are cleared
    // by the 8-bit masks below
    const uint32_t hit = __umulhi((r0 >> 4) | r1, 0x20408100u);
    const uint32_t imask = w0.w >> 24;
    gBase = w1.x;
    gBits = (hit & imask) | (imask << 8);
    tBase = w1.y;
    const uint32_t stride = w1.w & 31u, leafHits = hit & (w1.w >> 8) & 0xffu;
    const uint32_t xl = (leafHits << stride) | leafHits;
    tBits = ((xl << stride) | xl) & w1.z;
}

// travStepDual for a sun shadow ray in the light-space BVH: both sides' loads issued
// by every lane (a skipped side reads the resident record 0 / the root), the
// world-space Möller–Trumbore of the leaf records (the any-hit test of the world
// BVHs, bit for bit), the light-space node test.
template<int BLOCK>
__device__ __forceinline__ bool travStepSun(const SceneArgs& sc, TravState& ts, uint32_t& nBase, uint32_t& nBits, Stack<BLOCK>& st, V3 o, V3 d, V3 pl,
                                            float tmin, float tmax, uint32_t& cNodes, uint32_t& cTris)
{
    bool anyHit = false;
    const bool doTri = ts.tBits != 0;
    const bool doNode = nBits == 0 && ((ts.gBits & 0xffu) != 0 || st.depth != 0);
    uint32_t ti = 0;
    if (doTri) {
        ti = ts.tBase + static_cast<uint32_t>(__builtin_ctz(ts.tBits));
        ts.tBits &= ts.tBits - 1u;
    }
    uint4 a, b, c;
    {
        const uint4* src = reinterpret_cast<const uint4*>(sc.sun_tris + ti);
        a = src[0];
        b = src[1];
        c = src[2];
    }
    uint32_t child = static_cast<uint32_t>(sc.sun_root);
    if (doNode) {
        if ((ts.gBits & 0xffu) == 0) st.pop(ts.gBase, ts.gBits);
        child = nextChild(ts.gBase, ts.gBits, 0u);
        if (ts.gBits & 0xffu) st.push(ts.gBase, ts.gBits);
    }
    uint4 w0, w1, w2, w3, w4;
    {
        const uint4* src = reinterpret_cast<const uint4*>(sc.sun_nodes + child);
        w0 = src[0];
        w1 = src[1];
        w2 = src[2];
        w3 = src[3];
        w4 = src[4];
    }
    if (doTri) {
        cTris++;
        const GpuTriangle tr = triFromWords(a, b, c);
        bool bf;
        float tt, uu, vv;
        anyHit = intersectTri(o, d, tmin, tmax, tr, &tt, &uu, &vv, &bf);
    }
    if (doNode) {
        cNodes++;
        uint32_t lb, lbits;
        visitNodeSun(w0, w1, w2, w3, w4, pl, ts.gBase, ts.gBits, lb, lbits);
        if (lbits) {
            if (ts.tBits == 0) {
                ts.tBase = lb;
                ts.tBits = lbits;
            } else {
                nBase = lb;
                nBits = lbits;
            }
        }
    }
    if (ts.tBits == 0 && nBits != 0) {
        ts.tBase = nBase;
        ts.tBits = nBits;
        nBits = 0;
    }
    return anyHit;
}

// ---------------------------------------------------------------------------
// 3. traversal work distribution
// ---------------------------------------------------------------------------
// XCD-aware work split: the window's probes are cut into kRayParts contiguous
// partitions with one head counter each (ray_counter[p * kRayCounterStride]).
// A wave drains the partition of the XCD it runs on first (read from
// HW_REG_XCC_ID), then steals from the others in order. Rays of neighbouring
// probes touch the same BVH neighbourhood, so each XCD's L2 sees ~1/8 of the
// in-flight working set. Placement only affects speed: every ray is taken
// exactly once whichever wave takes it.
__device__ __forceinline__ uint32_t xccId()
{
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & (kRayParts - 1);
}

// Same partitioned dequeue over a flat list of `total` items (shadow rays).
__device__ __forceinline__ void grabItems(uint32_t* heads, uint32_t total, uint32_t home, uint32_t& tried, uint32_t& b, uint32_t& e, uint32_t CHUNK)
{
    b = e = 0;
    for (; tried < kRayParts; ++tried) {
        const uint32_t p = (home + tried) & (kRayParts - 1);
        const uint32_t pb = static_cast<uint32_t>(static_cast<uint64_t>(total) * p / kRayParts);
        const uint32_t pe = static_cast<uint32_t>(static_cast<uint64_t>(total) * (p + 1) / kRayParts);
        if (pb >= pe) continue;
        const uint32_t off = atomicAdd(heads + p * kRayCounterStride, CHUNK);
        if (off < pe - pb) {
            b = pb + off;
            e = min(b + CHUNK, pe);
            return;
        }
    }
}

__device__ __forceinline__ uint32_t partRayBegin(const FrameArgs& f, uint32_t p)
{
    return static_cast<uint32_t>(static_cast<uint64_t>(f.window_probes) * p / kRayParts) * f.R;
}

// One lane only: next chunk of at most CHUNK consecutive rays from the head
// counters at `heads`, or b >= e when every partition is drained.
// `tried` = partitions already found empty (uniform over the caller's group).
__device__ __forceinline__ void grabRays(const FrameArgs& f, uint32_t* heads, uint32_t home, uint32_t& tried, uint32_t& b, uint32_t& e, uint32_t CHUNK)
{
    b = e = 0;
    for (; tried < kRayParts; ++tried) {
        const uint32_t p = (home + tried) & (kRayParts - 1);
        const uint32_t pb = partRayBegin(f, p), pe = partRayBegin(f, p + 1);
        if (pb >= pe) continue;
        const uint32_t off = atomicAdd(heads + p * kRayCounterStride, CHUNK);
        if (off < pe - pb) {
            b = pb + off;
            e = min(b + CHUNK, pe);
            return;
        }
    }
}

// The same two grabs called by every lane of a wave with wave-uniform arguments
// (k_trace): the partition arithmetic stays on the scalar unit, lane 0 alone adds to
// the head counter and its answer is broadcast. The one-lane forms above run that
// arithmetic as vector instructions with one lane enabled.
__device__ __forceinline__ uint32_t waveAtomicAdd(uint32_t* p, uint32_t v, uint32_t lane)
{
    uint32_t off = 0;
    if (lane == 0) off = atomicAdd(p, v);
    return __builtin_amdgcn_readfirstlane(off);
}

__device__ __forceinline__ void grabItemsWave(uint32_t* heads, uint32_t total, uint32_t home, uint32_t lane, uint32_t& tried, uint32_t& b, uint32_t& e, uint32_t CHUNK)
{
    b = e = 0;
    for (; tried < kRayParts; ++tried) {
        const uint32_t p = (home + tried) & (kRayParts - 1);
        const uint32_t pb = static_cast<uint32_t>(static_cast<uint64_t>(total) * p / kRayParts);
        const uint32_t pe = static_cast<uint32_t>(static_cast<uint64_t>(total) * (p + 1) / kRayParts);
        if (pb >= pe) continue;
        const uint32_t off = waveAtomicAdd(heads + p * kRayCounterStride, CHUNK, lane);
        if (off < pe - pb) {
            b = pb + off;
            e = min(b + CHUNK, pe);
            return;
        }
    }
}

__device__ __forceinline__ void grabRaysWave(const FrameArgs& f, uint32_t* heads, uint32_t home, uint32_t lane, uint32_t& tried, uint32_t& b, uint32_t& e, uint32_t CHUNK)
{
    b = e = 0;
    for (; tried < kRayParts; ++tried) {
        const uint32_t p = (home + tried) & (kRayParts - 1);
        const uint32_t pb = partRayBegin(f, p), pe = partRayBegin(f, p + 1);
        if (pb >= pe) continue;
        const uint32_t off = waveAtomicAdd(heads + p * kRayCounterStride, CHUNK, lane);
        if (off < pe - pb) {
            b = pb + off;
            e = min(b + CHUNK, pe);
            return;
        }
    }
}

} // namespace dev
} // namespace ark
