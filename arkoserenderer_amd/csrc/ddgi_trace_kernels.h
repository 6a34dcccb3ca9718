// ddgi_trace_kernels.h — the two persistent traversal kernel templates over the core of
// ddgi_traversal.h: k_trace (closest hit, a ray source Src) and k_trace_shadow (any hit, a
// shadow MODE). A unit instantiates the instances it launches; each instance is emitted by
// exactly one unit:
//   ddgi_kernels.hip       k_trace<.., ProbeRays, ..>, k_trace_shadow World / Sun / SunWorld
//   ddgi_reflections.hip   k_trace<false, 6, ListRays>
//   ddgi_rt_shadows.hip    k_trace_shadow<false, 6, kShadowOpaque>
//   ddgi_path_tracer.hip   k_trace<false, 6, PathRays>, k_trace_shadow<false, 6, kShadowPath>
#pragma once

#include "ddgi_traversal.h"

namespace ark {
namespace dev {

// Persistent traversal at 6 waves/SIMD (80 VGPRs, no spill; round 1: 3.43 vs 3.61 ms
// at the compiler's 5 on C4, 8 spilled and took 5.4 ms); COUNT variants run at the
// compiler's occupancy.
// Dual-step traversal at 6 waves/SIMD (80 VGPRs): the only spills (4 VGPRs) sit in
// the masked pass's alpha test. C4: 2.39 ms, against 2.51 at 5 waves (96 VGPRs, no
// spill) and 2.65 for one step per iteration at 6 waves.
constexpr int kTraceWpe = 6, kShadowWpe = 6;

// ---------------------------------------------------------------------------
// 1. k_trace: closest-hit traversal (persistent, per-lane wave64 ballot refill)
// ---------------------------------------------------------------------------
// Every lane owns one probe ray at a time (pass 0 opaque, 1 masked). One outer
// iteration visits one BVH8 node or one leaf triangle per active lane; lanes whose
// ray finished are refilled at the top of the next iteration from a wave-private
// pool of consecutive rays (ballot + mbcnt rank, one atomic per 64 rays), so the SIMD
// stays full until the global ray counter runs out.
//
// The pool holds ray records, not just indices: when a wave grabs a chunk of at most
// 64 consecutive rays, lane i sets up ray i of the chunk with every lane enabled
// (Src::stage: the slot, origin and direction lookups, the rotation) and parks the
// record in slot i of the wave's LDS region. A refill, which runs with a quarter of
// the lanes, then only reads a record: no global load stands between a refill and
// the new rays' first node fetch. The setup used to run in every refill, about four
// times per chunk at quarter occupancy, behind two dependent global loads.

// Ray record of the pool: origin, direction, one word of the source's own (28 B in a
// 32-B slot, read and written as two 16-B halves).
struct PoolRec {
    V3 o, d;
    uint32_t a;
    uint32_t c; // the ray's hit candidate (seed_cache.h): a triangle record or seed::kNone
};

// The ray source Src of k_trace: a struct of static members, defined by the unit that
// instantiates the kernel with it (ProbeRays: ddgi_kernels.hip, ListRays:
// ddgi_reflections.hip, PathRays: ddgi_path_tracer.hip).
//   kAllClasses  bool: one closest hit over the opaque, masked and blend classes in turn
//                (`pass` is the class, class 1's candidates take alphaAcceptPath, the record's
//                word is the ray's tmin, an empty list returns at once); false: the opaque
//                class, then kMaskedPass
//   kMaskedPass  bool: an alpha-tested masked pass over [tmin, opaque hit] follows the
//                opaque pass
//   kSeeds       bool: the source's rays are offered a hit candidate (stage looks it up,
//                checked by seed::candidateOk against the launch's opaque class) and leave
//                their opaque-pass hit in the cache
//   kTmin        float: the rays' tmin (unless kAllClasses)
//   grab(f, home, lane, tried, b, e, chunk)  the next chunk [b, e) of at most `chunk` rays,
//                called by every lane of the wave with wave-uniform arguments; b >= e when
//                the supply is drained
//   stage(sc, f, r) -> PoolRec  the record of ray r (every lane, once per chunk)
//   take(f, r, recA, ray, tmax)  what a lane starting ray r needs besides o and d (hit
//                record index, tmax), from the record's own word

// SLOTS: records per wave pool. A chunk never exceeds it (the grab size is clamped to
// it below). 64 for the whole-grid launches; the half-occupancy windows, which grab 32
// rays at a time, run the 32-slot instance: their three workgroups per CU share the CU
// with the previous frame's shadow traversal and shading, and 4 KB of LDS per workgroup
// that no chunk would ever fill are taken from those (launch_trace).
// SEEDW: the instance leaves its rays' opaque-pass hits in the seed cache itself
// (FrameArgs::seed_offsets_write 0 with a cache).
template<bool COUNT, int WPE, class Src, int SLOTS = 64, bool SEEDW = false>
__global__ void __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(WPE))) k_trace(SceneArgs sc, FrameArgs f)
{
    if (frameAborted(f.abort_word)) return;
    if constexpr (Src::kAllClasses)
        if (*f.list_count == 0u) return;
    __shared__ uint32_t ldsStack[kStackLds * 2 * kTraceBlock];
    // nodes from global memory only (GF dual steps): no LDS node cache, the octant table
    __shared__ uint4 ldsNodes[5];
    // the waves' ray pools: SLOTS records each, as two 16-B halves [wave][half][slot]
    static_assert(SLOTS == 32 || SLOTS == 64, "a wave stages at most one record per lane");
    __shared__ uint4 ldsPool[2 * SLOTS * (kTraceBlock / 64)];
    const NodeCache nc = loadNodeCache<kTraceBlock, 0>(sc, ldsNodes);
    const uint32_t gtid = blockIdx.x * kTraceBlock + threadIdx.x;
    const uint32_t nthreads = gridDim.x * kTraceBlock;
    Stack<kTraceBlock> st { ldsStack + threadIdx.x, f.spill + gtid, nthreads, 0 };
    const uint32_t lane = threadIdx.x & 63u;
    uint4* const pool = ldsPool + 2u * SLOTS * (threadIdx.x >> 6);
    const uint32_t chunk = min(f.grab_chunk, static_cast<uint32_t>(SLOTS)); // a chunk fits the pool
    float tmin = Src::kTmin;
    auto classRoot = [&](int c) { return c == 0 ? sc.root_opaque : (c == 1 ? sc.root_masked : sc.root_blend); }; // (Src::kAllClasses; no indexed array: scratch)
    uint32_t cNodes = 0, cTris = 0, cHits = 0, cIter = 0, rSteps = 0;
    uint32_t cSeedHits = 0, seedTri = seed::kNone; // (COUNT) rays whose candidate was hit; the candidate of a ray's first step

    uint32_t poolNext = 0, poolEnd = 0; // rays of the pool not handed out yet
    uint32_t poolBase = 0;              // the ray whose record is in slot 0
    const uint32_t home = xccId();
    uint32_t tried = 0; // partitions found drained (wave-uniform)
    bool exhausted = false;
    bool active = false;
    uint32_t ray = 0;
    int pass = 0; // 0 opaque, 1 masked
    TravState ts { 0u, 0u, 0u, 0u };
    uint32_t nBase = 0, nBits = 0; // the next triangle group (dual step)
    uint32_t oct = 0;
    V3 o = { 0, 0, 0 }, d = { 0, 0, 1 }, idir = { 0, 0, 1 };
    RayHit h { 0.0f, 0.0f, 0.0f, kNoHit, 0u, 0u, false };
    float opaqueT = 0.0f; // signed t of the opaque hit, kept for the masked pass
    auto done = [&]() { return travDoneDual(ts, nBits, st); };
    // Deferred retirement: without a masked pass to continue into, a lane whose ray is
    // done only goes idle, and its hit record is written at the next refill, just
    // before the lane takes a new ray. A lane finishes a ray in nearly every step of a
    // wave (one ray per lane every ~25 steps), so the exec-masked store path would
    // otherwise run almost every step; at a refill it runs once per batch of idle
    // lanes. Lanes that finish after the ray supply is exhausted retire at once.
    bool pending = false;
    // The opaque pass's hit becomes the candidate of the probe's next ray in this direction
    // (a plain store: a lost race only changes which valid candidate is seen; a miss writes
    // nothing). h.tri is a record of the opaque class of the tree this launch traverses.
    auto seedWrite = [&]() {
        if (Src::kSeeds && SEEDW && h.tri != kNoHit) {
            const uint32_t probe = f.slots[ray / f.R].probe_index;
            f.seed_cache[static_cast<size_t>(probe) * seed::kProbeWords + seed::texelOf(d.x, d.y, d.z)] = h.tri;
        }
    };
    auto storeHit = [&]() {
        if (pass == 0) seedWrite();
        GpuHit out;
        if (h.tri == kNoHit) {
            out.t = __builtin_bit_cast(float, 0x7f800000u);
            out.u = out.v = 0.0f;
            out.tri = kNoHit;
        } else {
            out.t = h.backface ? -h.t : h.t;
            out.u = h.u;
            out.v = h.v;
            out.tri = h.tri;
            if (COUNT) cHits++;
        }
        f.hits[ray] = out;
        if (COUNT && f.ray_steps) f.ray_steps[ray] = static_cast<uint16_t>(min(rSteps, 65535u));
        if (COUNT) rSteps = 0;
    };

    for (;;) {
        // ---- refill finished lanes --------------------------------------------
        const uint64_t need = __ballot(!active);
        if (need != 0 && !exhausted && (static_cast<uint32_t>(__popcll(need)) >= f.refill_min || need == ~0ull)) {
            if (pending) {
                storeHit();
                pending = false;
            }
            const uint32_t n = static_cast<uint32_t>(__popcll(need));
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(need >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(need), 0u));
            const uint32_t avail = poolEnd - poolNext;
            uint32_t fb = 0, fe = 0; // fresh chunk [fb, fe)
            if (avail < n) Src::grab(f, home, lane, tried, fb, fe, chunk); // every lane, wave-uniform
            // An idle lane takes ray r by its rank among the idle lanes: the pool's
            // leftover first, then the fresh chunk. The leftover records are read
            // before the chunk is staged over them, and the chunk is staged before its
            // records are read. The region is the wave's own, so no workgroup barrier:
            // what is relied on is that the compiler keeps the region's reads and
            // writes in program order (one sequentially consistent wave-level fence
            // on each side of the staging) and that a wave's LDS operations execute
            // in the order issued. A record goes straight into the idle lane's own o
            // and d.
            uint32_t r = kNoHit, recA = 0, recC = seed::kNone;
            auto readRec = [&](uint32_t slot) {
                const uint4 lo = pool[slot], hi = pool[SLOTS + slot];
                o = { __uint_as_float(lo.x), __uint_as_float(lo.y), __uint_as_float(lo.z) };
                d = { __uint_as_float(lo.w), __uint_as_float(hi.x), __uint_as_float(hi.y) };
                recA = hi.z;
                recC = hi.w;
            };
            if (!active && rank < avail) {
                r = poolNext + rank;
                readRec(r - poolBase);
            }
            if (fb < fe) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (lane < fe - fb) {
                    const PoolRec s = Src::stage(sc, f, fb + lane);
                    pool[lane] = make_uint4(__float_as_uint(s.o.x), __float_as_uint(s.o.y), __float_as_uint(s.o.z), __float_as_uint(s.d.x));
                    pool[SLOTS + lane] = make_uint4(__float_as_uint(s.d.y), __float_as_uint(s.d.z), s.a, s.c);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                poolBase = __builtin_amdgcn_readfirstlane(fb);
                if (!active && rank >= avail && rank - avail < fe - fb) {
                    r = fb + (rank - avail);
                    readRec(rank - avail);
                }
            }
            if (r != kNoHit) {
                float tmax;
                Src::take(f, r, recA, ray, tmax);
                idir = safeInv(d);
                oct = rayOctant(idir);
                active = true;
                h = RayHit { tmax, 0.0f, 0.0f, kNoHit, 0u, 0u, false };
                pass = 0;
                st.depth = 0;
                nBits = 0;
                // the candidate is the ray's first pending triangle group: the step below tests
                // it like any leaf triangle, and the root visit of that step sees its h.t
                ts = TravState { static_cast<uint32_t>(sc.root_opaque), sc.root_opaque >= 0 ? rootGroupBits() : 0u, recC, recC != seed::kNone ? 1u : 0u };
                if constexpr (Src::kAllClasses) {
                    tmin = __uint_as_float(recA);
                    while (pass < 3 && classRoot(pass) < 0) ++pass;
                    ts = TravState { pass < 3 ? static_cast<uint32_t>(classRoot(pass)) : 0u, pass < 3 ? rootGroupBits() : 0u, 0u, 0u };
                }
                if (COUNT) seedTri = recC;
            }
            if (avail < n) {
                if (fb >= fe) {
                    exhausted = true;
                    poolNext = poolEnd = 0;
                } else {
                    poolNext = min(fb + (n - avail), fe);
                    poolEnd = fe;
                }
            } else {
                poolNext += n;
            }
        }
        if (__ballot(active) == 0) break;
        if (COUNT) {
            cIter++;
            rSteps += active ? 1u : 0u;
        }
        // ---- one step: a pending leaf triangle and the next node -------------------
        // (an active lane is never done here: the check after the step retires or
        // restarts it, and a step of a done lane would change nothing anyway)
        if (active) travStepDual<kTraceBlock, false, true, Src::kAllClasses>(sc, nc, ts, nBase, nBits, st, o, d, idir, oct, tmin, h, pass, cNodes, cTris);
        if (COUNT && active && seedTri != seed::kNone) {
            cSeedHits += h.tri == seedTri ? 1u : 0u;
            seedTri = seed::kNone;
        }
        // ---- pass finished -------------------------------------------------------------
        if constexpr (Src::kAllClasses) {
            // the next class with geometry, the hit so far kept (h.t is the query's tmax)
            if (active && done()) {
                ++pass;
                while (pass < 3 && classRoot(pass) < 0) ++pass;
                if (pass < 3) {
                    ts = TravState { static_cast<uint32_t>(classRoot(pass)), rootGroupBits(), 0u, 0u };
                    st.depth = 0;
                } else if (!exhausted) {
                    active = false;
                    pending = true;
                } else {
                    storeHit();
                    active = false;
                }
            }
        } else if (active && done() && (!Src::kMaskedPass || sc.root_masked < 0) && !exhausted) {
            active = false;
            pending = true;
        } else if (active && done()) {
            bool finished = true;
            if (Src::kMaskedPass && pass == 0) {
                // opaque pass done (raygen.rgen:35-62); masked pass: RayFlags_NoOpaque,
                // cullMask 0x02, tmax = previous hit T (:64-92); a negative tmax
                // (backface) is an empty interval.
                opaqueT = (h.tri != kNoHit) ? (h.backface ? -h.t : h.t) : f.z_far;
                if (sc.root_masked >= 0 && opaqueT >= tmin) {
                    seedWrite();
                    pass = 1;
                    finished = false;
                    ts = TravState { static_cast<uint32_t>(sc.root_masked), rootGroupBits(), 0u, 0u };
                    st.depth = 0;
                    // stash the opaque hit; the masked pass searches [tmin, opaqueT]
                    f.hits[ray] = GpuHit { h.tri == kNoHit ? __builtin_bit_cast(float, 0x7f800000u) : opaqueT, h.u, h.v, h.tri };
                    h = RayHit { opaqueT, 0.0f, 0.0f, kNoHit, 0u, 0u, false };
                }
            }
            if (finished) {
                GpuHit out;
                if (pass == 1 && h.tri == kNoHit) {
                    // masked pass found nothing: the opaque result (already stored) stands
                    out = f.hits[ray];
                    if (COUNT && out.tri != kNoHit) cHits++;
                    if (COUNT && f.ray_steps) f.ray_steps[ray] = static_cast<uint16_t>(min(rSteps, 65535u));
                    if (COUNT) rSteps = 0;
                } else {
                    storeHit();
                }
                active = false;
            }
        }
    }
    if (COUNT) {
        atomicAdd(&f.counters[0], static_cast<unsigned long long>(cNodes));
        atomicAdd(&f.counters[1], static_cast<unsigned long long>(cTris));
        atomicAdd(&f.counters[2], static_cast<unsigned long long>(cHits));
        if (lane == 0) atomicAdd(&f.counters[7], static_cast<unsigned long long>(cIter));
        if (f.seed_counts) atomicAdd(&f.seed_counts[0], cSeedHits);
    }
}

// ---------------------------------------------------------------------------
// 2. k_trace_shadow: any-hit traversal of a shadow-ray list
// ---------------------------------------------------------------------------
// Intra-wave splitting of the traversal tail:
// Once the ray supply has run dry, a persistent traversal wave only runs its last,
// longest rays, one dependent node fetch per iteration, while most of its lanes
// idle (C4: the shadow kernel spent 0.28 of 0.64 ms draining). So an idle lane of
// an exhausted wave takes work from a lane that is still traversing: the donor
// hands over the bottom entry of its node-group stack (the oldest deferred group,
// usually the largest subtree left) and the helper traverses that group with a
// copy of the donor's ray. Helpers can donate again; every helper reports to the
// ray's root lane, which finishes the ray only when its helper count is back to
// zero. The result does not depend on who visits which subtree: any-hit rays OR
// their occlusion, closest-hit rays keep the nearest hit with the (instance,
// primitive) tie rule, and box culling is conservative for any tmax that bounds
// the closest hit.
// Per wave LDS: a 64-entry donor table (rank -> donor lane) and, per lane, a byte
// with its outstanding helper count (bits 0-6) and a "ray resolved" flag (bit 7).
struct TailLds {
    uint8_t* table;  // [kTraceBlock]
    uint32_t* bytes; // [kTraceBlock / 4], one byte per lane
};

__device__ __forceinline__ uint32_t tailByte(const TailLds& tl, uint32_t t)
{
    return (__hip_atomic_load(tl.bytes + (t >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) >> (8u * (t & 3u))) & 0xffu;
}

__device__ __forceinline__ void tailAdd(const TailLds& tl, uint32_t t, uint32_t v)
{
    __hip_atomic_fetch_add(tl.bytes + (t >> 2), v << (8u * (t & 3u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void tailSub(const TailLds& tl, uint32_t t, uint32_t v)
{
    __hip_atomic_fetch_sub(tl.bytes + (t >> 2), v << (8u * (t & 3u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void tailOr(const TailLds& tl, uint32_t t, uint32_t v)
{
    __hip_atomic_fetch_or(tl.bytes + (t >> 2), v << (8u * (t & 3u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void tailClear(const TailLds& tl, uint32_t t)
{
    __hip_atomic_fetch_and(tl.bytes + (t >> 2), ~(0xffu << (8u * (t & 3u))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Removes the bottom entry (entry 0) of a non-empty stack and returns it; the top
// entry moves into its place (visiting order only affects speed).
template<int BLOCK>
__device__ __forceinline__ void stackTakeBottom(Stack<BLOCK>& st, uint32_t& a, uint32_t& b)
{
    // entry i is in LDS slot i % kStackLds while i >= depth - kStackLds, else at spill[i]
    if (st.depth <= kStackLds) {
        a = st.lds[0];
        b = st.lds[BLOCK];
    } else {
        a = st.spill[0];
        b = st.spill[st.spillStride];
    }
    uint32_t ta, tb;
    st.pop(ta, tb);
    if (st.depth > 0) {
        if (st.depth <= kStackLds) {
            st.lds[0] = ta;
            st.lds[BLOCK] = tb;
        } else {
            st.spill[0] = ta;
            st.spill[st.spillStride] = tb;
        }
    }
}

__device__ __forceinline__ V3 shfl3(V3 v, uint32_t src)
{
    return v3(__shfl(v.x, static_cast<int>(src)), __shfl(v.y, static_cast<int>(src)), __shfl(v.z, static_cast<int>(src)));
}

// Persistent any-hit traversal of the shadow-ray list (opaque.rchit:35-54:
// TerminateOnFirstHit | SkipClosestHit | Opaque, cullMask 0xff, tmin 0.025): the
// three hit-mask classes in turn, no alpha test, dual steps. Lanes are refilled
// from a wave-private pool like k_trace; an occluded ray sets bit 16 + light of its
// probe ray's word. `pass` of a helper lane holds (root lane + 1) << 8.
// MODE: kShadowWorld - the shadow rays through the three world BVHs; kShadowSun - the
// sun's list (FrameArgs::sun_rays) through the light-space BVH (one pass, travStepSun);
// kShadowSunWorld - both in one launch: each wave drains the sun's list, then takes
// rays from the other list, so the first list's tail overlaps the second list's work
// instead of ending a launch (C5: 1.98 ms one list, 3.27 ms two launches).
// kShadowOpaque - the list through the opaque class's world BVH only (cullMask
// RT_HIT_MASK_OPAQUE: rt-shadow/raygen.rgen:64-65, ddgi_rt_shadows.hip); an instantiation
// of its own, the other modes' code is what it was.
// kShadowPath - the path tracer's shadow rays (closesthit.rchit:31-49: cullMask opaque | masked,
// RayFlags_Opaque): roots {opaque, masked, -1}, no alpha test; an empty list returns at once.
constexpr int kShadowWorld = 0, kShadowSun = 1, kShadowSunWorld = 2, kShadowOpaque = 3, kShadowPath = 4;

template<bool COUNT, bool SUN, bool OPAQUE_ONLY = false, bool NO_BLEND = false>
__device__ __forceinline__ void shadowPhase(const SceneArgs& sc, const FrameArgs& f, const NodeCache& nc, Stack<kTraceBlock>& st, const TailLds& tl,
                                            uint32_t& cNodes, uint32_t& cTris, uint32_t& cShadow)
{
    const uint32_t lane = threadIdx.x & 63u, wbase = threadIdx.x & ~63u;
    if (lane < 16u) tl.bytes[(wbase >> 2) + lane] = 0u; // wave-private tail bytes
    const float tmin = 0.025f;
    const uint32_t total = SUN ? *f.sun_count : *f.shadow_count;
    uint32_t* const heads = SUN ? f.sun_heads : f.shadow_heads;
    const ShadowRay* const list = SUN ? f.sun_rays : f.shadow_rays;
    const int32_t roots[3] = { SUN ? sc.sun_root : sc.root_opaque, SUN || OPAQUE_ONLY ? -1 : sc.root_masked, SUN || OPAQUE_ONLY || NO_BLEND ? -1 : sc.root_blend };

    uint32_t poolNext = 0, poolEnd = 0;
    const uint32_t home = xccId();
    uint32_t tried = 0;
    bool exhausted = false, active = false;
    uint32_t owner = 0;
    int pass = 0;
    float tmax = 0.0f;
    TravState ts { 0u, 0u, 0u, 0u };
    uint32_t nBase = 0, nBits = 0; // the next triangle group (dual step)
    uint32_t oct = 0;
    V3 o = { 0, 0, 0 }, d = { 0, 0, 1 }, idir = { 0, 0, 1 };
    auto done = [&]() { return travDoneDual(ts, nBits, st); };
    auto stop = [&]() { ts = TravState { 0u, 0u, 0u, 0u }; nBits = 0; st.depth = 0; };
    for (;;) {
        const uint64_t need = __ballot(!active);
        if (need != 0 && !exhausted && (static_cast<uint32_t>(__popcll(need)) >= (SUN ? f.sun_refill_min : f.refill_min) || need == ~0ull)) {
            const uint32_t n = static_cast<uint32_t>(__popcll(need));
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(need >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(need), 0u));
            const uint32_t avail = poolEnd - poolNext;
            uint32_t fb = 0, fe = 0;
            if (avail < n) {
                uint32_t b = 0, e = 0, t = tried;
                if (lane == 0) grabItems(heads, total, home, t, b, e, f.grab_chunk);
                fb = __shfl(b, 0);
                fe = __shfl(e, 0);
                tried = __shfl(t, 0);
            }
            if (!active) {
                uint32_t r = kNoHit;
                if (rank < avail) r = poolNext + rank;
                else if (fb + (rank - avail) < fe) r = fb + (rank - avail);
                if (r != kNoHit) {
                    const ShadowRay sr = list[r];
                    o = v3(sr.origin_tmax.x, sr.origin_tmax.y, sr.origin_tmax.z);
                    d = v3(sr.dir_owner.x, sr.dir_owner.y, sr.dir_owner.z);
                    tmax = sr.origin_tmax.w;
                    owner = __float_as_uint(sr.dir_owner.w);
                    // SUN: idir holds the origin's light-space coordinates
                    idir = SUN ? sunCoords(sc, o) : safeInv(d);
                    oct = SUN ? 0u : rayOctant(idir);
                    stop();
                    pass = 0;
                    active = true;
                    if (tmax >= tmin) {
                        if (COUNT) cShadow++;
                        while (pass < 3 && roots[pass] < 0) ++pass;
                        if (pass < 3) ts = TravState { static_cast<uint32_t>(roots[pass]), rootGroupBits(), 0u, 0u };
                    } else {
                        pass = 3; // !(maxDistance >= tmin): not traced, not occluded
                    }
                }
            }
            if (avail < n) {
                if (fb >= fe) {
                    exhausted = true;
                    poolNext = poolEnd = 0;
                } else {
                    poolNext = min(fb + (n - avail), fe);
                    poolEnd = fe;
                }
            } else {
                poolNext += n;
            }
        }
        if (__ballot(active) == 0) break;
        if (exhausted) {
            // ---- tail: resolved rays stop, idle lanes take stack bottoms --------------
            const uint32_t root = pass >= 256 ? static_cast<uint32_t>(pass >> 8) - 1u : lane;
            if (active && (tailByte(tl, wbase + root) & 0x80u)) stop();
            const uint64_t idle = __ballot(!active);
            const bool can = active && st.depth > 0;
            const uint64_t donors = __ballot(can);
            const uint32_t m = min(static_cast<uint32_t>(__popcll(idle)), static_cast<uint32_t>(__popcll(donors)));
            if (m != 0) {
                const uint32_t dr = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(donors >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(donors), 0u));
                const uint32_t ir = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(idle >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(idle), 0u));
                uint32_t gB = 0, gBits = 0;
                if (can && dr < m) {
                    stackTakeBottom(st, gB, gBits);
                    tl.table[wbase + dr] = static_cast<uint8_t>(lane);
                    tailAdd(tl, wbase + root, 1u);
                }
                // every lane shuffles (a lane that takes nothing reads its own values)
                const bool take = !active && ir < m;
                const uint32_t src = take ? tl.table[wbase + ir] : lane;
                o = shfl3(o, src);
                d = shfl3(d, src);
                tmax = __shfl(tmax, static_cast<int>(src));
                owner = __shfl(owner, static_cast<int>(src));
                const uint32_t sroot = __shfl(root, static_cast<int>(src));
                gB = __shfl(gB, static_cast<int>(src));
                gBits = __shfl(gBits, static_cast<int>(src));
                if (take) {
                    idir = SUN ? sunCoords(sc, o) : safeInv(d);
                    oct = SUN ? 0u : rayOctant(idir);
                    pass = static_cast<int>((sroot + 1u) << 8);
                    stop();
                    ts = TravState { gB, gBits, 0u, 0u };
                    active = true;
                }
            }
        }
        if (active) {
            // (a done lane - a root waiting for its helpers - steps as a no-op)
            bool occluded;
            if constexpr (SUN) {
                occluded = travStepSun<kTraceBlock>(sc, ts, nBase, nBits, st, o, d, idir, tmin, tmax, cNodes, cTris);
            } else {
                RayHit h { tmax, 0.0f, 0.0f, kNoHit, 0u, 0u, false };
                occluded = travStepDual<kTraceBlock, true, false>(sc, nc, ts, nBase, nBits, st, o, d, idir, oct, tmin, h, 0, cNodes, cTris);
            }
            const bool helper = pass >= 256;
            const uint32_t root = helper ? static_cast<uint32_t>(pass >> 8) - 1u : lane;
            if (occluded) {
                atomicOr(&f.shadow_bits[owner >> 4], 1u << (16u + (owner & 15u)));
                if (exhausted) tailOr(tl, wbase + root, 0x80u);
                stop();
                if (!helper) pass = 3; // no further hit-mask classes
            }
            if (done()) {
                if (helper) {
                    tailSub(tl, wbase + root, 1u);
                    active = false;
                } else if (!exhausted || (tailByte(tl, wbase + lane) & 0x7fu) == 0) {
                    if (exhausted && (tailByte(tl, wbase + lane) & 0x80u)) pass = 3; // a helper found the occluder
                    ++pass;
                    while (pass < 3 && roots[pass] < 0) ++pass;
                    if (pass < 3) {
                        st.depth = 0;
                        ts = TravState { static_cast<uint32_t>(roots[pass]), rootGroupBits(), 0u, 0u };
                    } else {
                        if (exhausted) tailClear(tl, wbase + lane);
                        active = false;
                    }
                }
            }
        }
    }
}

template<bool COUNT, int WPE, int MODE = kShadowWorld>
__global__ void __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(WPE))) k_trace_shadow(SceneArgs sc, FrameArgs f)
{
    if (frameAborted(f.abort_word)) return;
    if constexpr (MODE == kShadowPath)
        if (*f.shadow_count == 0u) return;
    __shared__ uint32_t ldsStack[kStackLds * 2 * kTraceBlock];
    // 8 cached nodes fewer than k_trace: the tail tables then fit 6 workgroups per CU
    // (the light-space traversal caches none)
    constexpr int kNodes = MODE == kShadowSun ? 1 : kShadowLdsNodes;
    __shared__ uint4 ldsNodes[kNodes * 5];
    __shared__ uint8_t ldsTable[kTraceBlock];
    __shared__ uint32_t ldsBytes[kTraceBlock / 4];
    NodeCache nc { nullptr, 0u, 0u };
    if constexpr (MODE != kShadowSun) nc = loadNodeCache<kTraceBlock, kNodes>(sc, ldsNodes);
    (void)ldsNodes;
    const TailLds tl { ldsTable, ldsBytes };
    const uint32_t gtid = blockIdx.x * kTraceBlock + threadIdx.x;
    Stack<kTraceBlock> st { ldsStack + threadIdx.x, f.spill + gtid, gridDim.x * kTraceBlock, 0 };
    uint32_t cNodes = 0, cTris = 0, cShadow = 0;
    if constexpr (MODE == kShadowOpaque) {
        shadowPhase<COUNT, false, true>(sc, f, nc, st, tl, cNodes, cTris, cShadow);
    } else if constexpr (MODE == kShadowPath) {
        shadowPhase<COUNT, false, false, true>(sc, f, nc, st, tl, cNodes, cTris, cShadow);
    } else {
        if constexpr (MODE != kShadowWorld) shadowPhase<COUNT, true>(sc, f, nc, st, tl, cNodes, cTris, cShadow);
        if constexpr (MODE != kShadowSun) shadowPhase<COUNT, false>(sc, f, nc, st, tl, cNodes, cTris, cShadow);
    }
    if (COUNT) {
        atomicAdd(&f.counters[4], static_cast<unsigned long long>(cNodes));
        atomicAdd(&f.counters[5], static_cast<unsigned long long>(cTris));
        atomicAdd(&f.counters[3], static_cast<unsigned long long>(cShadow));
    }
}

} // namespace dev
} // namespace ark
