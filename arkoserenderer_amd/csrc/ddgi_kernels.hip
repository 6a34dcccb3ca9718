// ddgi_kernels.hip — the DDGI probe-update hot path as HIP kernels for gfx950.
//
// One update (DDGINode.cpp:132-259) is these launches on one stream:
//   1. k_probe_slots    window -> slot table (probe position + offset, per-probe
//                       ray rotation), the slots' traversal order and the
//                       spherical-Fibonacci table.
//   2. k_trace          persistent traversal of all K*R probe rays: opaque pass
//                       (closest hit) then masked pass (alpha-tested any-hit),
//                       software 8-wide quantized BVH (80 B nodes) with a per-lane
//                       LDS ring stack of node groups (spilling to HBM only beyond
//                       kStackLds entries) and wave64 ballot refill of finished
//                       lanes from a wave-private LDS pool of staged ray records
//                       (raygen.rgen:35-92).
//   3. k_shadow_gen     lit lights of every front hit -> shadow-ray list; the sun's ray
//                       resolved from the sun's cover map where its cell decides it
//                       (sun_cover_map.h) and not listed then
//      k_trace_shadow   persistent any-hit traversal of that list (opaque.rchit:35-54).
//   4. k_shade          closest-hit shading (opaque.rchit:105-176) with the shadow
//                       bits, environment on miss (raygen.rgen:71-80), indirect from
//                       the previous frame's atlases (probeSampling.glsl:64-163)
//                       -> fp16 surfels.
//      The sun-only schedule (shade_schedule.h: the sun is the only light and its cover
//      map is in use) has no k_shadow_gen: k_shade resolves the sun's ray itself and
//      shades; the rays the map leaves undecided it lists, k_trace_shadow traces them,
//      and a deferred k_shade instance shades those (3'. k_shade, k_trace_shadow,
//      4'. k_shade<kShadeDeferred>).
//   5. k_probe_update  (ddgi_update.hip) irradiance + visibility blend,
//                       tile border copy, probe offsets.
// No MFMA: the path is traversal/gather, latency/issue bound.
//
// This unit holds the update only. The traversal core is ddgi_traversal.h; k_trace and
// k_trace_shadow are the templates of ddgi_trace_kernels.h, instantiated here with the probe
// rays' source (ProbeRays) and the World / Sun / SunWorld shadow modes; k_shadow_gen and
// the front-hit shading are ddgi_shading.h's, the atlas lookup ddgi_sampling.h's. The other
// passes have units of their own: ddgi_bake.hip, ddgi_compose.hip, ddgi_reflections.hip,
// ddgi_rt_shadows.hip, ddgi_path_tracer.hip. Launchers follow the kernels.

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "../../include/ark_ddgi.h"
#include "ddgi_device.h"
#include "ddgi_kernels.h"
#include "ddgi_shading.h"
#include "ddgi_trace_kernels.h"

namespace ark {
namespace dev {

// ---------------------------------------------------------------------------
// 1. window -> slots
// ---------------------------------------------------------------------------
// sphericalFibonacciSample (common.glsl:121-130)
__device__ V3 sphericalFibonacciSample(uint32_t i, uint32_t n)
{
    float theta = kTwoPi * static_cast<float>(i) / kGoldenRatio;
    float phi = acosf_(2.0f * (static_cast<float>(i) / static_cast<float>(n)) - 1.0f);
    float sinPhi = sinf_(phi);
    float st, ct;
    sincosf_(theta, &st, &ct);
    return { ct * sinPhi, st * sinPhi, cosf_(phi) };
}

// Writes slot `slot` for probe `probeIdx` (ddgi/common.glsl:12-25 seed/rotation,
// :69-77 position, raygen.rgen:117-118 offset).
__device__ void writeSlot(const FrameArgs& f, uint32_t slot, uint32_t probeIdx)
{
    uint32_t tilesPerSheet = static_cast<uint32_t>(f.X * f.Z);
    uint32_t sheetProbeIdx = probeIdx % tilesPerSheet;
    int y = static_cast<int>(probeIdx / tilesPerSheet);
    int x = static_cast<int>(sheetProbeIdx % static_cast<uint32_t>(f.X));
    int z = static_cast<int>(sheetProbeIdx / static_cast<uint32_t>(f.X));
    V3 c = { static_cast<float>(x), static_cast<float>(y), static_cast<float>(z) };
    V3 pos = v3(f.origin[0], f.origin[1], f.origin[2]) + c * v3(f.spacing[0], f.spacing[1], f.spacing[2]);
    float4 off = f.offsets[probeIdx];
    pos = pos + v3(off.x, off.y, off.z);
    uint32_t st = wang_hash(512u * probeIdx + f.frame % 512u);
    // randomPointOnSphere (random.glsl:63-74)
    float theta = kTwoPi * randomFloat(st);
    float u = 2.0f * randomFloat(st) - 1.0f;
    float sr = sqrtf_(1.0f - u * u);
    float s, cth;
    sincosf_(theta, &s, &cth);
    V3 axis = { sr * cth, sr * s, u };
    float angle = kTwoPi * randomFloat(st);
    float as, ac;
    sincosf_(angle, &as, &ac);
    GpuProbeSlot ps;
    ps.pos[0] = pos.x;
    ps.pos[1] = pos.y;
    ps.pos[2] = pos.z;
    ps.probe_index = probeIdx;
    ps.axis[0] = axis.x;
    ps.axis[1] = axis.y;
    ps.axis[2] = axis.z;
    ps.angle_sin = as;
    ps.angle_cos = ac;
    ps._pad[0] = ps._pad[1] = ps._pad[2] = 0.0f;
    f.slots[slot] = ps;
}

__device__ __forceinline__ bool inSlab(const FrameArgs& f, uint32_t probeIdx)
{
    uint32_t sheetProbeIdx = probeIdx % static_cast<uint32_t>(f.X * f.Z);
    int z = static_cast<int>(sheetProbeIdx / static_cast<uint32_t>(f.X));
    return z >= f.slab_z0 && z < f.slab_z1;
}

// Unsharded: slot s <-> probe (first + s) % N (raygen.rgen:113). Sharded (Z-slab):
// the window's slab probes in window order, each slot from the closed-form count of
// slab probes before it (slabRankOf), so slots are deterministic and one thread each.
// Traversal order of the slots (f.slot_order: queue position -> slot), in the same
// pass: the probes are cut into 8 blocks of the x-z plane (4 along x, 2 along z, or
// 8 along x for a one-layer slab) and each block's slots keep their window order,
// whose slowest coordinate is y (a stable bucket sort, in closed form: slotQueuePos).
// The trace and shade queues hand the 8 per-XCD partitions out in this order, so
// partition p sweeps block p bottom to top and all XCDs work on the same few y-layers
// at any time: the chip-wide working set of BVH nodes and triangles is one slice of
// the scene (Infinity Cache sized) instead of eight. Only the order of work changes,
// never a result.
__global__ void __launch_bounds__(256) k_probe_slots(FrameArgs f)
{
    if (frameAborted(f.abort_word)) return;
    const uint32_t X = static_cast<uint32_t>(f.X), Y = static_cast<uint32_t>(f.Y), Z = static_cast<uint32_t>(f.Z);
    const uint32_t N = X * Y * Z;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    // this frame's work counters (trace / shadow heads, shadow-list count): zeroed here
    // rather than by a separate fill ahead of this kernel on the traversal stream
    for (uint32_t i = tid; i < kRayCounterWords; i += gridDim.x * blockDim.x) f.ray_counter[i] = 0u;
    if (tid < f.R) {
        V3 d = sphericalFibonacciSample(tid, f.R);
        f.fib[tid] = make_float4(d.x, d.y, d.z, 0.0f);
        // traversal order: position tid traces sample order[tid] (w = sample index)
        const uint32_t sample = f.order[tid];
        V3 e = sphericalFibonacciSample(sample, f.R);
        f.fib_order[tid] = make_float4(e.x, e.y, e.z, __uint_as_float(sample));
    }
    if (tid >= f.window) return;
    const uint32_t probeIdx = (tid + f.first) % N;
    const uint32_t z0 = f.sharded ? static_cast<uint32_t>(f.slab_z0) : 0u, z1 = f.sharded ? static_cast<uint32_t>(f.slab_z1) : Z;
    if (f.sharded && !inSlab(f, probeIdx)) return;
    const uint32_t slot = f.sharded ? slabRankOf(X, Y, Z, z0, z1, f.first, tid) : tid;
    writeSlot(f, slot, probeIdx);
    if (f.slot_order)
        const_cast<uint32_t*>(f.slot_order)[slotQueuePos(X, Y, Z, z0, max(1u, z1 - z0), f.first, f.window, tid, probeIdx)] = slot;
}

// ---------------------------------------------------------------------------
// 2. k_trace's source: the probe rays
// ---------------------------------------------------------------------------
// ProbeRays (the Src contract: ddgi_trace_kernels.h): the window's probe rays from
// the slot table (raygen.rgen:35-92: opaque pass then masked pass, tmin 1e-4, tmax
// zFar), partitions of whole probes.
struct ProbeRays {
    static constexpr bool kAllClasses = false;
    static constexpr bool kMaskedPass = true;
    static constexpr bool kSeeds = true;
    static constexpr float kTmin = 0.0001f;
    __device__ static void grab(const FrameArgs& f, uint32_t home, uint32_t lane, uint32_t& tried, uint32_t& b, uint32_t& e, uint32_t chunk)
    {
        grabRaysWave(f, f.ray_counter, home, lane, tried, b, e, chunk);
    }
    __device__ static PoolRec stage(const SceneArgs& sc, const FrameArgs& f, uint32_t r)
    {
        const uint32_t qp = r / f.R;
        const uint32_t slot = slotAt(f, qp);
        const float4 fv = f.fib_order[r - qp * f.R]; // (direction, sample index)
        const GpuProbeSlot ps = f.slots[slot];
        PoolRec rec;
        rec.o = { ps.pos[0], ps.pos[1], ps.pos[2] };
        rec.d = rotate(v3(fv.x, fv.y, fv.z), v3(ps.axis[0], ps.axis[1], ps.axis[2]), ps.angle_sin, ps.angle_cos);
        rec.a = slot * f.R + __float_as_uint(fv.w); // hit record index
        rec.c = seed::kNone;
        if (f.seed_cache) {
            const uint32_t w = f.seed_cache[static_cast<size_t>(ps.probe_index) * seed::kProbeWords + seed::texelOf(rec.d.x, rec.d.y, rec.d.z)];
            if (seed::candidateOk(w, sc.opaque_tri_first, sc.opaque_tri_end)) rec.c = w;
        }
        return rec;
    }
    __device__ static void take(const FrameArgs& f, uint32_t r, uint32_t recA, uint32_t& ray, float& tmax)
    {
        ray = recA;
        tmax = f.z_far;
    }
};

// ---------------------------------------------------------------------------
// 3. shading
// ---------------------------------------------------------------------------
// k_shade takes chunks of kShadeChunk consecutive probe rays. Misses and backface
// hits are finished in a classify pass; front hits are compacted into an LDS list
// and shaded densely (material, textures, BRDF per lit light, DDGI indirect). The
// shadow rays were traced before (k_shadow_gen + k_trace_shadow; the sun-only schedule's
// instances below resolve or defer the sun's ray themselves), and their per-ray light bits say
// which lit lights are occluded: base (+ T or Z per lit light, in light order) +
// indirect, the IEEE sequence of the single-pass closest-hit shader
// (opaque.rchit:105-176 with traceShadowRay's shadowFactor 1 or 0).
// MODE, the schedule (shade_schedule.h):
//  kShadeListed    every lit light's shadow ray was listed by k_shadow_gen and traced before
//                  this launch; shadow_bits holds the occluded bits.
//  kShadeSunFused  pass 1 of the sun-only schedule (one light, the sun, with its cover map;
//                  no k_shadow_gen): phase B resolves the sun's ray of a front hit itself,
//                  with the generator's functions and operand order (genHitPoint<false>:
//                  origin + T * dir, sunMapVerdict), so the verdict is the same bits.
//                  Occluded or lit: shaded at once, shadow_bits untouched. Undecided: the
//                  surfel is left to the deferred pass - shadow_bits[ray] = the lit mask and
//                  the ray joins an LDS list, which the block appends to the shadow-ray list
//                  (the sun's own with a light-space BVH) after one global atomic per chunk
//                  (a per-wave atomic on that counter serialises at L2, see k_shadow_gen).
//                  List order is free: any-hit bits are ORed, surfels are independent.
//                  The cover-map gather sits late, after the surface's texture fetches: issued
//                  beside them it held the light-space coordinates and the texel across the
//                  fetches, and the kernel has no register to spare at 4 waves per SIMD.
//  kShadeDeferred  pass 2, after k_trace_shadow: a fixed grid strides over that list (count
//                  read here) and shades each owner ray with its traced bit.
// The counting variant of pass 1 keeps k_shadow_gen's cover_counts and writes shadow_bits of
// every front hit as the generator did (k_sun_points reads them back).
constexpr int kShadeListed = 0, kShadeSunFused = 1, kShadeDeferred = 2;

template<bool COUNT, int WPE, int MODE = kShadeListed>
__global__ void __launch_bounds__(kShadeBlock) __attribute__((amdgpu_waves_per_eu(WPE))) k_shade(SceneArgs sc, FrameArgs f)
{
    if (frameAborted(f.abort_word)) return;
    // compacted front hits (ray index) from the start, misses from the end
    __shared__ uint32_t listA[kShadeChunk];
    // kShadeSunFused: the chunk's undecided front hits (ray index)
    __shared__ uint32_t listD[MODE == kShadeSunFused ? kShadeChunk : 1];
    __shared__ uint32_t counts[6];          // [0] front hits, [1] misses, [2,3] chunk, [4] deferred, [5] their list base
    uint32_t cFront = 0, cOccluded = 0, cLit = 0, cListed = 0;
    (void)listD; (void)cOccluded; (void)cLit; (void)cListed;
    // the spot lights, read once per workgroup: per front hit and lit spot they were a
    // dependent 96-B read ahead of the IES lookup (C5: k_shade 2.06 -> 1.97 ms, +1.2 %;
    // profiles/r04_s_shade_spots_lds.log)
    constexpr bool kSpots = MODE == kShadeListed; // (the sun-only schedule: the sun is the only light)
    __shared__ GpuSpotLight spotsL[kSpots ? kMaxLights - 1 : 1];
    if constexpr (kSpots) {
        const uint32_t words = static_cast<uint32_t>(sc.spot_count) * static_cast<uint32_t>(sizeof(GpuSpotLight) / 4u);
        for (uint32_t i = threadIdx.x; i < words; i += kShadeBlock)
            reinterpret_cast<uint32_t*>(spotsL)[i] = reinterpret_cast<const uint32_t*>(sc.spots)[i];
        __syncthreads();
    }

    if constexpr (MODE == kShadeDeferred) {
        const uint32_t total = f.sun_rays ? *f.sun_count : *f.shadow_count;
        const ShadowRay* const list = f.sun_rays ? f.sun_rays : f.shadow_rays;
        for (uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x; i < total; i += gridDim.x * kShadeBlock) {
            const uint32_t ray = __float_as_uint(list[i].dir_owner.w) >> 4;
            FrontSurface sf;
            frontSurface<kSpots>(sc, f, spotsL, ray, sf);
            shadeFront<kSpots>(sc, f, spotsL, ray, sf, f.shadow_bits[ray] >> 16);
        }
        return;
    }

    // chunks come from the second set of per-XCD partition heads (see grabRays)
    uint32_t* heads = f.ray_counter + kRayParts * kRayCounterStride;
    const uint32_t home = xccId();
    uint32_t tried = 0;
    for (;;) {
        if (threadIdx.x == 0) {
            uint32_t b, e;
            grabRays(f, heads, home, tried, b, e, static_cast<uint32_t>(kShadeChunk));
            counts[0] = 0;
            counts[1] = 0;
            counts[2] = b;
            counts[3] = e;
            if (MODE == kShadeSunFused) counts[4] = 0;
        }
        __syncthreads();
        const uint32_t chunk = counts[2], chunkEnd = counts[3];
        if (chunk >= chunkEnd) break;
        // ---- A. classify: backfaces finish here; front hits and misses are listed -
        // (a miss's environment lookup - atan2, acos, a texture sample - runs densely in
        // C below: inline, the few misses of a chunk made most of its waves run it)
        for (uint32_t r = threadIdx.x; r < kShadeChunk; r += kShadeBlock) {
            if (chunk + r >= chunkEnd) break;
            const uint32_t q = (chunk + r) / f.R;
            const uint32_t ray = slotAt(f, q) * f.R + (chunk + r - q * f.R);
            const GpuHit hit = f.hits[ray];
            if (hit.tri == kNoHit) {
                const uint32_t k = atomicAdd(&counts[1], 1u);
                listA[kShadeChunk - 1u - k] = ray;
            } else if (hit.t < 0.0f) {
                // backface: colour 0, depth x 0.2 (raygen.rgen:129-134); the closest-hit
                // colour and the indirect term are overwritten, so they are not evaluated.
                storeSurfel(f, ray, splat(0.0f), hit.t * 0.2f);
            } else {
                const uint32_t k = atomicAdd(&counts[0], 1u);
                listA[k] = ray;
            }
        }
        __syncthreads();
        const uint32_t nA = counts[0];
        // ---- B. dense surface shading of front hits -----------------------------
        for (uint32_t k0 = 0; k0 < nA; k0 += kShadeBlock) {
            const uint32_t kk = k0 + threadIdx.x;
            const bool valid = kk < nA;
            const uint32_t ray = valid ? listA[kk] : 0u;
            FrontSurface sf { splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u };
            if (valid) {
                if (COUNT) cFront++;
                frontSurface<kSpots>(sc, f, spotsL, ray, sf);
            }
            if (!valid) continue;
            uint32_t occ = 0u;
            if constexpr (MODE == kShadeSunFused) {
                // the sun (the only light, bit 0) by its cover map
                int vd = cover::kLit;
                if (sf.need) {
                    vd = sunMapVerdict(sc, sf.origin + sf.T * sf.dir);
                    if (COUNT) {
                        cOccluded += vd == cover::kOccluded;
                        cLit += vd == cover::kLit;
                        cListed += vd == cover::kUndecided;
                    }
                }
                if (COUNT || vd == cover::kUndecided) f.shadow_bits[ray] = sf.need | (vd == cover::kOccluded ? 1u << 16 : 0u);
                if (vd == cover::kUndecided) {
                    listD[atomicAdd(&counts[4], 1u)] = ray;
                    continue;
                }
                occ = vd == cover::kOccluded ? 1u : 0u;
            } else {
                occ = sf.need ? f.shadow_bits[ray] >> 16 : 0u;
            }
            shadeFront<kSpots>(sc, f, spotsL, ray, sf, occ);
        }
        // ---- C. misses (raygen.rgen:70-79) ------------------------------------------
        const uint32_t nM = counts[1];
        for (uint32_t k = threadIdx.x; k < nM; k += kShadeBlock) {
            const uint32_t ray = listA[kShadeChunk - 1u - k];
            V3 origin, dir;
            rayOf(f, ray, &origin, &dir);
            float u, v;
            sphericalUvFromDirection(dir, &u, &v);
            float4 c = sc.sample(sc.env_texture, u, v);
            storeSurfel(f, ray, f.environment_multiplier * v3(c.x, c.y, c.z), f.z_far);
        }
        __syncthreads();
        if constexpr (MODE == kShadeSunFused) {
            // the chunk's undecided rays to the shadow-ray list, as k_shadow_gen built them
            const uint32_t nD = counts[4];
            if (nD != 0) {
                if (threadIdx.x == 0) counts[5] = atomicAdd(f.sun_rays ? f.sun_count : f.shadow_count, nD);
                __syncthreads();
                ShadowRay* const list = (f.sun_rays ? f.sun_rays : f.shadow_rays) + counts[5];
                for (uint32_t i = threadIdx.x; i < nD; i += kShadeBlock) {
                    const uint32_t ray = listD[i];
                    const V3 hitPoint = genHitPoint<false>(f, ray, f.hits[ray].t);
                    V3 ld;
                    float tmax;
                    shadowRayOf(sc, f.z_far, 0u, hitPoint, &ld, &tmax);
                    list[i] = ShadowRay { make_float4(hitPoint.x, hitPoint.y, hitPoint.z, tmax), make_float4(ld.x, ld.y, ld.z, __uint_as_float((ray << 4) | 0u)) };
                }
                __syncthreads(); // before thread 0 resets the counts
            }
        }
    }
    if (COUNT) atomicAdd(&f.counters[6], static_cast<unsigned long long>(cFront));
    if (COUNT && MODE == kShadeSunFused && f.cover_counts) {
        atomicAdd(&f.cover_counts[0], cOccluded);
        atomicAdd(&f.cover_counts[1], cLit);
        atomicAdd(&f.cover_counts[2], cListed);
    }
}

// ---------------------------------------------------------------------------
// 4. debug read-back, frame sequencing, fills
// ---------------------------------------------------------------------------
// ark_ddgi_debug_sun_cover_counts: the origin of every sun shadow ray of the update `f`
// was (queue position order; w = 1, else zeros: no front hit, or the sun not lit there)
__global__ void __launch_bounds__(256) k_sun_points(FrameArgs f, float4* __restrict__ out)
{
    const uint32_t pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= f.window_rays) return;
    const uint32_t q = pos / f.R;
    const uint32_t ray = slotAt(f, q) * f.R + (pos - q * f.R);
    const GpuHit h = f.hits[ray];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (h.tri != kNoHit && !(h.t < 0.0f) && (f.shadow_bits[ray] & 1u)) {
        const V3 X = genHitPoint<false>(f, ray, h.t);
        o = make_float4(X.x, X.y, X.z, 1.0f);
    }
    out[pos] = o;
}

// Frame sequencing between a context's two streams (ddgi_frame.cpp, frame_book.h): the
// producer stream ends its part of frame n with k_seq_signal (word = n, a release
// store after the kernels before it on that stream), the consumer stream starts with
// k_seq_wait (one wave polls the word with acquire loads until it reaches n). A
// cross-queue event wait costs 12-16 us of queue latency per frame, satisfied or not
// (profiles/r03_v, r03_w); this pair costs two one-wave launches. Every wait ends:
// the word is written by work enqueued earlier on the other stream, which nothing
// blocks - unless something serialises the queues (a counter-collecting profiler
// runs one kernel at a time: the wait can then be scheduled ahead of its signal).
// The wait therefore fails closed: after timeout_ticks of the wall clock (or at once
// when an earlier wait of the context already gave up) it sets *timed_out, which
// every kernel of the path checks at entry (frameAborted: the frame's remaining
// launches leave their outputs untouched), and the host-mapped *host_flag, which the
// context's next call polls (ddgi_frame.cpp checkSequencing: ARK_DDGI_E_DEVICE, then
// event sequencing). Signals are never skipped, so the sequence words stay in step.
__global__ void __launch_bounds__(64) k_seq_signal(uint32_t* word, uint32_t value)
{
    if (threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(64) k_seq_wait(const uint32_t* word, uint32_t value, uint32_t* timed_out, uint32_t* host_flag, uint64_t timeout_ticks)
{
    if (threadIdx.x != 0) return;
    const uint64_t t0 = wall_clock64();
    while (static_cast<int32_t>(__hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - value) < 0) {
        if (wall_clock64() - t0 > timeout_ticks || __hip_atomic_load(timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
            __hip_atomic_store(timed_out, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (host_flag) __hip_atomic_store(host_flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// Atlas clears (DDGINode.cpp:50-55) as 32-bit fills.
__global__ void k_fill_u32(uint32_t* __restrict__ p, uint64_t n, uint32_t value)
{
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        p[i] = value;
}

} // namespace dev

// ---------------------------------------------------------------------------
// 5. launchers
// ---------------------------------------------------------------------------
hipError_t launch_probe_slots(const FrameArgs& f, hipStream_t s)
{
    const uint32_t n = f.window > f.R ? f.window : f.R;
    hipLaunchKernelGGL(dev::k_probe_slots, dim3((n + 255u) / 256u), dim3(256), 0, s, f);
    return hipGetLastError();
}

const void* kernel_trace_ptr(bool count)
{
    return count ? reinterpret_cast<const void*>(&dev::k_trace<true, 1, dev::ProbeRays>) : reinterpret_cast<const void*>(&dev::k_trace<false, dev::kTraceWpe, dev::ProbeRays>);
}

// A launch whose chunks are at most 32 rays (the half-occupancy windows) runs the
// instance with 32-slot pools: 4 KB less LDS per workgroup for the kernels beside it.
hipError_t launch_trace(const SceneArgs& sc, const FrameArgs& f, uint32_t blocks, bool count, hipStream_t s)
{
    void* args[] = { const_cast<SceneArgs*>(&sc), const_cast<FrameArgs*>(&f) };
    const bool small = !count && f.grab_chunk <= 32u;
    const void* fn = kernel_trace_ptr(count);
    if (small) fn = reinterpret_cast<const void*>(&dev::k_trace<false, dev::kTraceWpe, dev::ProbeRays, 32>);
    if (f.seed_cache && !f.seed_offsets_write) {
        // the instances that write the seed cache themselves
        fn = count ? reinterpret_cast<const void*>(&dev::k_trace<true, 1, dev::ProbeRays, 64, true>)
             : small ? reinterpret_cast<const void*>(&dev::k_trace<false, dev::kTraceWpe, dev::ProbeRays, 32, true>)
                     : reinterpret_cast<const void*>(&dev::k_trace<false, dev::kTraceWpe, dev::ProbeRays, 64, true>);
    }
    return hipLaunchKernel(fn, dim3(blocks), dim3(kTraceBlock), args, 0, s);
}

// Co-resident workgroups of a persistent kernel on this device (cached per kernel).
static uint32_t persistentBlocks(const void* fn, int block, uint32_t fallback)
{
    static thread_local std::vector<std::pair<const void*, uint32_t>> cache;
    for (const auto& c : cache)
        if (c.first == fn) return c.second;
    int dev = 0, cus = 0, occ = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, block, 0) != hipSuccess || occ <= 0 || cus <= 0)
        return fallback;
    cache.emplace_back(fn, static_cast<uint32_t>(occ * cus));
    return cache.back().second;
}

// One-pass shading at <= 128 VGPRs, 4 waves/SIMD, no spill (round 1: 0.57 -> 0.50 ms
// at C4 against the compiler's 133 VGPRs, 3 waves). Round 3: 5 waves (96 VGPRs)
// spills 30 and shades in 0.525 instead of 0.469 ms (profiles/r03_ak).
constexpr int kShadeWpe = 4;
// sunFused: pass 1 of the sun-only schedule (shade_schedule.h), which resolves the sun's ray
// itself and lists the undecided ones; launch_shade_deferred follows their traversal.
hipError_t launch_shade(const SceneArgs& sc, const FrameArgs& f, uint32_t blocks, bool count, hipStream_t s, bool sunFused)
{
    if (sunFused && (f.light_count != 1u || !sc.has_sun || sc.sun_map == nullptr)) return hipErrorInvalidValue;
    void* args[] = { const_cast<SceneArgs*>(&sc), const_cast<FrameArgs*>(&f) };
    const void* fn;
    if (count) {
        fn = sunFused ? reinterpret_cast<const void*>(&dev::k_shade<true, 1, dev::kShadeSunFused>) : reinterpret_cast<const void*>(&dev::k_shade<true, 1>);
    } else {
        fn = sunFused ? reinterpret_cast<const void*>(&dev::k_shade<false, kShadeWpe, dev::kShadeSunFused>)
                      : reinterpret_cast<const void*>(&dev::k_shade<false, kShadeWpe>);
        blocks = persistentBlocks(fn, kShadeBlock, blocks);
    }
    return hipLaunchKernel(fn, dim3(blocks), dim3(kShadeBlock), args, 0, s);
}

// Pass 2 of the sun-only schedule: the listed rays' surfels, a fixed grid striding over
// the list (its count is read on the device; C4 lists ~97 K of 8.4 M rays).
constexpr uint32_t kDeferredBlocks = 512;
hipError_t launch_shade_deferred(const SceneArgs& sc, const FrameArgs& f, hipStream_t s)
{
    hipLaunchKernelGGL((dev::k_shade<false, kShadeWpe, dev::kShadeDeferred>), dim3(kDeferredBlocks), dim3(kShadeBlock), 0, s, sc, f);
    return hipGetLastError();
}

// One launch: the sun's list through the light-space BVH (when k_shadow_gen split it
// off; then the other lights' list in the same launch, kShadowSunWorld), or every
// shadow ray through the world BVHs.
hipError_t launch_trace_shadow(const SceneArgs& sc, const FrameArgs& f, uint32_t blocks, bool count, hipStream_t s)
{
    void* args[] = { const_cast<SceneArgs*>(&sc), const_cast<FrameArgs*>(&f) };
    const void* fn = kernel_trace_shadow_ptr(count);
    if (f.sun_rays && f.light_count <= 1u)
        fn = count ? reinterpret_cast<const void*>(&dev::k_trace_shadow<true, 1, dev::kShadowSun>)
                   : reinterpret_cast<const void*>(&dev::k_trace_shadow<false, dev::kShadowWpe, dev::kShadowSun>);
    else if (f.sun_rays)
        fn = count ? reinterpret_cast<const void*>(&dev::k_trace_shadow<true, 1, dev::kShadowSunWorld>)
                   : reinterpret_cast<const void*>(&dev::k_trace_shadow<false, dev::kShadowWpe, dev::kShadowSunWorld>);
    return hipLaunchKernel(fn, dim3(blocks), dim3(kTraceBlock), args, 0, s);
}

hipError_t launch_shadow_gen(const SceneArgs& sc, const FrameArgs& f, hipStream_t s)
{
    const uint32_t blocks = (f.window_rays + dev::kGenSpan - 1u) / dev::kGenSpan;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_shadow_gen<false>, dim3(blocks), dim3(256), 0, s, sc, f);
    return hipGetLastError();
}

hipError_t launch_sun_points(const FrameArgs& f, float4* out, hipStream_t s)
{
    if (f.window_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(dev::k_sun_points, dim3((f.window_rays + 255u) / 256u), dim3(256), 0, s, f, out);
    return hipGetLastError();
}

hipError_t launch_seq_signal(uint32_t* word, uint32_t value, hipStream_t s)
{
    hipLaunchKernelGGL(dev::k_seq_signal, dim3(1), dim3(64), 0, s, word, value);
    return hipGetLastError();
}

hipError_t launch_seq_wait(const uint32_t* word, uint32_t value, uint32_t* timedOut, uint32_t* hostFlag, uint64_t timeoutTicks, hipStream_t s)
{
    hipLaunchKernelGGL(dev::k_seq_wait, dim3(1), dim3(64), 0, s, word, value, timedOut, hostFlag, timeoutTicks);
    return hipGetLastError();
}

hipError_t launch_fill_u32(void* p, uint64_t count, uint32_t value, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    uint64_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dev::k_fill_u32, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, s, static_cast<uint32_t*>(p), count, value);
    return hipGetLastError();
}

const void* kernel_shade_ptr(bool count)
{
    return count ? reinterpret_cast<const void*>(&dev::k_shade<true, 1>) : reinterpret_cast<const void*>(&dev::k_shade<false, kShadeWpe>);
}

const void* kernel_trace_shadow_ptr(bool count)
{
    return count ? reinterpret_cast<const void*>(&dev::k_trace_shadow<true, 1>) : reinterpret_cast<const void*>(&dev::k_trace_shadow<false, dev::kShadowWpe>);
}

} // namespace ark
