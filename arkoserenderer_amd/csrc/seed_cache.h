// seed_cache.h — the probe rays' hit candidates (k_trace): per probe a small
// octahedral map direction -> triangle record, holding the opaque-pass hit of the last ray
// of that probe seen in the texel's directions. A new ray of the probe tests its texel's
// record before anything else (as its first pending triangle group), so that its node tests
// prune by a real hit distance from the root down. The record is only ever a candidate:
// the traversal's own triangle step tests it, and the closest hit does not depend on the
// order in which triangles are met.
//
// What the kernels, the host (tests, the reset) and the simulator share: the texel of a
// direction and the rule for which words may be tested at all.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ARK_SEED_FN __host__ __device__ inline
#else
#define ARK_SEED_FN inline
#endif

namespace ark {
namespace seed {

#ifndef ARK_SEED_TEXELS
// 16 x 16 texels per probe (1 KB): 13 % fewer traversal iterations per ray in steady state
// on the C4 soup; 24 x 24: 15 % at 2.25 x the memory (EXPERIMENTS.md)
#define ARK_SEED_TEXELS 16
#endif
constexpr uint32_t kTexels = ARK_SEED_TEXELS;      // T: texels along one side
constexpr uint32_t kProbeWords = kTexels * kTexels; // words per probe
constexpr uint32_t kNone = 0xffffffffu;             // no candidate

// Texel in [0, T * T) of a direction (any length; zero and non-finite ones land in a fixed
// texel): the octahedral map of the atlases, cut into T x T cells. Any fixed mapping would
// do - it only chooses which earlier ray's hit a ray is offered.
// (texels: T, for the simulator's sweeps over map sizes; the kernels' is kTexels)
ARK_SEED_FN uint32_t texelOfT(float x, float y, float z, uint32_t texels)
{
    const float ax = x < 0.0f ? -x : x, ay = y < 0.0f ? -y : y, az = z < 0.0f ? -z : z;
    const float n = ax + ay + az;
    const float inv = n > 0.0f ? 1.0f / n : 0.0f;
    float u = x * inv, v = y * inv;
    if (z < 0.0f) {
        const float au = u < 0.0f ? -u : u, av = v < 0.0f ? -v : v;
        const float fu = (1.0f - av) * (u < 0.0f ? -1.0f : 1.0f);
        const float fv = (1.0f - au) * (v < 0.0f ? -1.0f : 1.0f);
        u = fu;
        v = fv;
    }
    const float T = static_cast<float>(texels);
    const float fx = (u * 0.5f + 0.5f) * T, fy = (v * 0.5f + 0.5f) * T;
    // (comparisons that a NaN fails on both sides: texel 0)
    const uint32_t ix = fx > 0.0f ? (fx < T ? static_cast<uint32_t>(fx) : texels - 1u) : 0u;
    const uint32_t iy = fy > 0.0f ? (fy < T ? static_cast<uint32_t>(fy) : texels - 1u) : 0u;
    return iy * texels + ix;
}

ARK_SEED_FN uint32_t texelOf(float x, float y, float z) { return texelOfT(x, y, z, kTexels); }

// Whether a cache word may be tested by pass 0 of a launch over the world BVHs whose
// opaque class owns the records [first, end) (SceneArgs::opaque_tri_first / _end): only
// records of that class. A masked-class record tested in pass 0 would skip the alpha
// test; an index past the array would read outside it. kNone is never in range.
ARK_SEED_FN bool candidateOk(uint32_t word, uint32_t first, uint32_t end)
{
    return word >= first && word < end;
}

} // namespace seed
} // namespace ark
