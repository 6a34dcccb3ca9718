// ddgi_sampling.h — the read side of the DDGI atlases (probeSampling.glsl): octahedral
// tile addressing, the linear atlas filter and the 8-probe lookup sampleDDGI, shared by
// k_shade, lighting compose, probe debug and the reflections' closest hit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddgi_device.h"
#include "ddgi_kernels.h"

namespace ark {
namespace dev {

// probeSampling.glsl:9-27
__device__ __forceinline__ void atlasSampleUV(const FrameArgs& f, int px, int py, int pz, V3 dir, int res, float invW, float invH, float* u, float* v)
{
    const int pad = ARK_DDGI_ATLAS_PADDING;
    int tileX = px + py * f.X, tileY = pz;
    int firstX = pad + tileX * (res + 2 * pad), firstY = pad + tileY * (res + 2 * pad);
    float ex, ey;
    octahedralEncode(dir, &ex, &ey);
    float tx = (ex * 0.5f + 0.5f) * static_cast<float>(res);
    float ty = (ey * 0.5f + 0.5f) * static_cast<float>(res);
    float ax = static_cast<float>(firstX) + tx, ay = static_cast<float>(firstY) + ty;
    *u = ax * invW;
    *v = ay * invH;
}

// Linear filter, clamp to edge, over an fp16 atlas (DDGINode.cpp:274).
template<int CH, int NOUT>
__device__ __forceinline__ void sampleAtlas(const uint16_t* __restrict__ atlas, int W, int H, float u, float v, float* out)
{
    float x = u * static_cast<float>(W) - 0.5f;
    float y = v * static_cast<float>(H) - 0.5f;
    float x0f = floorf_(x), y0f = floorf_(y);
    float fx = x - x0f, fy = y - y0f;
    int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
    int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
    int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    uint16_t q[4][CH];
    // one load per texel row when the two texels are adjacent (xb = xa + 1, i.e. not
    // clamped at the atlas edge): 16 B for RGBA16F, 8 B for RG16F, at the texel's
    // own (8 B / 4 B) alignment - the device handles the misaligned wide load
    // (tools/probe/unaligned_load.hip)
    auto loadRow = [&](int k, int yy) {
        const uint16_t* pa = atlas + (static_cast<size_t>(yy) * W + xa) * CH;
        const uint16_t* pb = atlas + (static_cast<size_t>(yy) * W + xb) * CH;
        if (CH == 4) {
            uint2 wa, wb;
            if (xb == xa + 1) {
                const uint4 w = *reinterpret_cast<const uint4*>(pa);
                wa = make_uint2(w.x, w.y);
                wb = make_uint2(w.z, w.w);
            } else {
                wa = *reinterpret_cast<const uint2*>(pa);
                wb = *reinterpret_cast<const uint2*>(pb);
            }
            q[k][0] = static_cast<uint16_t>(wa.x & 0xffffu);
            q[k][1] = static_cast<uint16_t>(wa.x >> 16);
            q[k][2 % CH] = static_cast<uint16_t>(wa.y & 0xffffu);
            q[k][3 % CH] = static_cast<uint16_t>(wa.y >> 16);
            q[k + 1][0] = static_cast<uint16_t>(wb.x & 0xffffu);
            q[k + 1][1] = static_cast<uint16_t>(wb.x >> 16);
            q[k + 1][2 % CH] = static_cast<uint16_t>(wb.y & 0xffffu);
            q[k + 1][3 % CH] = static_cast<uint16_t>(wb.y >> 16);
        } else {
            uint32_t wa, wb;
            if (xb == xa + 1) {
                const uint2 w = *reinterpret_cast<const uint2*>(pa);
                wa = w.x;
                wb = w.y;
            } else {
                wa = *reinterpret_cast<const uint32_t*>(pa);
                wb = *reinterpret_cast<const uint32_t*>(pb);
            }
            q[k][0] = static_cast<uint16_t>(wa & 0xffffu);
            q[k][1] = static_cast<uint16_t>(wa >> 16);
            q[k + 1][0] = static_cast<uint16_t>(wb & 0xffffu);
            q[k + 1][1] = static_cast<uint16_t>(wb >> 16);
        }
    };
    loadRow(0, ya); // q[0] = (xa, ya), q[1] = (xb, ya)
    loadRow(2, yb); // q[2] = (xa, yb), q[3] = (xb, yb)
    for (int c = 0; c < NOUT; ++c) {
        float t00 = f16_to_f32(q[0][c]), t10 = f16_to_f32(q[1][c]);
        float t01 = f16_to_f32(q[2][c]), t11 = f16_to_f32(q[3][c]);
        out[c] = lerpf(lerpf(t00, t10, fx), lerpf(t01, t11, fx), fy);
    }
}

// One bilinear tap of an fp16 atlas, split into fetch and filter so that the taps of
// several probes can be in flight at once. The two texels (xa, xb) of a row come
// from one wide load at texel m = min(xa, W - 2) (xb is xa or xa + 1, both in
// {m, m + 1}); `sel` says which half each one is. Same texels, weights and lerps as
// sampleAtlas.
template<int CH>
struct AtlasTap {
    using Row = typename std::conditional<CH == 4, uint4, uint2>::type;
    Row r0, r1; // rows ya, yb: texels (m, m + 1)
    float fx, fy;
    uint32_t sel; // bit 0: texel a is m + 1, bit 1: texel b is m + 1
};

template<int CH>
__device__ __forceinline__ AtlasTap<CH> atlasTap(const uint16_t* __restrict__ atlas, int W, int H, float u, float v)
{
    using Row = typename AtlasTap<CH>::Row;
    AtlasTap<CH> t;
    float x = u * static_cast<float>(W) - 0.5f;
    float y = v * static_cast<float>(H) - 0.5f;
    float x0f = floorf_(x), y0f = floorf_(y);
    t.fx = x - x0f;
    t.fy = y - y0f;
    int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
    int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
    int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
    const int m = min(xa, W - 2);
    t.sel = (xa != m ? 1u : 0u) | (xb != m ? 2u : 0u);
    t.r0 = *reinterpret_cast<const Row*>(atlas + (static_cast<size_t>(ya) * W + m) * CH);
    t.r1 = *reinterpret_cast<const Row*>(atlas + (static_cast<size_t>(yb) * W + m) * CH);
    return t;
}

template<int CH, int NOUT>
__device__ __forceinline__ void atlasFilter(const AtlasTap<CH>& t, float* out)
{
    uint16_t q[4][CH];
    auto split = [&](int k, const typename AtlasTap<CH>::Row& r) {
        if constexpr (CH == 4) {
            const uint2 lo = make_uint2(r.x, r.y), hi = make_uint2(r.z, r.w);
            const uint2 wa = (t.sel & 1u) ? hi : lo, wb = (t.sel & 2u) ? hi : lo;
            q[k][0] = static_cast<uint16_t>(wa.x & 0xffffu);
            q[k][1] = static_cast<uint16_t>(wa.x >> 16);
            q[k][2] = static_cast<uint16_t>(wa.y & 0xffffu);
            q[k][3] = static_cast<uint16_t>(wa.y >> 16);
            q[k + 1][0] = static_cast<uint16_t>(wb.x & 0xffffu);
            q[k + 1][1] = static_cast<uint16_t>(wb.x >> 16);
            q[k + 1][2] = static_cast<uint16_t>(wb.y & 0xffffu);
            q[k + 1][3] = static_cast<uint16_t>(wb.y >> 16);
        } else {
            const uint32_t wa = (t.sel & 1u) ? r.y : r.x, wb = (t.sel & 2u) ? r.y : r.x;
            q[k][0] = static_cast<uint16_t>(wa & 0xffffu);
            q[k][1] = static_cast<uint16_t>(wa >> 16);
            q[k + 1][0] = static_cast<uint16_t>(wb & 0xffffu);
            q[k + 1][1] = static_cast<uint16_t>(wb >> 16);
        }
    };
    split(0, t.r0); // q[0] = (xa, ya), q[1] = (xb, ya)
    split(2, t.r1); // q[2] = (xa, yb), q[3] = (xb, yb)
    for (int c = 0; c < NOUT; ++c) {
        float t00 = f16_to_f32(q[0][c]), t10 = f16_to_f32(q[1][c]);
        float t01 = f16_to_f32(q[2][c]), t11 = f16_to_f32(q[3][c]);
        out[c] = lerpf(lerpf(t00, t10, t.fx), lerpf(t01, t11, t.fx), t.fy);
    }
}

// probeSampling.glsl:64-163. The 8 cage probes in groups of GB whose visibility and
// irradiance taps are issued together before their weights are formed; every weight
// and sum is the same IEEE sequence as the per-probe loop, and the irradiance sums run
// in probe order. GB = 1 (kGatherBatch): 2 and 4 measured no faster on C4.
constexpr int kGatherBatch = 1;
template<int GB>
__device__ V3 sampleDDGI(const FrameArgs& f, V3 P, V3 N, V3 Vw)
{
    const V3 spacing = v3(f.spacing[0], f.spacing[1], f.spacing[2]);
    const V3 origin = v3(f.origin[0], f.origin[1], f.origin[2]);
    V3 rel = (P - origin) / spacing;
    int bx = min(max(static_cast<int>(rel.x), 0), f.X - 1);
    int by = min(max(static_cast<int>(rel.y), 0), f.Y - 1);
    int bz = min(max(static_cast<int>(rel.z), 0), f.Z - 1);
    V3 baseProbePos = origin + v3(static_cast<float>(bx), static_cast<float>(by), static_cast<float>(bz)) * spacing;
    V3 sumIrradiance = splat(0.0f);
    float sumWeight = 0.0f;
    V3 al = (P - baseProbePos) / spacing;
    V3 alpha = { clampf(al.x, 0.0f, 1.0f), clampf(al.y, 0.0f, 1.0f), clampf(al.z, 0.0f, 1.0f) };
    const float invWi = 1.0f / static_cast<float>(f.Wi), invHi = 1.0f / static_cast<float>(f.Hi);
    const float invWv = 1.0f / static_cast<float>(f.Wv), invHv = 1.0f / static_cast<float>(f.Hv);
    const float minDistanceBetweenProbes = fminf_(spacing.x, fminf_(spacing.y, spacing.z));
    const V3 nN = normalize(N);
    const float tunableShadowBias = 0.3f;
    const V3 selfShadowBias = (N * 0.2f + Vw * 0.8f) * (0.75f * minDistanceBetweenProbes) * tunableShadowBias;
    const V3 biasedPosition = P + selfShadowBias;
    auto probeOf = [&](int i, int& px, int& py, int& pz) {
        px = min(max(bx + (i & 1), 0), f.X - 1);
        py = min(max(by + ((i >> 1) & 1), 0), f.Y - 1);
        pz = min(max(bz + ((i >> 2) & 1), 0), f.Z - 1);
    };
    auto probePosOf = [&](int px, int py, int pz) {
        return origin + v3(static_cast<float>(px), static_cast<float>(py), static_cast<float>(pz)) * spacing;
    };
    // --- 4 probes at a time: visibility and irradiance taps issued together, then
    // the weights, then the sums in probe order -----------------------------------
#pragma unroll
    for (int h = 0; h < 8; h += GB) {
        AtlasTap<2> vt[GB];
        AtlasTap<4> it[GB];
#pragma unroll
        for (int j = 0; j < GB; ++j) {
            int px, py, pz;
            probeOf(h + j, px, py, pz);
            const V3 directionToProbe = normalize(probePosOf(px, py, pz) - biasedPosition);
            float u, v;
            atlasSampleUV(f, px, py, pz, -directionToProbe, ARK_DDGI_VISIBILITY_RES, invWv, invHv, &u, &v);
            vt[j] = atlasTap<2>(f.vis, f.Wv, f.Hv, u, v);
            atlasSampleUV(f, px, py, pz, nN, ARK_DDGI_IRRADIANCE_RES, invWi, invHi, &u, &v);
            it[j] = atlasTap<4>(f.irr, f.Wi, f.Hi, u, v);
        }
#pragma unroll
        for (int j = 0; j < GB; ++j) {
            const int i = h + j;
            int px, py, pz;
            probeOf(i, px, py, pz);
            const int ox = i & 1, oy = (i >> 1) & 1, oz = (i >> 2) & 1;
            V3 tri = { fmaxf_(0.001f, mixf(1.0f - alpha.x, alpha.x, static_cast<float>(ox))),
                       fmaxf_(0.001f, mixf(1.0f - alpha.y, alpha.y, static_cast<float>(oy))),
                       fmaxf_(0.001f, mixf(1.0f - alpha.z, alpha.z, static_cast<float>(oz))) };
            float trilinearWeight = tri.x * tri.y * tri.z;
            float weight = 1.0f;
            const V3 probePos = probePosOf(px, py, pz);
            const V3 pointToProbe = probePos - biasedPosition;
            V3 unbiasedDirectionToProbe = normalize(probePos - P);
            const float smoothFloor = 0.02f, additionalSmoothening = 0.25f;
            weight *= smoothFloor + (1.0f - smoothFloor) * powf_(saturate(dot(unbiasedDirectionToProbe, N)), additionalSmoothening);
            {
                float vis[2];
                atlasFilter<2, 2>(vt[j], vis);
                float meanDistanceToOccluder = vis[0];
                float variance = fabsf_(vis[1] - square(vis[0]));
                float distToProbe = length(pointToProbe);
                float chebychevWeight = 1.0f;
                if (distToProbe > meanDistanceToOccluder) {
                    chebychevWeight = variance / (variance + square(distToProbe - meanDistanceToOccluder));
                    chebychevWeight = chebychevWeight * chebychevWeight * chebychevWeight;
                }
                chebychevWeight = fmaxf_(0.05f, chebychevWeight);
                weight *= chebychevWeight;
            }
            weight = fmaxf_(0.000001f, weight);
            const float crushThreshold = 0.2f;
            if (weight < crushThreshold) weight *= square(weight) * (1.0f / square(crushThreshold));
            weight *= trilinearWeight;
            float irr[3];
            atlasFilter<4, 3>(it[j], irr);
            // pow(irradiance, 0.5 * DDGI_IRRADIANCE_GAMMA), powf_ per component and not pow3: in a
            // unit whose every pow3 call passes this one exponent the compiler specialises pow3
            // for it before inlining (interprocedural constant propagation) and orders the
            // decode's instructions differently than in a unit that also holds k_probe_debug's
            // pow3(raw, 5) - the same values, but the code of k_shade would depend on which
            // kernels share its unit. powf_ is called with several exponents wherever this is.
            const float decodeExp = 5.0f * 0.5f;
            V3 probeIrradiance = { powf_(irr[0], decodeExp), powf_(irr[1], decodeExp), powf_(irr[2], decodeExp) };
            sumIrradiance = sumIrradiance + weight * probeIrradiance;
            sumWeight += weight;
        }
    }
    V3 irradiance = sumIrradiance / sumWeight;
    irradiance = irradiance * irradiance;
    irradiance = irradiance * (0.5f * kPi);
    return irradiance;
}

} // namespace dev
} // namespace ark
