// rt_shadows_host.cpp — see rt_shadows_host.h; at the end the host-only ark_ddgi_debug_rt_shadows_*
// entries (include/ark_ddgi_debug.h), which need nothing else of the library.
#include "rt_shadows_host.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/ark_ddgi_debug.h"
#include "rt_shadows.h"

namespace ark {
namespace rtshadow {

const char* descProblem(const ArkRtShadowsDesc& d)
{
    if (d.light_count > ARK_RT_SHADOWS_MAX_LIGHTS) return "more than ARK_RT_SHADOWS_MAX_LIGHTS lights";
    if (static_cast<uint64_t>(d.width) * d.height >= (1ull << 28)) return "target too large: the owner word is (pixel << 4) | light";
    if (!d.depth) return "no depth plane";
    if (d.light_count && !d.lights) return "no lights array";
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(d.world_from_view[k]) || !std::isfinite(d.view_from_projection[k])) return "non-finite camera matrix";
    for (uint32_t l = 0; l < d.light_count; ++l) {
        float v[8];
        lightFloats(d.lights[l], v);
        for (float x : v)
            if (!std::isfinite(x)) return "non-finite light field";
        if (!d.lights[l].out_mask) return "null out_mask";
        for (uint32_t m = 0; m < l; ++m)
            if (d.lights[m].out_mask == d.lights[l].out_mask) return "repeated out_mask";
    }
    return nullptr;
}

namespace {

struct Tri {
    float v0[3], e1[3], e2[3];
};

// the kernels' Möller–Trumbore (shading_math.h intersectTri, ddgi_traversal.h), any hit in [tmin, tmax]
bool hits(const float o[3], const float d[3], float tmin, float tmax, const Tri& g)
{
    auto cr = [](const float* a, const float* b, float* c) {
        c[0] = std::fma(a[1], b[2], -(a[2] * b[1]));
        c[1] = std::fma(a[2], b[0], -(a[0] * b[2]));
        c[2] = std::fma(a[0], b[1], -(a[1] * b[0]));
    };
    auto dt = [](const float* a, const float* b) { return std::fma(a[0], b[0], std::fma(a[1], b[1], a[2] * b[2])); };
    float p[3], q[3];
    cr(d, g.e2, p);
    const float det = dt(g.e1, p);
    const float inv = 1.0f / det;
    const float s[3] = { o[0] - g.v0[0], o[1] - g.v0[1], o[2] - g.v0[2] };
    const float u = dt(s, p) * inv;
    cr(s, g.e1, q);
    const float v = dt(d, q) * inv;
    const float t = dt(g.e2, q) * inv;
    return (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t >= tmin) & (t <= tmax);
}

} // namespace

int hostShadows(const uint32_t* records, uint64_t nRecords, const int32_t* classOf, uint64_t nInstances, uint32_t classMask, const ArkRtShadowsDesc& d,
                uint64_t* counts)
{
    if (descProblem(d) || (nRecords && !records) || (nInstances && !classOf)) return -1;
    const uint32_t nl = d.light_count;
    if (counts) std::memset(counts, 0, sizeof(uint64_t) * 4 * nl);
    if (nl == 0 || d.width == 0 || d.height == 0) return 0;
    // the records of the occluding classes
    std::vector<Tri> tris;
    for (uint64_t i = 0; i < nRecords; ++i) {
        const uint32_t* w = records + 12 * i;
        const uint32_t inst = w[9];
        if (inst == 0xffffffffu || inst >= nInstances) continue; // a hole
        const int32_t c = classOf[inst];
        if (c < 0 || c > 2 || !((classMask >> c) & 1u)) continue;
        Tri t;
        std::memcpy(t.v0, w, 12);
        std::memcpy(t.e1, w + 3, 12);
        std::memcpy(t.e2, w + 6, 12);
        tris.push_back(t);
    }
    float lights[ARK_RT_SHADOWS_MAX_LIGHTS][8];
    for (uint32_t l = 0; l < nl; ++l) lightFloats(d.lights[l], lights[l]);
    float PW[16];
    mat4Mul(d.world_from_view, d.view_from_projection, PW);
    const uint32_t T = static_cast<uint32_t>(std::min<uint64_t>(8, std::max<uint32_t>(1, d.height / 8)));
    std::vector<uint64_t> part(static_cast<size_t>(T) * 4 * nl, 0);
    auto rows = [&](uint32_t t, uint32_t y0, uint32_t y1) {
        uint64_t* cnt = part.data() + static_cast<size_t>(t) * 4 * nl;
        for (uint32_t py = y0; py < y1; ++py)
            for (uint32_t px = 0; px < d.width; ++px) {
                const uint64_t p = static_cast<uint64_t>(py) * d.width + px;
                const float depth = d.depth[p];
                if (depth >= kSkyDepth) { // the reference returns: the cleared texel stays
                    for (uint32_t l = 0; l < nl; ++l) {
                        d.lights[l].out_mask[p] = 0;
                        cnt[4 * l]++;
                    }
                    continue;
                }
                float P[3], dx, dy;
                shadingPoint(PW, px, py, d.width, d.height, depth, P);
                uint32_t state = pixelSeed(d.frame_index, px, py);
                pointInDisk(state, &dx, &dy);
                for (uint32_t l = 0; l < nl; ++l) {
                    float L[3], tmax;
                    if (!lightRay(P, lights[l], dx, dy, L, &tmax)) {
                        d.lights[l].out_mask[p] = 0;
                        cnt[4 * l + 1]++;
                        continue;
                    }
                    bool occluded = false;
                    if (tmax >= kTmin)
                        for (const Tri& g : tris)
                            if (hits(P, L, kTmin, tmax, g)) {
                                occluded = true;
                                break;
                            }
                    d.lights[l].out_mask[p] = occluded ? 0 : 255;
                    cnt[4 * l + (occluded ? 3 : 2)]++;
                }
            }
    };
    if (T == 1) {
        rows(0, 0, d.height);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < T; ++t)
            pool.emplace_back(rows, t, static_cast<uint32_t>(static_cast<uint64_t>(d.height) * t / T), static_cast<uint32_t>(static_cast<uint64_t>(d.height) * (t + 1) / T));
        for (auto& th : pool) th.join();
    }
    if (counts)
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t k = 0; k < 4 * nl; ++k) counts[k] += part[static_cast<size_t>(t) * 4 * nl + k];
    return 0;
}

} // namespace rtshadow
} // namespace ark

// ark_ddgi_debug.h: the host-only entries of the restatement, no GPU
extern "C" int ark_ddgi_debug_rt_shadows_check_desc(const ArkRtShadowsDesc* desc)
{
    if (!desc || desc->struct_size != sizeof(ArkRtShadowsDesc)) return ARK_DDGI_E_INVALID_ARGUMENT;
    return ark::rtshadow::descProblem(*desc) ? ARK_DDGI_E_INVALID_ARGUMENT : ARK_DDGI_OK;
}

extern "C" int ark_ddgi_debug_rt_shadows_host(const uint32_t* records, uint64_t n_records, const int32_t* class_of, uint64_t n_instances, uint32_t class_mask,
                                               const ArkRtShadowsDesc* desc, uint64_t* counts)
{
    if (ark_ddgi_debug_rt_shadows_check_desc(desc) != ARK_DDGI_OK) return ARK_DDGI_E_INVALID_ARGUMENT;
    return ark::rtshadow::hostShadows(records, n_records, class_of, n_instances, class_mask, *desc, counts) == 0 ? ARK_DDGI_OK : ARK_DDGI_E_INVALID_ARGUMENT;
}

extern "C" int ark_ddgi_debug_rt_shadows_sample(uint32_t frame_index, uint32_t px, uint32_t py, uint32_t* out_state, float* out_disk)
{
    if (!out_state || !out_disk) return ARK_DDGI_E_INVALID_ARGUMENT;
    uint32_t state = ark::rtshadow::pixelSeed(frame_index, px, py);
    out_state[0] = state;
    out_state[1] = ark::rtshadow::randXorshift(state);
    out_state[2] = ark::rtshadow::randXorshift(out_state[1]);
    ark::rtshadow::pointInDisk(state, &out_disk[0], &out_disk[1]);
    return state == out_state[2] ? ARK_DDGI_OK : ARK_DDGI_E_DEVICE;
}

extern "C" int ark_ddgi_debug_rt_shadows_layout(uint32_t* out, int n)
{
    const uint32_t offsets[] = { offsetof(ArkRtShadowLight, direction), offsetof(ArkRtShadowLight, outer_cone_angle_cos), offsetof(ArkRtShadowLight, source_radius),
                                 offsetof(ArkRtShadowLight, out_mask), offsetof(ArkRtShadowsDesc, frame_index), offsetof(ArkRtShadowsDesc, world_from_view),
                                 offsetof(ArkRtShadowsDesc, view_from_projection), offsetof(ArkRtShadowsDesc, depth), offsetof(ArkRtShadowsDesc, lights),
                                 offsetof(ArkRtShadowsDesc, light_count), offsetof(ArkRtShadowsDesc, reserved) };
    const int m = static_cast<int>(sizeof(offsets) / sizeof(offsets[0]));
    if (!out) return 0;
    for (int i = 0; i < n && i < m; ++i) out[i] = offsets[i];
    return m < n ? m : n;
}
