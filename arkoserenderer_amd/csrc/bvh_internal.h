// bvh_internal.h — what the host BVH sources share besides their public headers: the box
// type, bvh_builder.cpp's node writer and child-box inflation (lbvh_host.cpp restates the device
// build with them). Only bvh_builder.cpp, lbvh_host.cpp and bvh8_check.cpp include it.
#pragma once

#include <algorithm>
#include <cmath>

#include "ddgi_types.h"

namespace ark {

struct Aabb {
    float lo[3] = { INFINITY, INFINITY, INFINITY };
    float hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    void grow(const float p[3])
    {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], p[a]);
            hi[a] = std::max(hi[a], p[a]);
        }
    }
    void grow(const Aabb& b)
    {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], b.lo[a]);
            hi[a] = std::max(hi[a], b.hi[a]);
        }
    }
    float area() const
    {
        float d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
        if (!(d0 >= 0.0f)) return 0.0f;
        return 2.0f * (d0 * d1 + d1 * d2 + d2 * d0);
    }
    // SAH surface with per-face weights w = {xy, yz, zx} (BvhBuildOptions::area_w):
    // {1, 1, 1} is the surface area; rays parallel to z (the light-space BVH of the
    // sun's shadow rays) cross a box with a probability proportional to its xy face
    float area(const float* w) const
    {
        float d0 = hi[0] - lo[0], d1 = hi[1] - lo[1], d2 = hi[2] - lo[2];
        if (!(d0 >= 0.0f)) return 0.0f;
        return 2.0f * (w[0] * d0 * d1 + w[1] * d1 * d2 + w[2] * d2 * d0);
    }
};

// The node writer: the quantization grid of a node over `box` (p, e) and the
// outward-rounded planes of its slots' boxes (null: an unused slot, left as it is)
void writeNodePlanes(GpuBvh8Node& nd, const Aabb& box, const Aabb* const slotBox[8]);

// The builder's inflation of a child box (k_refit_nodes inflateBox)
void inflateChildBox(Aabb& b, float inflateAbs);

// the vertices Möller-Trumbore tests: v0, v0 + e1, v0 + e2
inline void recordVertices(const GpuTriangle& g, float v[3][3])
{
    const float e1[3] = { g.t0[3], g.t1[0], g.t1[1] }, e2[3] = { g.t1[2], g.t1[3], g.t2[0] };
    for (int a = 0; a < 3; ++a) {
        v[0][a] = g.t0[a];
        v[1][a] = g.t0[a] + e1[a];
        v[2][a] = g.t0[a] + e2[a];
    }
}

} // namespace ark
