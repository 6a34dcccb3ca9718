// rt_shadows_host.h — the host side of the ray-traced local-light shadow masks
// (ark_ddgi_rt_local_shadows): the entry's argument checks and a serial restatement of the
// raygen (rt_shadows.h, the functions k_rtshadow_gen calls) whose rays are tested against
// every triangle record by brute force. Host only, no HIP (also built on its own, tests/cpp).
#pragma once

#include <stdint.h>

#include "../../include/ark_ddgi.h"

namespace ark {
namespace rtshadow {

// What ark_ddgi_rt_local_shadows refuses about a descriptor of the right struct_size
// (null: nothing): no depth, light_count > 16, lights missing, a null or repeated out_mask,
// a non-finite light field or matrix, width * height >= 2^28 (the owner word is
// (pixel << 4) | light). The pointers are compared, never followed.
const char* descProblem(const ArkRtShadowsDesc& d);

// ArkRtShadowLight's eight floats in rt_shadows.h's order
inline void lightFloats(const ArkRtShadowLight& l, float out[8])
{
    for (int k = 0; k < 3; ++k) {
        out[k] = l.position[k];
        out[3 + k] = l.direction[k];
    }
    out[6] = l.outer_cone_angle_cos;
    out[7] = l.source_radius;
}

// The masks of `d` (depth and out_mask are host pointers here) over `nRecords` 48-byte
// triangle records (12 words: v0, e1, e2, instance, primitive, flip; instance 0xffffffff is
// a hole). classOf[instance] = hit-mask class 0 opaque, 1 masked, 2 translucent; bit c of
// classMask: class c occludes. The triangle test is the kernels' Möller–Trumbore
// (intersectTri: crossFma / dotFma3, 1 / det) in [0.025, tmax]; a ray with
// !(tmax >= 0.025) is not traced and is lit. counts[4 * light + k]: k = 0 sky, 1 outside
// the cone, 2 lit, 3 occluded. Returns 0, or -1 for what descProblem refuses.
int hostShadows(const uint32_t* records, uint64_t nRecords, const int32_t* classOf, uint64_t nInstances, uint32_t classMask, const ArkRtShadowsDesc& d,
                uint64_t* counts);

} // namespace rtshadow
} // namespace ark
