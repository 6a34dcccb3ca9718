// shade_schedule.h — which shading schedule an update runs (ddgi_frame.cpp: callerPart). Pure
// host logic over plain values: no device call, so that the decision is tested on the CPU
// (tests/cpp/shade_schedule_test.cpp).
#pragma once

#include <cstdint>

#include "../../include/ark_ddgi.h"

namespace ark {

// Listed:  k_shadow_gen lists every lit light's shadow ray, k_trace_shadow traces the
//          list, k_shade shades every surfel with the traced bits.
// SunOnly: k_shade resolves the sun's ray from the cover map itself and shades at once;
//          the rays the map leaves undecided are listed by k_shade, traced, and shaded by
//          a second, deferred k_shade pass over that list. No k_shadow_gen.
enum class ShadeSchedule { Listed, SunOnly };

// What an update knows when it decides.
struct ShadeScheduleState {
    uint32_t lightCount = 0;    // the sun (if any) + the spot lights
    bool hasSun = false;
    bool coverMapInUse = false; // SceneArgs::sun_map != nullptr: valid for this geometry, sun direction and z_far
    uint32_t flags = 0;         // ArkDdgiDesc.flags
    // the update is a pipelined window whose traversal runs the half-occupancy grid (ddgi_context.h:
    // kPipeHalfRays): the previous frame's shading chain runs beside the next traversal
    bool halfOccupancyWindow = false;
    bool sunOnlyInSmallWindows = false; // ark_ddgi_debug_set_sun_only_small_windows (tests)
};

// SunOnly needs the sun as the only light (with a spot nearly every front hit has a lit
// light whose ray must be traced: deferral would cover them all), its cover map in use (a
// stale or dropped map, or ARK_DDGI_FLAG_NO_SUN_COVER_MAP, leave every sun ray to the
// traversal), and no ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE.
// A half-occupancy window keeps the generator schedule: there the chain is hidden beside the
// next frame's traversal, which leaves it half of every CU, so the generator's pass costs
// the frame nothing, while shading launched first, at the moment that traversal starts,
// lengthens the frame (C4 windows of 2,048 to 16,384 probes: + 7 % to + 2.5 %,
// EXPERIMENTS.md). With the full traversal grid the chain gets CUs only as traversal
// workgroups retire, and what it no longer does comes off the step (the whole C4 grid: - 6 %).
inline ShadeSchedule shadeScheduleOf(const ShadeScheduleState& q)
{
    if (q.flags & ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE) return ShadeSchedule::Listed;
    if (!q.hasSun || q.lightCount != 1u || !q.coverMapInUse) return ShadeSchedule::Listed;
    if (q.halfOccupancyWindow && !q.sunOnlyInSmallWindows) return ShadeSchedule::Listed;
    return ShadeSchedule::SunOnly;
}

} // namespace ark
