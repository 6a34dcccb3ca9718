// shade_schedule_test.cpp — which shading schedule an update runs (shade_schedule.h:
// shadeScheduleOf) as a table of cases and as the exhaustive sweep of its inputs against the
// rule stated in the header. Stand-alone: built and run under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_shade_schedule.py. No GPU.
#include <cstdint>
#include <cstdio>

#include "shade_schedule.h"
#include "../../include/ark_ddgi.h"

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
            return 1;                                                       \
        }                                                                   \
    } while (0)

using namespace ark;
using S = ShadeSchedule;

namespace {

constexpr uint32_t kNoFused = ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE, kNoMap = ARK_DDGI_FLAG_NO_SUN_COVER_MAP;

S of(uint32_t lights, bool sun, bool map, uint32_t flags, bool half = false, bool small = false)
{
    ShadeScheduleState q;
    q.lightCount = lights;
    q.hasSun = sun;
    q.coverMapInUse = map;
    q.flags = flags;
    q.halfOccupancyWindow = half;
    q.sunOnlyInSmallWindows = small;
    return shadeScheduleOf(q);
}

int table()
{
    // the flagship: the sun alone, its map in use
    CHECK(of(1, true, true, 0) == S::SunOnly);
    // the flag keeps the generator schedule
    CHECK(of(1, true, true, kNoFused) == S::Listed);
    // a spot beside the sun, ten of them, a spot alone (one light, but no sun)
    CHECK(of(2, true, true, 0) == S::Listed);
    CHECK(of(11, true, true, 0) == S::Listed);
    CHECK(of(1, false, false, 0) == S::Listed);
    CHECK(of(1, false, true, 0) == S::Listed);
    // no light
    CHECK(of(0, false, false, 0) == S::Listed);
    // a stale or dropped map, or none wanted (the map is then never in use)
    CHECK(of(1, true, false, 0) == S::Listed);
    CHECK(of(1, true, false, kNoMap) == S::Listed);
    // flags that do not bear on shading leave the choice alone
    const uint32_t others = ARK_DDGI_FLAG_SERIAL_FRAMES | ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD | ARK_DDGI_FLAG_GPU_REBUILD | ARK_DDGI_FLAG_GPU_REBUILD_SUN |
                            ARK_DDGI_FLAG_GPU_REBUILD_SAH;
    CHECK(of(1, true, true, others) == S::SunOnly);
    CHECK(of(1, true, true, others | kNoFused) == S::Listed);
    // a pipelined window beside a half-occupancy traversal keeps the generator schedule,
    // unless the debug switch asks otherwise; the switch overrides nothing else
    CHECK(of(1, true, true, 0, true) == S::Listed);
    CHECK(of(1, true, true, 0, true, true) == S::SunOnly);
    CHECK(of(1, true, true, 0, false, true) == S::SunOnly);
    CHECK(of(1, true, true, kNoFused, true, true) == S::Listed);
    CHECK(of(2, true, true, 0, true, true) == S::Listed);
    CHECK(of(1, true, false, 0, false, true) == S::Listed);
    // the bit's value is part of the C-ABI
    CHECK(kNoFused == 0x40u);
    // the default state: no light
    CHECK(shadeScheduleOf(ShadeScheduleState {}) == S::Listed);
    return 0;
}

int sweep()
{
    int sunOnly = 0;
    for (uint32_t lights = 0; lights <= 12; ++lights)
        for (int sun = 0; sun < 2; ++sun)
            for (int map = 0; map < 2; ++map)
                for (uint32_t flags = 0; flags < 0x80u; ++flags)
                    for (int w = 0; w < 4; ++w) {
                        const bool half = (w & 1) != 0, small = (w & 2) != 0;
                        const bool want = lights == 1 && sun && map && !(flags & kNoFused) && (!half || small);
                        CHECK((of(lights, sun != 0, map != 0, flags, half, small) == S::SunOnly) == want);
                        sunOnly += want;
                    }
    CHECK(sunOnly == 64 * 3); // one (lights, sun, map) x the 64 flag words without the bit x 3 of the 4 window states
    return 0;
}

} // namespace

int main()
{
    if (table()) return 1;
    std::printf("table: OK\n");
    if (sweep()) return 1;
    std::printf("sweep: OK\n");
    return 0;
}
