// scene_rebuild_policy.h — which background BVH build a scene call starts (scene_store.cpp:
// sceneMaintenance, sceneSunStep) and how a job goes on after its device build
// (runRebuildJob). Pure host logic over plain values: no device call, so that the
// turn-taking and the fallback decision are tested on the CPU (tests/cpp/sanitize_test.cpp).
#pragma once

#include <cstdint>

#include "../../include/ark_ddgi.h"

namespace ark {

// the background build started last (loosened BVHs take turns)
enum : uint8_t { kBackgroundNone, kBackgroundWorld, kBackgroundSun };

// What a scene call knows when it decides, after it collected the finished jobs.
struct RebuildState {
    bool sunWanted = false;      // set_scene chose the light-space sun BVH
    bool hasSun = false;         // the calling context has a sun
    bool sunJobRunning = false, worldJobRunning = false;
    bool sunInstalled = false;   // a light-space BVH is installed for the caller's sun direction
    bool requestStable = false;  // the scene's contexts asked for this direction at least twice in a row
    bool sunFailedHere = false;  // a sun build failed for this direction and scene version
    bool worldRebuildFailed = false;
    bool worldGpuBuilt = false;  // the installed world BVHs are a device build
    bool sunGpuBuilt = false;    // the light-space BVH installed for the caller's sun direction is a device build
    uint32_t refitsSinceBuild = 0, sunRefitsSinceBuild = 0; // refits since the installed BVHs' snapshots
    uint32_t flags = 0;          // ArkDdgiDesc.flags of the caller
    uint8_t lastBackground = kBackgroundNone;
    bool sunOnly = false;        // set_lights: the world BVHs' rebuilds are left to the next update or set_instances
};

enum class RebuildStart { None, Sun, WorldHost, WorldDevice, SunDevice };

// The one build to start now.
//  - A light-space BVH missing for the caller's sun starts at once, even beside a running
//    world rebuild (until it is installed the sun's shadow rays traverse the world BVHs);
//    only on a stable request, and not again after a failure for the same direction and
//    scene version. Nothing else starts in that call.
//  - Loosened BVHs (refits since their build; not with ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD,
//    the world ones not after a failed rebuild) start only while no background build runs,
//    and when both the world BVHs and the light-space one are loosened they take turns
//    (under continuous motion each would otherwise start again the moment its last one is
//    installed).
//  - ARK_DDGI_FLAG_GPU_REBUILD: loosened world BVHs are rebuilt on the device; once the
//    motion has stopped (a device build installed, no refit since its snapshot) one host
//    rebuild replaces the LBVH with the SAH tree a static scene traces faster.
//  - ARK_DDGI_FLAG_GPU_REBUILD_SUN: a missing or loosened light-space BVH is built on the
//    device (SunDevice), under the conditions above; once the installed one is a device
//    build for the caller's direction and no refit has come since its snapshot, one host
//    rebuild (Sun) replaces it - the settle rule, in turns with a world settle rebuild like
//    any other pair of background builds. Without the bit nothing here changes.
//  - sunOnly never starts a world rebuild; the sun's turn there yields to loosened world
//    BVHs (not to a settle rebuild).
inline RebuildStart rebuildToStart(const RebuildState& q)
{
    const bool background = !(q.flags & ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD);
    const bool sunDevice = (q.flags & ARK_DDGI_FLAG_GPU_REBUILD_SUN) != 0;
    bool sunMissing = false, sunLoosened = false, sunSettle = false;
    if (q.sunWanted && q.hasSun && !q.sunJobRunning && q.requestStable && !q.sunFailedHere) {
        sunMissing = !q.sunInstalled;
        sunLoosened = q.sunInstalled && q.sunRefitsSinceBuild != 0 && background;
        sunSettle = sunDevice && q.sunInstalled && q.sunGpuBuilt && q.sunRefitsSinceBuild == 0;
    }
    if (sunMissing) return sunDevice ? RebuildStart::SunDevice : RebuildStart::Sun;
    if (q.sunJobRunning || q.worldJobRunning) return RebuildStart::None;
    const bool worldOk = background && !q.worldRebuildFailed;
    const bool worldLoosened = worldOk && q.refitsSinceBuild != 0;
    const bool worldSettle = worldOk && (q.flags & ARK_DDGI_FLAG_GPU_REBUILD) && q.worldGpuBuilt && q.refitsSinceBuild == 0;
    const bool world = !q.sunOnly && (worldLoosened || worldSettle);
    const bool sun = sunLoosened || sunSettle;
    if (world && (!sun || q.lastBackground != kBackgroundWorld))
        return worldLoosened && (q.flags & ARK_DDGI_FLAG_GPU_REBUILD) ? RebuildStart::WorldDevice : RebuildStart::WorldHost;
    const bool sunYields = q.sunOnly ? worldLoosened : world;
    if (sun && (!sunYields || q.lastBackground != kBackgroundSun)) return sunLoosened && sunDevice ? RebuildStart::SunDevice : RebuildStart::Sun;
    return RebuildStart::None;
}

// How a rebuild job goes on after its device build (scene_rebuild.cpp: runRebuildJob): the
// result is Installed as built; the job has Failed (the device is not used again by it);
// or the HostBuild builds this scene from the same snapshot, within the job.
enum class DeviceBuildOutcome { Installed, HostBuild, Failed };

// hipOk: every HIP call of the attempt succeeded; deviceFault: the failing one's error is a
// device fault (isDeviceFault); declined: the build named a reason to leave the scene to
// the host. A HIP error that is not a device fault is the host's too.
inline DeviceBuildOutcome deviceBuildOutcome(bool hipOk, bool deviceFault, bool declined)
{
    if (hipOk && !declined) return DeviceBuildOutcome::Installed;
    return deviceFault ? DeviceBuildOutcome::Failed : DeviceBuildOutcome::HostBuild;
}

} // namespace ark
