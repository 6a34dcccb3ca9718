// DDGINode.h — drop-in DDGI node on the HIP backend. Same name ("DDGI"), same
// members and defaults as arkose/rendering/nodes/DDGINode.h:10-39, same published
// resource ("DDGISamplingSet" = {grid CB, probe offsets SB, irradiance atlas,
// visibility atlas}, DDGINode.cpp:62-66). The GPU work is the C-ABI of
// libark_ddgi (include/ark_ddgi.h) instead of a Vulkan RT pipeline.
#pragma once

#include "../GpuScene.h"
#include "../RenderPipelineNode.h"
#include "../backend/hip/SlabExchange.h"

#include <cstdint>
#include <vector>

class DDGINode final : public RenderPipelineNode {
public:
    std::string name() const override { return "DDGI"; }
    void drawGui() override {}

    ExecuteCallback construct(GpuScene&, Registry&) override;

    // Settings the reference edits through ImGui (DDGINode.cpp:17-35); exposed as setters here.
    void setRaysPerProbe(int r) { m_raysPerProbeInt = r; }
    void setProbeUpdatesPerFrame(int n) { m_probeUpdatesPerFrame = n; }
    void setHysteresis(float irradiance, float visibility) { m_hysteresisIrradiance = irradiance; m_hysteresisVisibility = visibility; }
    void setVisibilitySharpness(float s) { m_visibilitySharpness = s; }
    void setComputeProbeOffsets(bool c) { m_computeProbeOffsets = c; }
    void setApplyProbeOffsets(bool a) { m_applyProbeOffsets = a; }
    void setMaxProbeUpdates(int n) { m_maxProbeUpdates = n; }
    void setShard(int rank, int count) { m_shardRank = rank; m_shardCount = count; }
    // ARK_DDGI_FLAG_GPU_REBUILD (before construct; experimental, off): the world BVHs'
    // background rebuilds after moved instances run on the device instead of host threads
    void setGpuRebuild(bool on) { m_gpuRebuild = on; }
    // ARK_DDGI_FLAG_GPU_REBUILD_SUN (before construct; experimental, off; either may be set
    // alone): the light-space sun BVH's background builds run on the device too
    void setGpuRebuildSun(bool on) { m_gpuRebuildSun = on; }
    // ARK_DDGI_FLAG_GPU_REBUILD_SAH (before construct; experimental, off): those device builds
    // rebuild every subtree of at most 256 triangles by a sweep SAH; alone it does nothing
    void setGpuRebuildSah(bool on) { m_gpuRebuildSah = on; }
    // ARK_DDGI_FLAG_GPU_REBUILD_PLAN (before construct; experimental, off): the device builds
    // that run the SAH pass collapse by the SAH-optimal plan; without that pass it does nothing
    void setGpuRebuildPlan(bool on) { m_gpuRebuildPlan = on; }
    // off: ARK_DDGI_FLAG_NO_RAY_SEEDS (before construct; on by default): no per-probe cache of
    // the last hit per direction for the probe rays to test first; same results
    void setRaySeeds(bool on) { m_raySeeds = on; }
    // Z-slab ranks: the atlas exchange after each update (RCCL all-gather, or device
    // copies for contexts in one process); frame n+1's shading waits for frame n's.
    void setSlabExchange(SlabExchange* exchange) { m_exchange = exchange; }
    // the event the last exchange completes (null without an exchange): consumers of
    // DDGISamplingSet on other ranks' bands wait on it
    void* pendingExchange() const { return m_exchangePending; }
    ArkDdgiCtx* context() const { return m_ctx; }
    int probeUpdateIdx() const { return m_probeUpdateIdx; }
    void setProbeUpdateIdx(int idx) { m_probeUpdateIdx = idx; }
    // DDGI history checkpoint (ark_ddgi_save_state / _load_state): atlases, offsets and
    // the rolling window position, so a resumed node continues where it stopped
    bool saveState(std::vector<uint8_t>& out) const;
    bool loadState(const std::vector<uint8_t>& blob);

    // we can dynamically choose to do fewer samples or probes, but not more since it defines the fixed image size
    static constexpr int MaxNumProbeSamples { ARK_DDGI_MAX_RAYS_PER_PROBE };
    static constexpr int MaxNumProbeUpdates { ARK_DDGI_REFERENCE_MAX_PROBE_UPDATES };

private:
    int m_raysPerProbeInt = 256;
    float m_hysteresisIrradiance { 0.93f };
    float m_hysteresisVisibility { 0.93f };

    float m_visibilitySharpness { 50.0f };

    int m_probeUpdatesPerFrame { 2048 };
    int m_probeUpdateIdx { 0 };

    bool m_computeProbeOffsets { true };
    bool m_applyProbeOffsets { true };

    bool m_useSceneAmbient { true };
    float m_injectedAmbientLx { 100.0f };

    // MI355X: the window may cover the whole grid (288 GB of HBM; the reference caps at 4096)
    int m_maxProbeUpdates { MaxNumProbeUpdates };
    int m_shardRank { 0 };
    int m_shardCount { 1 };
    bool m_gpuRebuild { false };
    bool m_gpuRebuildSun { false };
    bool m_gpuRebuildSah { false };
    bool m_gpuRebuildPlan { false };
    bool m_raySeeds { true };
    ArkDdgiCtx* m_ctx { nullptr };
    uint32_t m_instanceVersion { 0 }; // GpuScene::instanceVersion() the context's BVHs follow
    uint32_t m_vertexVersion { 0 };   // GpuScene::vertexVersion() its pools follow
    uint32_t m_poseVersion { 0 };     // GpuScene::poseVersion() its skins' ranges follow (0: the bind pose)
    std::vector<uint32_t> m_skins;    // the context's skin of each skeletal mesh instance
    // the scene's skeletal mesh instances registered with the context (after every set_scene, which drops them)
    bool registerSkins(GpuScene& scene);
    // the poses newer than m_poseVersion, with `instances` (null: the transforms stay), in one refit on `stream`
    int sendPoses(GpuScene& scene, const ArkRTInstance* instances, uint32_t instanceCount, void* stream);
    SlabExchange* m_exchange { nullptr };
    void* m_updateDone { nullptr };      // hipEvent_t recorded after each update
    void* m_exchangePending { nullptr }; // hipEvent_t of the last exchange
public:
    ~DDGINode() override;
};
