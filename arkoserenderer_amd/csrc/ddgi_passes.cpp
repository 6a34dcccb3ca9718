// ddgi_passes.cpp — the context's passes beside the update: the AO / bent-normal bake and
// its read-back, the DDGI consumers (lighting compose, RT reflections), the ray-traced
// local-light shadow masks, the reflection denoiser passes and the probe debug view. Each is enqueued whole on the caller's stream, in call order (orderBegin / orderEnd).
#include <algorithm>
#include <cstring>

#include "ddgi_context.h"
#include "path_tracer_host.h"
#include "refl_denoise_host.h"
#include "rt_shadows_host.h"

namespace {

// RT reflections' ray-list work set for `pixels` rays (ark_ddgi_rt_reflections)
int ensureReflWork(ArkDdgiCtx* ctx, uint64_t pixels)
{
    if (pixels >= (1ull << 28) && ctx->lightCount > 0)
        return ctx->fail(ARK_DDGI_E_UNSUPPORTED, "%llu reflection rays: shadow-ray owners pack (ray << 4) | light in 32 bits", static_cast<unsigned long long>(pixels));
    auto al = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t bytes = al(pixels * 32) + al(pixels * sizeof(GpuHit)) + al(pixels * 4) + al((kRayCounterWords + kRayCounterStride) * 4) +
                           al(pixels * ctx->lightCount * sizeof(ShadowRay));
    if (ctx->reflWork.bytes < bytes) ARK_HIP(ctx->reflWork.alloc(bytes));
    return ARK_DDGI_OK;
}

} // namespace

extern "C" {

// AO / bent-normal bake (include/ark_ddgi.h; BakeAmbientOcclusionNode.cpp:15-131):
// raster -> barycentrics (+ covered-texel list) -> persistent AO rays, one stream.
int ark_ddgi_bake_ao(ArkDdgiCtx* ctx, const ArkBakeAoDesc* d, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!d || d->struct_size != sizeof(ArkBakeAoDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkBakeAoDesc");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake: no scene");
    if (d->instance_index >= ctx->sceneStore->instHost.size()) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake: instance %u out of range", d->instance_index);
    if (d->width == 0 || d->height == 0 || d->width > 16384 || d->height > 16384 || d->sample_count == 0)
        return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake: extent %ux%u / %u samples", d->width, d->height, d->sample_count);
    const ArkRTInstance& inst = ctx->sceneStore->instHost[d->instance_index];
    const ArkRTTriangleMesh& mesh = ctx->sceneStore->meshHost[inst.rt_mesh_index];
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    if (ctx->sceneVersion != ctx->sceneStore->version) // a sharing context refitted the scene or installed a deeper sun BVH
        if (const int rc = refreshScene(ctx)) return rc;
    ARK_HIP(orderBegin(ctx, s));
    const size_t texels = static_cast<size_t>(d->width) * d->height;
    const size_t outBytes = texels * (d->bent_normals ? 4 : 1);
    if (ctx->bakeTri.bytes < texels * 4) ARK_HIP(ctx->bakeTri.alloc(texels * 4));
    if (ctx->bakeBary.bytes < texels * 8) ARK_HIP(ctx->bakeBary.alloc(texels * 8));
    if (ctx->bakeOut.bytes < outBytes) ARK_HIP(ctx->bakeOut.alloc(outBytes));
    if (ctx->bakePixels.bytes < texels * 4) ARK_HIP(ctx->bakePixels.alloc(texels * 4));
    if (ctx->bakeCounters.bytes < 256) ARK_HIP(ctx->bakeCounters.alloc(256));
    ARK_HIP(hipMemsetAsync(ctx->bakeTri.ptr, 0, texels * 4, s)); // ClearValue::blackAtMaxDepth
    ARK_HIP(hipMemsetAsync(ctx->bakeCounters.ptr, 0, 256, s));
    BakeArgs b {};
    b.W = d->width;
    b.H = d->height;
    b.samples = d->sample_count;
    b.tri_count = inst.triangle_count;
    b.bent = d->bent_normals ? 1 : 0;
    b.first_index = static_cast<uint32_t>(mesh.first_index);
    b.first_vertex = static_cast<uint32_t>(mesh.first_vertex);
    b.indices = ctx->sceneStore->indices.as<uint32_t>();
    b.positions = ctx->sceneStore->positions.as<float>();
    b.vertices = ctx->sceneStore->vertices.as<float>();
    b.tri_idx = ctx->bakeTri.as<uint32_t>();
    b.bary = ctx->bakeBary.as<uint16_t>();
    b.out = ctx->bakeOut.as<uint8_t>();
    b.pixels = ctx->bakePixels.as<uint32_t>();
    b.counters = ctx->bakeCounters.as<uint32_t>();
    b.spill = ctx->spill.as<uint32_t>();
    if (b.tri_count > 0) ARK_HIP(launch_bake(ctx->scene, b, 0, 0, s));
    ARK_HIP(launch_bake(ctx->scene, b, 0, 1, s));
    // the persistent AO kernel uses the traversal spill area sized for shadowBlocks workgroups
    ARK_HIP(launch_bake(ctx->scene, b, ctx->shadowBlocks, 2, s));
    ARK_HIP(scenePositionsRead(*ctx->sceneStore, s)); // (the next vertex update's positions follow the bake)
    ARK_HIP(orderEnd(ctx, s));
    ctx->bakeW = d->width;
    ctx->bakeH = d->height;
    ctx->bakeBent = b.bent;
    return ARK_DDGI_OK;
}

int ark_ddgi_bake_read(ArkDdgiCtx* ctx, int which, void* dst, uint64_t bytes)
{
    if (!ctx || !dst) return ARK_DDGI_E_INVALID_ARGUMENT;
    const size_t texels = static_cast<size_t>(ctx->bakeW) * ctx->bakeH;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
    case ARK_BAKE_TRIANGLE_INDEX: src = ctx->bakeTri.ptr; n = texels * 4; break;
    case ARK_BAKE_BARYCENTRICS: src = ctx->bakeBary.ptr; n = texels * 8; break;
    case ARK_BAKE_OUTPUT: src = ctx->bakeOut.ptr; n = texels * (ctx->bakeBent ? 4 : 1); break;
    default: return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake_read: unknown resource %d", which);
    }
    if (texels == 0) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake_read: no bake yet");
    if (bytes != n) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bake_read: %llu bytes, resource has %zu", static_cast<unsigned long long>(bytes), n);
    ARK_HIP(hipSetDevice(ctx->device));
    ARK_HIP(hipDeviceSynchronize());
    ARK_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return ARK_DDGI_OK;
}

int ark_ddgi_lighting_compose(ArkDdgiCtx* ctx, const ArkComposeDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkComposeDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkComposeDesc");
    if (!desc->out) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "lighting_compose: no output plane");
    if (static_cast<uint64_t>(desc->width) * desc->height >= (1ull << 32)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "lighting_compose: target too large");
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    const FrameArgs f = samplingSetArgs(ctx);
    ArkComposeDesc c = *desc;
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(launch_lighting_compose(f, c, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

int ark_ddgi_rt_reflections(ArkDdgiCtx* ctx, const ArkReflectionsDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkReflectionsDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkReflectionsDesc");
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "rt_reflections before ark_ddgi_set_scene");
    if (!desc->out_radiance || !desc->out_direction) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections: no output image");
    if (desc->blue_noise && (desc->noise_width == 0 || desc->noise_height == 0)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections: empty blue noise");
    if (static_cast<uint64_t>(desc->width) * desc->height >= (1ull << 32)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections: target too large");
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    int rc;
    // the scene first: a sharing context's deeper sun BVH may grow,
    // i.e. reallocate, the spill area that f.spill points into below
    if (ctx->sceneVersion != ctx->sceneStore->version) {
        if ((rc = refreshScene(ctx)) != 0) return rc;
    } else if ((rc = ensureSpill(ctx)) != 0) {
        return rc;
    }
    FrameArgs f = samplingSetArgs(ctx);
    f.z_far = ctx->desc.z_far;
    f.ambient_amount = desc->ambient_amount;
    f.environment_multiplier = desc->environment_multiplier;
    f.spill = ctx->spill.as<uint32_t>();
    // ray-list work set (ensureReflWork): rays, hit records, light bits, shadow rays, counters
    const uint64_t pixels = static_cast<uint64_t>(desc->width) * desc->height;
    if (pixels == 0) return ARK_DDGI_OK;
    if ((rc = ensureReflWork(ctx, pixels)) != 0) return rc;
    {
        char* w = static_cast<char*>(ctx->reflWork.ptr);
        auto take = [&](uint64_t bytes) {
            char* q = w;
            w += (bytes + 255) & ~static_cast<uint64_t>(255);
            return q;
        };
        f.ray_list = reinterpret_cast<const float4*>(take(pixels * 32));
        f.hits = reinterpret_cast<GpuHit*>(take(pixels * sizeof(GpuHit)));
        f.shadow_bits = reinterpret_cast<uint32_t*>(take(pixels * 4));
        f.ray_counter = reinterpret_cast<uint32_t*>(take((kRayCounterWords + kRayCounterStride) * 4));
        f.shadow_rays = reinterpret_cast<ShadowRay*>(take(pixels * ctx->lightCount * sizeof(ShadowRay)));
    }
    f.shadow_count = f.ray_counter + kShadowCountWord;
    f.shadow_heads = f.ray_counter + kShadowHeadWord;
    f.list_count = f.ray_counter + kRayCounterWords;
    f.light_count = ctx->lightCount;
    f.refill_min = ctx->refillMin;
    f.sun_refill_min = ctx->sunRefillMin;
    f.grab_chunk = ctx->grabChunk;
    f.counters = ctx->counters.as<unsigned long long>();
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(flushLights(ctx, s));
    ARK_HIP(hipMemsetAsync(f.ray_counter, 0, (kRayCounterWords + kRayCounterStride) * 4, s));
    ARK_HIP(launch_rt_reflections(ctx->scene, f, *desc, ctx->traceBlocks, shadowBlocksFor(ctx, pixels), s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

// Ray-traced local-light shadow masks (include/ark_ddgi.h; RTLocalShadowNode.cpp:47-90):
// per batch of lights the ray list and its opaque-only traversal, then one resolve.
int ark_ddgi_rt_local_shadows(ArkDdgiCtx* ctx, const ArkRtShadowsDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkRtShadowsDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkRtShadowsDesc");
    if (const char* why = rtshadow::descProblem(*desc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_local_shadows: %s", why);
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "rt_local_shadows before ark_ddgi_set_scene");
    const uint64_t pixels = static_cast<uint64_t>(desc->width) * desc->height;
    if (pixels == 0 || desc->light_count == 0) return ARK_DDGI_OK;
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    int rc;
    // the scene first, as ark_ddgi_rt_reflections: a deeper sun BVH may reallocate the spill area
    if (ctx->sceneVersion != ctx->sceneStore->version) {
        if ((rc = refreshScene(ctx)) != 0) return rc;
    } else if ((rc = ensureSpill(ctx)) != 0) {
        return rc;
    }
    RtShadowArgs a {};
    a.width = desc->width;
    a.height = desc->height;
    a.frame_index = desc->frame_index;
    a.light_count = desc->light_count;
    std::memcpy(a.world_from_view, desc->world_from_view, sizeof(a.world_from_view));
    std::memcpy(a.view_from_projection, desc->view_from_projection, sizeof(a.view_from_projection));
    a.depth = desc->depth;
    for (uint32_t l = 0; l < desc->light_count; ++l) {
        rtshadow::lightFloats(desc->lights[l], a.lights[l]);
        a.masks[l] = desc->lights[l].out_mask;
    }
    // work set: result words, counters, the largest batch's ray list (ddgi_rt_shadows.inc: kRtShadowRayBudget)
    const uint32_t perBatch = static_cast<uint32_t>(std::min<uint64_t>(desc->light_count, std::max<uint64_t>(1, kRtShadowRayBudget / (pixels * sizeof(ShadowRay)))));
    auto al = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t counterBytes = (kRayCounterWords + kRayCounterStride) * 4;
    const uint64_t bytes = al(pixels * 4) + al(counterBytes) + al(pixels * perBatch * sizeof(ShadowRay));
    if (ctx->rtShadowWork.bytes < bytes) ARK_HIP(ctx->rtShadowWork.alloc(bytes));
    FrameArgs f = samplingSetArgs(ctx);
    f.spill = ctx->spill.as<uint32_t>();
    {
        char* w = static_cast<char*>(ctx->rtShadowWork.ptr);
        a.result = reinterpret_cast<uint32_t*>(w);
        w += al(pixels * 4);
        f.ray_counter = reinterpret_cast<uint32_t*>(w);
        w += al(counterBytes);
        f.shadow_rays = reinterpret_cast<ShadowRay*>(w);
    }
    f.shadow_bits = a.result;
    f.shadow_count = f.ray_counter + kShadowCountWord;
    f.shadow_heads = f.ray_counter + kShadowHeadWord;
    f.refill_min = ctx->refillMin;
    f.sun_refill_min = ctx->sunRefillMin;
    f.grab_chunk = ctx->grabChunk;
    ARK_HIP(orderBegin(ctx, s));
    for (uint32_t l0 = 0; l0 < desc->light_count; l0 += perBatch) {
        const uint32_t l1 = std::min(desc->light_count, l0 + perBatch);
        ARK_HIP(hipMemsetAsync(f.ray_counter, 0, counterBytes, s));
        ARK_HIP(launch_rt_shadow_batch(ctx->scene, f, a, l0, l1, shadowBlocksFor(ctx, pixels * (l1 - l0)), s));
    }
    ARK_HIP(launch_rt_shadow_resolve(a, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

// The path tracer (include/ark_ddgi.h; PathTracerNode.cpp:81-103; ddgi_path_tracer.inc): the
// frame in batches of whole 8 x 8 tiles whose lists and path state fit kPathTracerBudget,
// each batch 16 segments enqueued without a wait, then the accumulate step or the reset copy.
// The work set grows only when a call needs more than any before it (width, height and the
// light count decide), so a steady sequence of frames allocates nothing.
int ark_ddgi_path_trace(ArkDdgiCtx* ctx, const ArkPathTracerDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkPathTracerDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkPathTracerDesc");
    if (const char* why = pt::descProblem(*desc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "path_trace: %s", why);
    if (!ctx->hasScene) return ctx->fail(ARK_DDGI_E_NO_SCENE, "path_trace before ark_ddgi_set_scene");
    const uint64_t pixels = static_cast<uint64_t>(desc->width) * desc->height;
    if (pixels == 0) return ARK_DDGI_OK;
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    int rc;
    // the scene first, as ark_ddgi_rt_reflections: a deeper sun BVH may reallocate the spill area
    if (ctx->sceneVersion != ctx->sceneStore->version) {
        if ((rc = refreshScene(ctx)) != 0) return rc;
    } else if ((rc = ensureSpill(ctx)) != 0) {
        return rc;
    }
    PtArgs a {};
    a.width = desc->width;
    a.height = desc->height;
    a.frame_index = desc->frame_index;
    a.flags = desc->flags;
    a.accumulated_frames = desc->accumulated_frames;
    a.environment_multiplier = desc->environment_multiplier;
    a.z_near = desc->z_near;
    a.z_far = desc->z_far;
    std::memcpy(a.world_from_view, desc->world_from_view, sizeof(a.world_from_view));
    std::memcpy(a.view_from_projection, desc->view_from_projection, sizeof(a.view_from_projection));
    a.image = desc->image;
    a.accumulation = desc->accumulation;
    // batches of whole tiles under the budget, or the caller's size
    const uint64_t slots = static_cast<uint64_t>((desc->width + 7u) / 8u) * ((desc->height + 7u) / 8u) * 64u;
    const uint64_t perSlot = ptBytesPerSlot(ctx->lightCount);
    uint64_t batch = std::max<uint64_t>(64, kPathTracerBudget / perSlot / 64u * 64u);
    if (desc->max_paths_per_batch) batch = std::max<uint64_t>(64, std::min<uint64_t>(batch, desc->max_paths_per_batch / 64u * 64u));
    batch = std::min(batch, slots);
    auto al = [](uint64_t b) { return (b + 255) & ~static_cast<uint64_t>(255); };
    const uint64_t counterBytes = kPtCounterWords * 4u;
    const uint64_t bytes = al(counterBytes) + al(batch * 32) + 2 * al(batch * 32) + al(batch * 64) + al(batch * sizeof(GpuHit)) + al(batch * 4) +
                           al(batch * ctx->lightCount * sizeof(ShadowRay));
    if (ctx->ptWork.bytes < bytes) {
        if (ctx->ptWork.ptr) ARK_HIP(drainContext(ctx)); // an earlier frame may still use the smaller one
        ARK_HIP(ctx->ptWork.alloc(bytes));
    }
    FrameArgs f = samplingSetArgs(ctx);
    f.z_far = desc->z_far;
    f.spill = ctx->spill.as<uint32_t>();
    uint32_t* counters;
    {
        char* w = static_cast<char*>(ctx->ptWork.ptr);
        auto take = [&](uint64_t b) {
            char* q = w;
            w += al(b);
            return q;
        };
        counters = reinterpret_cast<uint32_t*>(take(counterBytes));
        a.state = reinterpret_cast<float4*>(take(batch * 32));
        a.lists[0] = reinterpret_cast<float4*>(take(batch * 32));
        a.lists[1] = reinterpret_cast<float4*>(take(batch * 32));
        a.surf = reinterpret_cast<float4*>(take(batch * 64));
        f.hits = reinterpret_cast<GpuHit*>(take(batch * sizeof(GpuHit)));
        f.shadow_bits = reinterpret_cast<uint32_t*>(take(batch * 4));
        f.shadow_rays = reinterpret_cast<ShadowRay*>(take(batch * ctx->lightCount * sizeof(ShadowRay)));
    }
    f.light_count = ctx->lightCount;
    f.refill_min = ctx->refillMin;
    f.sun_refill_min = ctx->sunRefillMin;
    f.grab_chunk = ctx->grabChunk;
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(flushLights(ctx, s));
    for (uint64_t s0 = 0; s0 < slots; s0 += batch) {
        a.slot0 = static_cast<uint32_t>(s0);
        a.slot1 = static_cast<uint32_t>(std::min(slots, s0 + batch));
        ARK_HIP(hipMemsetAsync(counters, 0, counterBytes, s));
        ARK_HIP(launch_path_trace_batch(ctx->scene, f, a, counters, ctx->traceBlocks, shadowBlocksFor(ctx, a.slot1 - a.slot0), s, ctx->ptSegments));
    }
    if (desc->flags) ARK_HIP(launch_path_trace_accumulate(a, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

// The reflection denoiser passes (include/ark_ddgi.h; RTReflectionsNode.cpp:86-139), in the
// node's order on one stream. No scene, no state: every plane is the caller's.
int ark_ddgi_rt_reflections_denoise(ArkDdgiCtx* ctx, const ArkReflDenoiseDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkReflDenoiseDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkReflDenoiseDesc");
    if (const char* why = refl::descProblem(*desc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "rt_reflections_denoise: %s", why);
    const uint64_t pixels = static_cast<uint64_t>(desc->width) * desc->height;
    if (pixels == 0) return ARK_DDGI_OK;
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    const refl::Args a = refl::argsOf(*desc);
    ARK_HIP(orderBegin(ctx, s));
    if (desc->flags & ARK_REFL_DENOISE_DISABLED) {
        ARK_HIP(hipMemcpyAsync(desc->resolved, desc->radiance, pixels * 8, hipMemcpyDeviceToDevice, s));
    } else {
        for (int pass = (desc->flags & ARK_REFL_DENOISE_FIRST_FRAME) ? 0 : 1; pass <= 4; ++pass) ARK_HIP(launch_refl_denoise_pass(a, pass, s));
    }
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

int ark_ddgi_probe_debug(ArkDdgiCtx* ctx, const ArkProbeDebugDesc* desc, void* hipStream)
{
    if (!ctx) return ARK_DDGI_E_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(ArkProbeDebugDesc)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "bad ArkProbeDebugDesc");
    if (desc->count && (!desc->probe_indices || !desc->directions || !desc->out)) return ctx->fail(ARK_DDGI_E_INVALID_ARGUMENT, "probe_debug: null plane");
    const hipStream_t s = streamOf(hipStream);
    ARK_HIP(hipSetDevice(ctx->device));
    const FrameArgs f = samplingSetArgs(ctx);
    ARK_HIP(orderBegin(ctx, s));
    ARK_HIP(launch_probe_debug(f, *desc, s));
    ARK_HIP(orderEnd(ctx, s));
    return ARK_DDGI_OK;
}

} // extern "C"
