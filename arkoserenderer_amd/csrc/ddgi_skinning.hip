// ddgi_skinning.hip — k_skin_vertices: the reference's skinning pass (arkose/shaders/
// skinning/skinning.comp, dispatched per segment of every skeletal-mesh instance ahead of
// its BLAS update, GpuScene.cpp:629-711) for gfx950. One vertex per thread, 256 per
// workgroup; the arithmetic is skinning.h's, shared with the host restatement
// (skinning_host.cpp) and compared with it by bits.
//
// A streaming kernel. Bytes per vertex, with K morph targets:
//   in   12 bind position + 36 bind ArkRTVertex + 32 ArkSkinningVertex + 36 K morph targets
//        + 12 previous position (from the second run on) + four gathered 48-B joints
//   out  12 position + 36 ArkRTVertex + 12 velocity
// = 140 + 36 K (+ 12) B of streamed traffic; the joints (48 B x joint_count, 12 KB at 256)
// are read once per workgroup and stay in L2, so they are not counted per vertex.
//
// Coalescing. Rows of 12 and 36 B do not line up with 16 B per lane, so a workgroup's rows
// are staged through LDS as flat word ranges (k_stage_vertices' answer, across a workgroup):
// a range is copied with 16-B accesses from its first 16-B-aligned word on and word by word
// before and after (stageIn / stageOut), every wave-instruction touching consecutive bytes;
// a thread then reads its row from LDS at a stride of 3 or 9 words, both odd, so the 32
// lanes of a group fall on 32 different banks. A range's LDS image starts at the word
// offset its global address has within 16 B, so that both sides of a 16-B copy are aligned.
// A workgroup's slice of a skin's own arrays starts 16-B aligned (256 rows); morph target
// k's slice (k n rows in) and an output that begins at any vertex need not, and every
// first-word offset 0..3 and every tail length takes the same code. ArkSkinningVertex rows
// are 32 B and aligned: two 16-B loads per lane, no staging.
//
// Joints. Up to skin::kLdsJoints (256, 12 KB) are copied to LDS once per workgroup and the
// four a vertex blends are read from there; a larger skeleton gathers them from global
// memory (L2) instead. Two instantiations of one kernel, chosen at launch.
//
// LDS: 772 + 2 x 2,308 words of staging (21.6 KB) + 12 KB of joints = 33.8 KB per
// workgroup, four workgroups per CU by LDS.
#include <hip/hip_runtime.h>

#include "ddgi_kernels.h"
#include "skinning.h"

namespace ark {
namespace dev {

namespace {

constexpr uint32_t kSkinBlock = 256;

// the word offset of a global address within 16 B
__device__ __forceinline__ uint32_t wordInQuad(const float* g) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(g) >> 2) & 3u; }

// `words` floats g -> lds by the whole workgroup; lds points wordInQuad(g) words past a
// 16-B-aligned LDS address. Reads exactly [g, g + words).
__device__ __forceinline__ void stageIn(float* lds, const float* __restrict__ g, uint32_t words)
{
    const uint32_t t = threadIdx.x;
    const uint32_t head = min(words, (4u - wordInQuad(g)) & 3u), quads = (words - head) >> 2, tail = head + 4u * quads;
    if (t < head) lds[t] = g[t];
    for (uint32_t i = t; i < quads; i += kSkinBlock) *reinterpret_cast<float4*>(lds + head + 4u * i) = *reinterpret_cast<const float4*>(g + head + 4u * i);
    if (t < words - tail) lds[tail + t] = g[tail + t];
}

// the reverse: writes exactly [g, g + words)
__device__ __forceinline__ void stageOut(float* __restrict__ g, const float* lds, uint32_t words)
{
    const uint32_t t = threadIdx.x;
    const uint32_t head = min(words, (4u - wordInQuad(g)) & 3u), quads = (words - head) >> 2, tail = head + 4u * quads;
    if (t < head) g[t] = lds[t];
    for (uint32_t i = t; i < quads; i += kSkinBlock) *reinterpret_cast<float4*>(g + head + 4u * i) = *reinterpret_cast<const float4*>(lds + head + 4u * i);
    if (t < words - tail) g[tail + t] = lds[tail + t];
}

} // namespace

template<bool kJointsInLds>
__global__ void __launch_bounds__(kSkinBlock) k_skin_vertices(SkinArgs a)
{
    __shared__ __attribute__((aligned(16))) float sPos[3 * kSkinBlock + 4];
    __shared__ __attribute__((aligned(16))) float sVert[9 * kSkinBlock + 4];
    __shared__ __attribute__((aligned(16))) float sAux[9 * kSkinBlock + 4]; // a morph target's rows, then the previous positions, then the velocities
    __shared__ __attribute__((aligned(16))) float sJoint[kJointsInLds ? 12 * skin::kLdsJoints : 4];

    const uint32_t t = threadIdx.x;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kSkinBlock;
    const uint32_t cnt = static_cast<uint32_t>(min(static_cast<uint64_t>(kSkinBlock), a.vertexCount - base));
    const bool live = t < cnt;

    const float* gPos = a.bindPositions + 3u * base;
    const float* gVert = a.bindVertices + 9u * base;
    float* inPos = sPos + wordInQuad(gPos);
    float* inVert = sVert + wordInQuad(gVert);
    stageIn(inPos, gPos, 3u * cnt);
    stageIn(inVert, gVert, 9u * cnt);
    if (kJointsInLds && a.skinning)
        for (uint32_t i = t; i < 3u * a.jointCount; i += kSkinBlock) reinterpret_cast<float4*>(sJoint)[i] = reinterpret_cast<const float4*>(a.joints)[i];
    __syncthreads();

    skin::Vertex v {};
    if (live) skin::loadVertex(v, inPos + 3u * t, inVert + 9u * t);

    // skinning.comp:46-65
    for (uint32_t k = 0; k < a.morphCount; ++k) {
        const float* g = a.morph + 9u * (static_cast<uint64_t>(k) * a.vertexCount + base);
        float* rows = sAux + wordInQuad(g);
        stageIn(rows, g, 9u * cnt);
        __syncthreads();
        if (live) skin::morphStep(v, rows + 9u * t, a.morphWeights[k]);
        __syncthreads();
    }
    if (a.morphCount && live) skin::morphFinish(v);

    // skinning.comp:69-85
    if (a.skinning && live) {
        const uint4 ji = a.skinning[2u * (base + t)];
        const float4 jw = reinterpret_cast<const float4*>(a.skinning)[2u * (base + t) + 1u];
        const float w[4] = { jw.x, jw.y, jw.z, jw.w };
        const float* J = kJointsInLds ? sJoint : a.joints;
        float A[12];
        skin::blendJoints(A, J + 12u * ji.x, J + 12u * ji.y, J + 12u * ji.z, J + 12u * ji.w, w);
        skin::applyJoints(v, A);
    }

    // skinning.comp:92-98: the previous run's position of this vertex
    float prev[3] = { 0.0f, 0.0f, 0.0f };
    if (a.prev) {
        const float* g = a.prev + 3u * base;
        float* rows = sAux + wordInQuad(g);
        stageIn(rows, g, 3u * cnt);
        __syncthreads();
        if (live) prev[0] = rows[3u * t], prev[1] = rows[3u * t + 1u], prev[2] = rows[3u * t + 2u];
    }
    // (every thread holds its row in registers: the staging areas become the outputs' images)
    __syncthreads();
    float* gOutPos = a.outPositions + 3u * base;
    float* gOutVert = a.outVertices + 9u * base;
    float* gOutVel = a.outVelocities + 3u * base;
    float* outPos = sPos + wordInQuad(gOutPos);
    float* outVert = sVert + wordInQuad(gOutVert);
    float* outVel = sAux + wordInQuad(gOutVel);
    if (live) {
        skin::storeVertex(v, outPos + 3u * t, outVert + 9u * t);
        skin::velocity(outVel + 3u * t, v.p, prev, a.prev == nullptr);
    }
    __syncthreads();
    stageOut(gOutPos, outPos, 3u * cnt);
    stageOut(gOutVert, outVert, 9u * cnt);
    stageOut(gOutVel, outVel, 3u * cnt);
}

} // namespace dev

hipError_t launch_skin_vertices(const SkinArgs& a, hipStream_t s)
{
    if (a.vertexCount == 0) return hipSuccess;
    const dim3 grid((a.vertexCount + dev::kSkinBlock - 1u) / dev::kSkinBlock), block(dev::kSkinBlock);
    if (a.skinning && a.jointCount > skin::kLdsJoints)
        hipLaunchKernelGGL(dev::k_skin_vertices<false>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(dev::k_skin_vertices<true>, grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace ark
