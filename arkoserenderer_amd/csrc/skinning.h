// skinning.h — the arithmetic of the reference's skinning pass (arkose/shaders/skinning/
// skinning.comp:35-98), written once: k_skin_vertices (ddgi_skinning.hip) and the serial
// host restatement (skinning_host.cpp) call these functions in the same order, and both
// sides are compiled with -ffp-contract=off, so their results are compared by bits. Pure
// C++ without a HIP dependency (the host side is also built on its own, tests/cpp).
//
// Adopted semantics:
//  - normalize is the kernels' own (ddgi_device.h): v * (1 / sqrt(dot(v, v))), dot left to right.
//  - A joint is 12 floats, rows 0-2 of the reference's mat4 (row-major 3 x 4): the shader
//    only ever forms vec3(A * vec4(p, 1)), which drops w, and mat3(A), which drops row and
//    column 3, so row 3 of a joint matrix is unobservable and the result is unchanged.
//  - The blend M0*w.x + M1*w.y + M2*w.z + M3*w.w is component-wise, left to right.
//  - A * vec4(p, 1), per row: A_r0*p.x + A_r1*p.y + A_r2*p.z + A_r3, left to right.
//  - transpose(inverse(mat3(A))) is the cofactor matrix times 1 / det. With a_rc the blended
//    3 x 3, the cofactors are
//        C00 = a11*a22 - a12*a21   C01 = a12*a20 - a10*a22   C02 = a10*a21 - a11*a20
//        C10 = a02*a21 - a01*a22   C11 = a00*a22 - a02*a20   C12 = a01*a20 - a00*a21
//        C20 = a01*a12 - a02*a11   C21 = a02*a10 - a00*a12   C22 = a00*a11 - a01*a10
//    det is expanded along the first column, det = a00*C00 + a10*C10 + a20*C20 (left to
//    right), inv = 1 / det, N_rc = C_rc * inv, and N * v per row is N_r0*v.x + N_r1*v.y +
//    N_r2*v.z, left to right. A singular blend gives non-finite normals and tangents, as in
//    the reference; the position does not pass through the inverse and stays finite.
//  - Morph target k's vertices start at k * vertex_count of the skin's own array, an
//    integer, where the reference passes the first vertex through a float (GpuScene.cpp:675,
//    uint(meta.x)): a deliberate deviation, the two agree below 2^24.
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "ark_fmath.h"

namespace ark {
namespace skin {

// a skin of at most this many joints keeps them in LDS (48 B each: 12 KB); more are gathered from global memory
constexpr uint32_t kLdsJoints = 256;

// One vertex in flight: the position and the NonPositionVertex (uv, normal, tangent.xyzw)
struct Vertex {
    float p[3];
    float uv[2];
    float n[3];
    float t[4];
};

// from / to a position (3 words) and an ArkRTVertex (9 words: uv, normal, tangent)
ARK_HD void loadVertex(Vertex& v, const float* p, const float* w)
{
    v.p[0] = p[0], v.p[1] = p[1], v.p[2] = p[2];
    v.uv[0] = w[0], v.uv[1] = w[1];
    v.n[0] = w[2], v.n[1] = w[3], v.n[2] = w[4];
    v.t[0] = w[5], v.t[1] = w[6], v.t[2] = w[7], v.t[3] = w[8];
}
ARK_HD void storeVertex(const Vertex& v, float* p, float* w)
{
    p[0] = v.p[0], p[1] = v.p[1], p[2] = v.p[2];
    w[0] = v.uv[0], w[1] = v.uv[1];
    w[2] = v.n[0], w[3] = v.n[1], w[4] = v.n[2];
    w[5] = v.t[0], w[6] = v.t[1], w[7] = v.t[2], w[8] = v.t[3];
}

ARK_HD void normalize3(float v[3])
{
    const float s = 1.0f / sqrtf_(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] = v[0] * s;
    v[1] = v[1] * s;
    v[2] = v[2] * s;
}

// skinning.comp:55-57, one morph target: d = MorphTargetVertex (position, normal, tangent)
ARK_HD void morphStep(Vertex& v, const float d[9], float w)
{
    for (int a = 0; a < 3; ++a) {
        v.p[a] = v.p[a] + d[a] * w;
        v.n[a] = v.n[a] + d[3 + a] * w;
        v.t[a] = v.t[a] + d[6 + a] * w;
    }
}

// skinning.comp:61-63, after the last morph target (not run at all when there is none)
ARK_HD void morphFinish(Vertex& v)
{
    normalize3(v.n);
    normalize3(v.t);
    const float d = v.n[0] * v.t[0] + v.n[1] * v.t[1] + v.n[2] * v.t[2];
    for (int a = 0; a < 3; ++a) v.t[a] = v.t[a] - v.n[a] * d;
    normalize3(v.t);
}

// skinning.comp:74-77: rows 0-2 of the blended matrix
ARK_HD void blendJoints(float A[12], const float* M0, const float* M1, const float* M2, const float* M3, const float w[4])
{
    for (int e = 0; e < 12; ++e) A[e] = M0[e] * w[0] + M1[e] * w[1] + M2[e] * w[2] + M3[e] * w[3];
}

// skinning.comp:79-83
ARK_HD void applyJoints(Vertex& v, const float A[12])
{
    const float px = v.p[0], py = v.p[1], pz = v.p[2];
    for (int r = 0; r < 3; ++r) v.p[r] = A[4 * r] * px + A[4 * r + 1] * py + A[4 * r + 2] * pz + A[4 * r + 3];
    const float a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[4], a11 = A[5], a12 = A[6], a20 = A[8], a21 = A[9], a22 = A[10];
    float C[9];
    C[0] = a11 * a22 - a12 * a21, C[1] = a12 * a20 - a10 * a22, C[2] = a10 * a21 - a11 * a20;
    C[3] = a02 * a21 - a01 * a22, C[4] = a00 * a22 - a02 * a20, C[5] = a01 * a20 - a00 * a21;
    C[6] = a01 * a12 - a02 * a11, C[7] = a02 * a10 - a00 * a12, C[8] = a00 * a11 - a01 * a10;
    const float det = a00 * C[0] + a10 * C[3] + a20 * C[6];
    const float inv = 1.0f / det;
    for (int e = 0; e < 9; ++e) C[e] = C[e] * inv;
    const float nx = v.n[0], ny = v.n[1], nz = v.n[2], tx = v.t[0], ty = v.t[1], tz = v.t[2];
    for (int r = 0; r < 3; ++r) {
        v.n[r] = C[3 * r] * nx + C[3 * r + 1] * ny + C[3 * r + 2] * nz;
        v.t[r] = C[3 * r] * tx + C[3 * r + 1] * ty + C[3 * r + 2] * tz;
    }
}

// skinning.comp:92-98: position - previous skinned position, zero on a skin's first run
ARK_HD void velocity(float vel[3], const float p[3], const float prev[3], bool first)
{
    for (int a = 0; a < 3; ++a) vel[a] = first ? 0.0f : p[a] - prev[a];
}

} // namespace skin
} // namespace ark
