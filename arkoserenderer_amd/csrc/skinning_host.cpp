// skinning_host.cpp — registration checks, the serial restatement of k_skin_vertices and
// the host bound of a pose's positions (skinning_host.h).
#include "skinning_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ark {
namespace skin {

namespace {

bool finiteAll(const float* v, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

void emptyBox(double* b)
{
    b[0] = b[1] = b[2] = INFINITY;
    b[3] = b[4] = b[5] = -INFINITY;
}

void growBox(double* b, const float* p)
{
    for (int a = 0; a < 3; ++a) {
        b[a] = std::min(b[a], static_cast<double>(p[a]));
        b[3 + a] = std::max(b[3 + a], static_cast<double>(p[a]));
    }
}

} // namespace

int buildSkin(const ArkDdgiSkinDesc* d, std::unique_ptr<SkinHost>& out, std::string& why)
{
    auto bad = [&](const char* m) {
        why = m;
        return static_cast<int>(ARK_DDGI_E_INVALID_ARGUMENT);
    };
    if (!d || d->struct_size != sizeof(ArkDdgiSkinDesc)) return bad("register_skin: bad ArkDdgiSkinDesc");
    const size_t n = d->vertex_count, K = d->morph_target_count;
    if (n == 0) return bad("register_skin: no vertices");
    if (!d->positions || !d->vertices) return bad("register_skin: bind positions and vertices are required");
    if (K && !d->morph_targets) return bad("register_skin: morph_target_count without morph_targets");
    if (d->skinning && d->joint_count == 0) return bad("register_skin: skinning vertices without joints");
    if (!d->skinning && K == 0) return bad("register_skin: neither a skeleton nor morph targets");
    if (static_cast<uint64_t>(d->first_vertex) + n > 0xffffffffull) return bad("register_skin: vertex range overflows");
    if (!finiteAll(d->positions, 3 * n)) return bad("register_skin: non-finite bind position");
    if (!finiteAll(reinterpret_cast<const float*>(d->vertices), 9 * n)) return bad("register_skin: non-finite bind vertex");
    if (K && !finiteAll(reinterpret_cast<const float*>(d->morph_targets), 9 * K * n)) return bad("register_skin: non-finite morph target");
    if (d->skinning)
        for (size_t i = 0; i < n; ++i)
            for (int q = 0; q < 4; ++q) {
                const float w = d->skinning[i].joint_weights[q];
                if (!std::isfinite(w) || w < 0.0f) return bad("register_skin: a joint weight is negative or not finite");
                if (d->skinning[i].joint_indices[q] >= d->joint_count) return bad("register_skin: a joint index is outside joint_count");
            }

    std::unique_ptr<SkinHost> s(new SkinHost);
    s->firstVertex = d->first_vertex;
    s->vertexCount = d->vertex_count;
    s->morphCount = d->morph_target_count;
    s->skeleton = d->skinning != nullptr;
    s->jointCount = s->skeleton ? d->joint_count : 0u;
    s->positions.assign(d->positions, d->positions + 3 * n);
    const float* v = reinterpret_cast<const float*>(d->vertices);
    s->vertices.assign(v, v + 9 * n);
    if (K) {
        const float* m = reinterpret_cast<const float*>(d->morph_targets);
        s->morph.assign(m, m + 9 * K * n);
    }
    if (s->skeleton) {
        s->indices.resize(4 * n);
        s->weights.resize(4 * n);
        for (size_t i = 0; i < n; ++i)
            for (int q = 0; q < 4; ++q) {
                s->indices[4 * i + q] = d->skinning[i].joint_indices[q];
                s->weights[4 * i + q] = d->skinning[i].joint_weights[q];
            }
    }
    const size_t J = s->boundJoints();
    s->jointBox.resize(6 * J);
    s->morphBox.resize(6 * J * std::max<size_t>(K, 1));
    for (size_t j = 0; j < J; ++j) emptyBox(&s->jointBox[6 * j]);
    for (size_t e = 0; e < J * K; ++e) emptyBox(&s->morphBox[6 * e]);
    auto add = [&](size_t j, size_t i) {
        growBox(&s->jointBox[6 * j], &s->positions[3 * i]);
        for (size_t k = 0; k < K; ++k) growBox(&s->morphBox[6 * (j * K + k)], &s->morph[9 * (k * n + i)]);
    };
    s->sMin = s->sMax = 1.0;
    if (s->skeleton) {
        s->sMin = INFINITY;
        s->sMax = -INFINITY;
        for (size_t i = 0; i < n; ++i) {
            double sum = 0.0;
            for (int q = 0; q < 4; ++q) {
                const float w = s->weights[4 * i + q];
                sum += w;
                if (w != 0.0f) add(s->indices[4 * i + q], i);
            }
            s->sMin = std::min(s->sMin, sum);
            s->sMax = std::max(s->sMax, sum);
        }
        if (!std::isfinite(s->sMax)) return bad("register_skin: a weight sum is not finite");
    } else {
        for (size_t i = 0; i < n; ++i) add(0, i);
    }
    out = std::move(s);
    return ARK_DDGI_OK;
}

void jointRows(const float* m, uint32_t count, float* out)
{
    for (uint32_t j = 0; j < count; ++j)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) out[12 * j + 4 * r + c] = m[16 * j + 4 * c + r];
}

// The bound of a pose (DESIGN §1 "Skinning").
//
// Exact arithmetic first. A morphed position of a vertex that joint j influences lies in
// P_j = B_j + sum_k m_k D_jk (interval arithmetic on the sign of m_k); y_j = M_j (p, 1) then
// lies in the box M_j P_j, and in Y, the union over the joints some vertex uses. A skinned
// position is sum_q w_q y_q with w_q >= 0, every y_q in Y (a zero weight's term is zero)
// and sum w in [sMin, sMax], so each coordinate lies in [min(sMin lo, sMax lo), max(sMin hi,
// sMax hi)]. All of this is evaluated in double from fp32 data: its own rounding, 2^-53
// relative per operation, is covered many times over by the widening below.
//
// The kernel's fp32 evaluation error (skinning.h; u = 2^-24, gamma_n = n u / (1 - n u),
// Higham 2002 §3.1). The longest chain a position coordinate passes through:
//   morphing     p + d_1 w_1 + ... + d_K w_K: each step one product and one sum, so every
//                term carries at most 2 K rounding factors;
//   the blend    A_rc = sum_q M_q,rc w_q: a product and three sums, at most 4 factors;
//   the row      A_r0 p.x + A_r1 p.y + A_r2 p.z + A_r3: a product and three sums, 4 factors.
// A term of the expanded result, w_q M_q,rc p_c (or w_q M_q,r3), is a product of these, so
// it carries at most n = 2 K + 8 factors (1 + delta), |delta| <= u, and the computed
// coordinate differs from the exact one by at most gamma_n sum |terms|. The sum of the
// terms' magnitudes is at most E_r = sMax max_j (sum_c |M_j,rc| |P_j|_c + |M_j,r3|) with
// |P_j|_c = max(|B_j lo_c|, |B_j hi_c|) + sum_k |m_k| max(|D_jk lo_c|, |D_jk hi_c|).
// Underflow adds at most 2^-150 per operation, n 2^-149 in all. The bound is widened by
// gamma_n E_r + n 2^-149 and rounded outward to fp32.
bool poseBound(const SkinHost& s, const float* joints12, const float* mw, float out[6], std::string& why)
{
    const size_t J = s.boundJoints(), K = s.morphCount;
    if (K && !finiteAll(mw, K)) {
        why = "skin_geometry: a morph weight is not finite";
        return false;
    }
    if (s.skeleton && !finiteAll(joints12, 12 * J)) {
        why = "skin_geometry: a joint matrix is not finite";
        return false;
    }
    static const float kIdentity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY }, E[3] = { 0, 0, 0 };
    for (size_t j = 0; j < J; ++j) {
        const double* B = &s.jointBox[6 * j];
        if (!(B[0] <= B[3])) continue; // no vertex uses the joint
        double plo[3], phi[3], pabs[3];
        for (int c = 0; c < 3; ++c) {
            plo[c] = B[c];
            phi[c] = B[3 + c];
            pabs[c] = std::max(std::fabs(B[c]), std::fabs(B[3 + c]));
        }
        for (size_t k = 0; k < K; ++k) {
            const double* D = &s.morphBox[6 * (j * K + k)];
            const double m = mw[k];
            for (int c = 0; c < 3; ++c) {
                plo[c] += m >= 0.0 ? m * D[c] : m * D[3 + c];
                phi[c] += m >= 0.0 ? m * D[3 + c] : m * D[c];
                pabs[c] += std::fabs(m) * std::max(std::fabs(D[c]), std::fabs(D[3 + c]));
            }
        }
        const float* M = s.skeleton ? joints12 + 12 * j : kIdentity;
        for (int r = 0; r < 3; ++r) {
            double l = M[4 * r + 3], h = M[4 * r + 3], e = std::fabs(static_cast<double>(M[4 * r + 3]));
            for (int c = 0; c < 3; ++c) {
                const double a = static_cast<double>(M[4 * r + c]) * plo[c], b = static_cast<double>(M[4 * r + c]) * phi[c];
                l += std::min(a, b);
                h += std::max(a, b);
                e += std::fabs(static_cast<double>(M[4 * r + c])) * pabs[c];
            }
            lo[r] = std::min(lo[r], l);
            hi[r] = std::max(hi[r], h);
            E[r] = std::max(E[r], e);
        }
    }
    const double n = 2.0 * static_cast<double>(K) + 8.0, u = std::ldexp(1.0, -24), gamma = n * u / (1.0 - n * u);
    for (int r = 0; r < 3; ++r) {
        if (!(lo[r] <= hi[r])) lo[r] = hi[r] = 0.0; // every weight zero: every position is 0
        const double l = std::min(s.sMin * lo[r], s.sMax * lo[r]), h = std::max(s.sMin * hi[r], s.sMax * hi[r]);
        const double widen = gamma * (s.sMax * E[r]) + n * std::ldexp(1.0, -149);
        out[r] = std::nextafter(static_cast<float>(l - widen), -INFINITY);
        out[3 + r] = std::nextafter(static_cast<float>(h + widen), INFINITY);
    }
    if (!finiteAll(out, 6)) {
        why = "skin_geometry: the pose's bound is not finite";
        return false;
    }
    return true;
}

void skinRun(const SkinHost& s, const float* joints12, const float* mw, const float* prev, float* outP, float* outV, float* outVel)
{
    const size_t n = s.vertexCount, K = s.morphCount;
    for (size_t i = 0; i < n; ++i) {
        Vertex v;
        loadVertex(v, &s.positions[3 * i], &s.vertices[9 * i]);
        if (K) {
            for (size_t k = 0; k < K; ++k) morphStep(v, &s.morph[9 * (k * n + i)], mw[k]);
            morphFinish(v);
        }
        if (s.skeleton) {
            const uint32_t* ji = &s.indices[4 * i];
            float A[12];
            blendJoints(A, joints12 + 12 * ji[0], joints12 + 12 * ji[1], joints12 + 12 * ji[2], joints12 + 12 * ji[3], &s.weights[4 * i]);
            applyJoints(v, A);
        }
        const float zero[3] = { 0, 0, 0 };
        velocity(outVel + 3 * i, v.p, prev ? prev + 3 * i : zero, prev == nullptr);
        storeVertex(v, outP + 3 * i, outV + 9 * i);
    }
}

int Registry::add(const ArkDdgiSkinDesc* desc, uint32_t* handle, std::string& why)
{
    std::unique_ptr<SkinHost> s;
    if (const int rc = buildSkin(desc, s, why)) return rc;
    if (!handle) {
        why = "register_skin: null out_skin";
        return ARK_DDGI_E_INVALID_ARGUMENT;
    }
    *handle = static_cast<uint32_t>(skins.size());
    skins.push_back(std::move(s));
    return ARK_DDGI_OK;
}

bool Registry::remove(uint32_t handle)
{
    if (handle >= skins.size() || !skins[handle]) return false;
    skins[handle].reset();
    return true;
}

size_t Registry::live() const
{
    size_t n = 0;
    for (const auto& s : skins) n += s ? 1 : 0;
    return n;
}

} // namespace skin
} // namespace ark
