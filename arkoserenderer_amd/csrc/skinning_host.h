// skinning_host.h — the host side of the skinning pass (skinning.h): a registered skin's
// arrays and what its pose bounds need, the serial restatement of k_skin_vertices that the
// kernel is compared with bit for bit, and the conservative bound of a pose's positions
// that ark_ddgi_skin_geometry hands the refit. Pure host code without a HIP dependency
// (tests/cpp/skin_bounds_test.cpp builds it on its own).
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ark_ddgi.h"
#include "skinning.h"

namespace ark {
namespace skin {

// A registered skin (ark_ddgi_register_skin), its arrays copied and checked.
struct SkinHost {
    uint32_t firstVertex = 0, vertexCount = 0, jointCount = 0, morphCount = 0;
    bool skeleton = false;          // false: morph-only (identity joint, weight 1)
    std::vector<float> positions;   // 3 n
    std::vector<float> vertices;    // 9 n (ArkRTVertex)
    std::vector<uint32_t> indices;  // 4 n (skeleton)
    std::vector<float> weights;     // 4 n (skeleton)
    std::vector<float> morph;       // 9 K n: target k's vertices at k n
    // The pose bound's data. Per joint j (one pseudo joint for a morph-only skin) the box
    // B_j of the bind positions of the vertices that give j a non-zero weight (lo xyz, hi
    // xyz; lo > hi: no vertex uses j), per (j, k) the box D_jk of target k's position
    // deltas over the same vertices, and the least and greatest weight sum of a vertex.
    std::vector<double> jointBox; // 6 per joint
    std::vector<double> morphBox; // 6 per (joint, target): [(j K + k) 6]
    double sMin = 1.0, sMax = 1.0;
    uint32_t boundJoints() const { return skeleton ? jointCount : 1u; }
};

// Registration's checks and the bound data. 0, or ARK_DDGI_E_INVALID_ARGUMENT with `why`
// set and `out` untouched: a wrong struct_size, missing arrays, a skeleton without joints,
// a non-finite or negative weight, a joint index >= joint_count (a device fault if it got
// through; the reference checks none of this), non-finite bind or morph data.
int buildSkin(const ArkDdgiSkinDesc* desc, std::unique_ptr<SkinHost>& out, std::string& why);

// Rows 0-2 of `count` column-major mat4s (the reference's appliedJointMatrices) as 12
// floats each, row-major 3 x 4: a copy of words, no arithmetic.
void jointRows(const float* matrices16, uint32_t count, float* out12);

// The bound (lo xyz, hi xyz) of every position k_skin_vertices can produce for the pose:
// finite and conservative, or false with `why` (a non-finite joint matrix or morph weight,
// or a bound that is not finite). joints12: boundJoints() x 12 (ignored for a morph-only skin).
bool poseBound(const SkinHost& s, const float* joints12, const float* morphWeights, float out[6], std::string& why);

// k_skin_vertices restated serially. prev: the previous run's positions (3 n), or null on
// the skin's first run (velocity 0). outP 3 n, outV 9 n, outVel 3 n.
void skinRun(const SkinHost& s, const float* joints12, const float* morphWeights, const float* prev, float* outP, float* outV, float* outVel);

// The skins of one scene by handle (handles are not reused within a registry).
struct Registry {
    std::vector<std::unique_ptr<SkinHost>> skins;
    int add(const ArkDdgiSkinDesc* desc, uint32_t* handle, std::string& why);
    bool remove(uint32_t handle);
    const SkinHost* get(uint32_t handle) const { return handle < skins.size() ? skins[handle].get() : nullptr; }
    size_t live() const;
};

} // namespace skin
} // namespace ark
