"""The host restatement of the skinning pass (csrc/skinning.h through
ark_ddgi_debug_skin_host; no GPU) against a float64 evaluation of skinning.comp:35-98 written
independently (skin_cases.reference_f64).

Positions, per coordinate: within (16 + 4 K) 2^-24 sum_j sum_c |w_j M_j,rc p_c|. 16 2^-24 is
gamma_8 of the two four-term chains (the joint blend, then the row of A (p, 1)) with a factor
2 of slack; the K morph steps before them put at most 2 K more rounding factors on every
term (a product and a sum per step), gamma_2K, again with a factor 2: 4 K 2^-24. The sum runs
over the translation's term too (c = 3, p_3 = 1), which is a term of the same chain, and p_c
stands for the morphed position's own term magnitudes |p_c| + sum_k |d_k,c m_k|.

Normals and tangents: the joints are rotations times a uniform scale in [0.5, 2], each
within 0.6 rad of a common rotation as a posed skeleton's are (skin_cases.joint_matrices), so
the blended matrices stay well-conditioned. The restatement's greatest relative error
against float64 measured here on the CPU over the cases below is 3.02e-7 (normals 3.02e-7 in
test_skeleton_only[1], tangents 2.89e-7 in test_skeleton_and_morph[8]); the tests assert 4 x
that, 1.21e-6. The margin guards the meaning of the formulas on a fixed input, not
their rounding, which the bitwise GPU comparison pins (test_gpu_skin_parity.py)."""
import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import skin_cases as SC

U = 2.0 ** -24
NORMAL_REL_MEASURED = 3.02e-7
NORMAL_REL_BOUND = 4 * NORMAL_REL_MEASURED


def _check(arr, skin, M, mw, K, what):
    pose = D.SkinPose(0, None if M is None else SC.column_major(M), mw)
    p, v, vel, bounds = D.skin_host(skin, pose)
    P, N, T, _, terms = SC.reference_f64(arr, M, mw)
    err = np.abs(p.astype(np.float64) - P)
    tol = (16 + 4 * K) * U * terms if M is not None else 4 * K * U * terms
    print(f"{what}: greatest position error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), (what, float(np.max(err / np.maximum(tol, 1e-300))))
    rel = {}
    for name, got, want in (("normal", v[:, 2:5], N), ("tangent", v[:, 5:8], T)):
        rel[name] = float(np.max(np.linalg.norm(got.astype(np.float64) - want, axis=1) / np.linalg.norm(want, axis=1)))
    print(f"{what}: greatest relative error normal {rel['normal']:.3e} tangent {rel['tangent']:.3e}")
    assert rel["normal"] <= NORMAL_REL_BOUND and rel["tangent"] <= NORMAL_REL_BOUND, (what, rel)
    # uv and the tangent's w pass through
    assert np.array_equal(v[:, 0:2], arr["vertices"][:, 0:2]) and np.array_equal(v[:, 8], arr["vertices"][:, 8])
    assert np.all(vel == 0)
    # the host bound holds every position
    assert np.all(p >= bounds[:3]) and np.all(p <= bounds[3:]), what
    return p


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_skeleton_only(seed):
    skin, arr = SC.random_skin(seed, 500, 7, 0)
    M = SC.joint_matrices(np.random.default_rng(100 + seed), 7)
    _check(arr, skin, M, None, 0, "skeleton only")


@pytest.mark.parametrize("seed", [4, 5])
def test_morph_only(seed):
    skin, arr = SC.random_skin(seed, 500, 0, 3, skeleton=False)
    _check(arr, skin, None, [0.7, -0.4, 1.3], 3, "morph only")


@pytest.mark.parametrize("seed", [6, 7, 8])
def test_skeleton_and_morph(seed):
    skin, arr = SC.random_skin(seed, 500, 5, 2)
    M = SC.joint_matrices(np.random.default_rng(200 + seed), 5)
    _check(arr, skin, M, [0.9, -0.6], 2, "skeleton and morph")


def test_no_morph_targets_leave_a_bind_normal_unnormalised():
    """K = 0: the shader skips :46-65 altogether, so a bind normal of length 3 under an
    identity joint comes out with length 3."""
    skin, arr = SC.random_skin(9, 64, 2, 0)
    arr["vertices"][:, 2:5] *= np.float32(3.0)
    skin = D.Skin(0, arr["positions"], arr["vertices"], arr["joint_indices"], arr["joint_weights"], 2)
    M = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    _, v, _, _ = D.skin_host(skin, D.SkinPose(0, SC.column_major(M)))
    assert np.allclose(np.linalg.norm(v[:, 2:5], axis=1), 3.0, rtol=1e-5)
    # with a morph target, even of weight 0, it is renormalised
    skin2 = D.Skin(0, arr["positions"], arr["vertices"], arr["joint_indices"], arr["joint_weights"], 2, np.zeros((1, 64, 9), np.float32))
    _, v2, _, _ = D.skin_host(skin2, D.SkinPose(0, SC.column_major(M), [0.0]))
    assert np.allclose(np.linalg.norm(v2[:, 2:5], axis=1), 1.0, rtol=1e-5)


def test_velocity_is_zero_first_then_the_difference():
    skin, arr = SC.random_skin(10, 200, 4, 1)
    rng = np.random.default_rng(11)
    M1, M2 = SC.joint_matrices(rng, 4), SC.joint_matrices(rng, 4)
    p1, _, vel1, _ = D.skin_host(skin, D.SkinPose(0, SC.column_major(M1), [0.2]))
    assert np.all(vel1 == 0)
    p2, _, vel2, _ = D.skin_host(skin, D.SkinPose(0, SC.column_major(M2), [0.5]), p1)
    assert np.array_equal(vel2, p2 - p1) and np.any(vel2 != 0)


def test_singular_joint_gives_non_finite_normals_and_finite_positions():
    skin, arr = SC.random_skin(12, 100, 3, 0, influences=1)
    M = SC.joint_matrices(np.random.default_rng(13), 3)
    M[1, :3, :3] = 0.0
    M[1, 0, 0] = 1.0  # rank 1
    p, v, _, bounds = D.skin_host(skin, D.SkinPose(0, SC.column_major(M)))
    on1 = arr["joint_indices"][:, 0] == 1
    assert on1.any() and (~on1).any()
    assert np.all(np.isfinite(p)) and np.all(p >= bounds[:3]) and np.all(p <= bounds[3:])
    assert not np.any(np.isfinite(v[on1, 2:5]).all(axis=1))
    assert np.all(np.isfinite(v[~on1, 2:8]))


def test_refused_skins_and_poses():
    skin, arr = SC.random_skin(14, 32, 3, 1)
    M = SC.column_major(SC.joint_matrices(np.random.default_rng(15), 3))
    bad = M.copy()
    bad[2, 1, 1] = np.nan
    for pose in (D.SkinPose(0, bad, [0.1]), D.SkinPose(0, M, [np.inf]), D.SkinPose(0, None, [0.1]), D.SkinPose(0, M, None)):
        with pytest.raises(abi.ArkDdgiError):
            D.skin_host(skin, pose)
    ji = arr["joint_indices"].copy()
    ji[5, 2] = 3  # >= joint_count
    jw = arr["joint_weights"].copy()
    jw[7, 0] = -0.25
    P = arr["positions"].copy()
    P[3, 1] = np.inf
    for s in (D.Skin(0, arr["positions"], arr["vertices"], ji, arr["joint_weights"], 3), D.Skin(0, arr["positions"], arr["vertices"], arr["joint_indices"], jw, 3),
              D.Skin(0, P, arr["vertices"], arr["joint_indices"], arr["joint_weights"], 3), D.Skin(0, arr["positions"], arr["vertices"])):
        with pytest.raises(abi.ArkDdgiError):
            D.skin_host(s, D.SkinPose(0, M, None))
