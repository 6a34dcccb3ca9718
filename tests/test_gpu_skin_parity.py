"""k_skin_vertices (csrc/ddgi_skinning.hip) against its host restatement, by bits
(ark_ddgi_debug_skin_device_parity): positions, vertices and velocities, every count 0, and
no word written outside the outputs' ranges.

Vertex counts around the wave (64) and the workgroup (256) and several workgroups with a
tail; the outputs starting at every vertex offset mod 4 (a 12-B stride is 16-B aligned only
every fourth vertex; morph target k's rows start k n vertices in, so odd counts also move
the inputs' alignment); joint counts 1, 2, the LDS cap and the cap + 1 (the global-gather
instantiation); K in {0, 1, 3}; morph-only skins; a singular joint (NaNs equal NaNs); the
velocity of a second pose against the first pose's positions."""
import numpy as np
import pytest

from arkoserenderer_amd import ddgi as D
import skin_cases as SC

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023]
JOINTS = [1, 2, SC.LDS_JOINTS, SC.LDS_JOINTS + 1]
MORPHS = [0, 1, 3]
ZERO = dict(positions=0, vertices=0, velocities=0, outside=0)


def _counts(r):
    return {k: r[k] for k in ZERO}


def _poses(seed, joints, K):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        M = SC.column_major(SC.joint_matrices(rng, joints)) if joints else None
        out.append(D.SkinPose(0, M, rng.uniform(-1.0, 1.0, K).astype(np.float32) if K else None))
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_parity_by_bits(n):
    seed = 1000 + n
    for joints in JOINTS:
        for K in MORPHS:
            skin, _ = SC.random_skin(seed, n, joints, K)
            first_pose, second_pose = _poses(seed + 17 * joints + K, joints, K)
            p1, _, _, _ = D.skin_host(skin, first_pose)
            for first in range(4):
                # the first run (velocity 0) at one offset, the second pose against the first's positions at the others
                prev = None if first == (n + K) % 4 else p1
                r = D.skin_device_parity(skin, second_pose if prev is not None else first_pose, prev, dst_first_vertex=first)
                assert _counts(r) == ZERO, (n, joints, K, first, r)
            seed += 1


@pytest.mark.parametrize("n", [5, 257])
@pytest.mark.parametrize("K", [1, 3])
def test_morph_only_skins(n, K):
    skin, _ = SC.random_skin(2000 + n + K, n, 0, K, skeleton=False)
    a, b = _poses(7 + n, 0, K)
    p1, _, _, _ = D.skin_host(skin, a)
    for first in range(4):
        r = D.skin_device_parity(skin, b, p1 if first else None, dst_first_vertex=first)
        assert _counts(r) == ZERO, (n, K, first, r)


@pytest.mark.parametrize("joints", [3, SC.LDS_JOINTS + 1])
def test_singular_joint(joints):
    """A rank-1 joint: its vertices' normals and tangents are non-finite on both sides, their positions finite."""
    _, arr = SC.random_skin(3000 + joints, 300, joints, 1, influences=1)
    arr["joint_indices"][::5, 0] = 1  # every fifth vertex hangs on the singular joint alone
    skin = D.Skin(0, arr["positions"], arr["vertices"], arr["joint_indices"], arr["joint_weights"], joints, arr["morph_targets"])
    M = SC.joint_matrices(np.random.default_rng(5), joints)
    M[1, :3, :3] = 0.0
    M[1, 0, 0] = 1.0
    pose = D.SkinPose(0, SC.column_major(M), [0.3])
    p, v, _, _ = D.skin_host(skin, pose)
    on1 = arr["joint_indices"][:, 0] == 1
    assert on1.any() and not np.isfinite(v[on1, 2:5]).all(axis=1).any() and np.isfinite(p).all()
    r = D.skin_device_parity(skin, pose, None, dst_first_vertex=1)
    assert _counts(r) == ZERO, r


def test_unnormalised_bind_normals_without_morph_targets():
    skin, arr = SC.random_skin(4000, 130, 4, 0)
    arr["vertices"][:, 2:5] *= np.float32(2.5)
    skin = D.Skin(0, arr["positions"], arr["vertices"], arr["joint_indices"], arr["joint_weights"], 4)
    pose = _poses(9, 4, 0)[0]
    r = D.skin_device_parity(skin, pose, None, dst_first_vertex=3)
    assert _counts(r) == ZERO, r
