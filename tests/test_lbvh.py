"""Host-side check of the device LBVH build's logic (csrc/lbvh_build.h, the functions the
kernels of ddgi_bvh_build.hip call) run serially by ark_ddgi_debug_lbvh_check: Morton
keys, the radix tree, the BVH2 -> BVH8 cut, slots and private rows, the planes written by
the host collapse's node writer. Same checks as test_bvh8.py's. No GPU."""
import ctypes as C

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D


def soup(n=20000):
    """test_bvh8.py's 20,000-triangle soup"""
    rng = np.random.default_rng(7)
    v0 = rng.uniform(-31, 31, (n, 3)).astype(np.float32)
    return np.concatenate([v0, v0 + rng.uniform(-0.3, 0.3, (n, 3)), v0 + rng.uniform(-0.3, 0.3, (n, 3))], axis=1)


def edge_case(case):
    """test_bvh8.py's edge cases"""
    rng = np.random.default_rng(3)
    if case == "single":
        return np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    if case == "degenerate":  # zero-area triangles and repeated points (zero-extent boxes)
        p = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
        return np.concatenate([p, p, p], axis=1)
    if case == "far":  # far from the origin: plane anchors need coarse grids
        v0 = rng.uniform(1e5, 1e5 + 10, (500, 3)).astype(np.float32)
        return np.concatenate([v0, v0 + 0.5, v0 + np.float32([0.5, 0, 0.25])], axis=1)
    if case == "tiny_far":  # boxes far smaller than one ulp step of their position
        v0 = np.full((64, 3), 3.0e6, np.float32) + rng.integers(0, 4, (64, 3)).astype(np.float32)
        return np.concatenate([v0, v0, v0], axis=1)
    assert case == "coplanar"
    xy = rng.uniform(-5, 5, (2000, 2)).astype(np.float32)
    z = np.zeros((2000, 1), np.float32)
    v0 = np.concatenate([xy, z], axis=1)
    return np.concatenate([v0, v0 + np.float32([0.1, 0, 0]), v0 + np.float32([0, 0.1, 0])], axis=1)


def _assert_valid(tris, rc, out):
    nodes, leaves, depth, violations, ntris, _, internal, _ = out
    assert rc == 0 and violations == 0, out
    assert ntris == np.asarray(tris).reshape(-1, 9).shape[0]
    assert internal == nodes - 1  # every node but the root is some node's internal child


def test_soup_lbvh_structure():
    tris = soup()
    rc, out = D.lbvh_check(tris)
    _assert_valid(tris, rc, out)
    # the SAH cost an LBVH pays, next to set_scene's binned-SAH build with the SAH-optimal collapse
    ref = (C.c_uint64 * 8)()
    a = np.ascontiguousarray(tris, np.float32)
    assert abi.load_library().ark_ddgi_debug_bvh8_check(a.ctypes.data, a.shape[0], ref) == 0
    by_count = D.lbvh_check(tris, 0)[1]
    print(f"BVH8 SAH cost, 20,000 soup: LBVH {out[7] / 1e6:.3f} ({out[0]} nodes, depth {out[2]}; opening by count "
          f"{by_count[7] / 1e6:.3f}, {by_count[0]} nodes), host build {ref[7] / 1e6:.3f} ({ref[0]} nodes, depth {ref[2]})")


@pytest.mark.parametrize("case", ["single", "degenerate", "far", "tiny_far", "coplanar"])
def test_lbvh_edge_cases(case):
    tris = edge_case(case)
    rc, out = D.lbvh_check(tris)
    _assert_valid(tris, rc, out)


@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 25, 65])
def test_lbvh_small_counts(n, criterion):
    """1-3: the root is one leaf slot; 4: the root opened once (two leaf slots); 9: one node whose
    cut ends below 8 members (none of more than 3 triangles is left to open); 25, 65: more
    than one level."""
    tris = soup(65)[:n]
    rc, out = D.lbvh_check(tris, criterion)
    _assert_valid(tris, rc, out)
    nodes, leaves, depth = out[0], out[1], out[2]
    if n <= 3:
        assert (nodes, leaves, depth) == (1, 1, 1)
    elif n == 4:
        assert (nodes, leaves, depth) == (1, 2, 1)
    elif n == 9:
        assert (nodes, depth) == (1, 1) and 3 <= leaves <= 8
    else:
        assert depth >= 2 and nodes >= 2


def test_lbvh_coincident_triangles():
    """200 copies of one triangle: every key is equal, and the radix tree splits on the
    sorted index instead (a tie left to the keys alone gives a chain 200 deep)."""
    tris = np.tile(soup(1), (200, 1))
    rc, out = D.lbvh_check(tris)
    _assert_valid(tris, rc, out)
    assert out[2] <= 16, out
