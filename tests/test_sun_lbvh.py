"""Host-side check of the device build of the sun's light-space BVH8
(ARK_DDGI_FLAG_GPU_REBUILD_SUN; csrc/lbvh_build.h: the light vertices, the light-space key,
the slots in ascending w) run serially by ark_ddgi_debug_sun_lbvh_check: the structure, the
records, the boxes' inflation against the host build's, and a sun shadow ray from points
on the triangles through the tree against brute force. test_lbvh.py's inputs. No GPU."""
import ctypes as C

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D

from test_lbvh import edge_case, soup

SUNS = {"oblique": (0.3, -1.0, -0.4), "axis": (0.0, -1.0, 0.0)}


def origins_on(tris, n=512, seed=11):
    """Points on the triangles (uniform barycentrics), as sun_sample_origins takes them"""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(t), n)
    r1, r2 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    sq = np.sqrt(r1)
    b0, b1, b2 = 1 - sq, sq * (1 - r2), sq * r2
    return (b0[:, None] * t[k, 0] + b1[:, None] * t[k, 1] + b2[:, None] * t[k, 2]).astype(np.float32)


def _assert_clean(tris, rc, r):
    assert rc == 0, r
    assert r["mismatches"] == 0 and r["violations"] == 0 and r["inflation_differs"] == 0, r
    assert r["occluded_bvh"] == r["occluded_brute"]


@pytest.mark.parametrize("sun", list(SUNS))
def test_soup(sun):
    """The 20,000 soup: structure, records, inflation, rays; the slots of every node ascend
    in the low w edge of their Morton cells (counted among the violations)."""
    tris = soup()
    org = origins_on(tris, 1024)
    rc, r = D.sun_lbvh_check(tris, SUNS[sun], org)
    _assert_clean(tris, rc, r)
    assert r["rays"] == 1024 and r["nodes"] > 1 and r["depth"] >= 2
    assert r["w_bits"] == 18  # the default split, 21 / 21 / 18 (EXPERIMENTS.md "Device LBVH build")
    print(f"sun {sun}, 20,000 soup: any-hit steps per ray LBVH {r['cost_lbvh']:.2f}, host build {r['cost_host']:.2f} "
          f"({r['nodes']} nodes, depth {r['depth']}, {r['occluded_brute']} of {r['rays']} rays occluded)")


def test_plain_entry_point_matches_opts():
    """ark_ddgi_debug_sun_lbvh_check is the _opts variant at the default split: out[12]."""
    tris = np.ascontiguousarray(soup(500), np.float32)
    org = origins_on(tris, 64)
    sd = np.asarray(SUNS["oblique"], np.float32)
    out = (C.c_uint64 * 12)()
    rc = abi.load_library().ark_ddgi_debug_sun_lbvh_check(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], 1e30, out)
    rc2, r = D.sun_lbvh_check(tris, sd, org)
    assert rc == 0 and rc2 == 0
    assert [int(v) for v in out[:4]] == [r["rays"], r["occluded_brute"], r["occluded_bvh"], r["mismatches"]]
    assert int(out[6]) == r["nodes"] and int(out[8]) == 0 and int(out[9]) == 0
    assert int(out[10]) == round(r["cost_lbvh"] * 1e6) and int(out[11]) == round(r["cost_host"] * 1e6)


@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("case", ["single", "degenerate", "far", "tiny_far", "coplanar"])
def test_edge_cases(case, sun):
    tris = edge_case(case)
    rc, r = D.sun_lbvh_check(tris, SUNS[sun], origins_on(tris, 256))
    _assert_clean(tris, rc, r)


@pytest.mark.parametrize("w_bits", [18, 20, 12, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 25, 65])
def test_small_counts(n, w_bits):
    """test_lbvh_small_counts' expectations: 1-3 the root is one leaf slot; 4 the root opened
    once; 9 one node whose cut ends below 8 members; 25, 65 more than one level."""
    tris = soup(65)[:n]
    rc, r = D.sun_lbvh_check(tris, SUNS["oblique"], origins_on(tris, 64), w_bits=w_bits)
    _assert_clean(tris, rc, r)
    nodes, leaves, depth = r["nodes"], r["leaf_children"], r["depth"]
    if n <= 3:
        assert (nodes, leaves, depth) == (1, 1, 1)
    elif n == 4:
        assert (nodes, leaves, depth) == (1, 2, 1)
    elif n == 9:
        assert (nodes, depth) == (1, 1) and 3 <= leaves <= 8
    else:
        assert depth >= 2 and nodes >= 2


def test_coincident_triangles():
    """200 copies of one triangle: every key is equal, the radix tree splits on the index."""
    tris = np.tile(soup(1), (200, 1))
    rc, r = D.sun_lbvh_check(tris, SUNS["oblique"], origins_on(tris, 64))
    _assert_clean(tris, rc, r)
    assert r["depth"] <= 16, r


def test_invalid_split_is_a_build_error():
    tris = soup(16)
    rc, _ = D.sun_lbvh_check(tris, SUNS["oblique"], origins_on(tris, 4), w_bits=13)
    assert rc == 1
