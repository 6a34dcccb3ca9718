"""The device BVH build with the SAH pass (ARK_DDGI_FLAG_GPU_REBUILD_SAH: the work list of
k_lbvh_hierarchy, k_lbvh_treelet_sah, the collapse by the pass's boxes) against its host
restatement, bit for bit and stage by stage: ark_ddgi_debug_lbvh_device_parity_sah. As
test_gpu_lbvh_parity.py, plus the treelet list as a set, the sorted record indices after the
pass, and the boxes per BVH2 node and per sorted primitive by bits. No tolerance anywhere.

test_gpu_lbvh_parity.py's inputs (three classes in turn), and one-class inputs at the pass's
edges: 4 and 5 primitives (the smallest treelets, at the leaf boundary), 65 (a segment across
a wave boundary), 256 (one treelet of exactly the workgroup's size), 257 (two treelets under
one upper node), 513."""
import functools

import numpy as np
import pytest

from arkoserenderer_amd import ddgi as D

from test_gpu_lbvh_parity import SUNS, _no_device_error, case_input
from test_lbvh import soup

pytestmark = pytest.mark.gpu

INPUTS = ["n255", "n256", "n257", "n513", "n4099", "soup", "holes", "one_record_class", "no_opaque", "degenerate", "far", "tiny_far", "coplanar",
          "coincident", "signed_zero", "flat", "one4", "one5", "one65", "one256", "one257", "one513", "coincident300"]
# (sun, w_bits) of the builds: the world's, and the light build with 18, 0 and 20 bits for w
BUILDS = {"world": (None, None), "light_w18": ("oblique", 18), "light_w0": ("oblique", 0), "light_w20": ("oblique", 20)}


@functools.lru_cache(maxsize=None)
def sah_input(name):
    """(records, class_of, primitives): test_gpu_lbvh_parity.py's, or one class of the first n of a soup"""
    if name.startswith("one") and name[3:].isdigit():
        n = int(name[3:])
        tris = soup(513)[:n]
    elif name == "coincident300":  # two treelets of equal boxes: every candidate ties
        n = 300
        tris = np.tile(soup(1), (n, 1))
    else:
        return case_input(name)
    rec = D.triangle_records(np.ascontiguousarray(tris, np.float32), np.zeros(n, np.uint32))
    rec.setflags(write=False)
    return rec, (0,), n


def _assert_clean(rc, r, prims):
    _no_device_error(rc, r)
    assert r["why"] == "", r
    for k in D.LBVH_PARITY_SAH_MISMATCHES:
        assert r[k] == 0, (k, r)
    assert rc == 0, r
    assert r["prims"] == prims and r["nodes"] == r["host_nodes"] == r["pairs"] and r["nodes"] >= 1, r


def _run(name, build):
    rec, class_of, prims = sah_input(name)
    sun, w_bits = BUILDS[build]
    rc, r = D.lbvh_device_parity(rec, class_of, None if sun is None else SUNS[sun], w_bits, sah=True)
    _assert_clean(rc, r, prims)
    return r


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", INPUTS)
def test_parity(name, build):
    r = _run(name, build)
    one_tree = build != "world" or name.startswith("one") or name == "coincident300"
    if one_tree and r["prims"] <= 256:
        assert r["treelets"] == (1 if r["prims"] > 3 else 0), r  # the root itself (256: exactly one workgroup's worth)
    if one_tree and r["prims"] in (257, 300):
        assert 1 <= r["treelets"] <= 2, r  # the two children of the one upper node (a child of 3 or fewer is none)
    if name in ("n4099", "soup"):
        assert r["treelets"] > 16 and r["depth"] >= 3, r


@pytest.mark.parametrize("build", list(BUILDS))
def test_counts_1_to_65(build):
    """Every count from 1 to 65, the three classes in turn: roots that are one leaf slot (no
    treelet), treelets of 4 and 5 at the leaf boundary, up to one across a wave boundary."""
    for n in range(1, 66):
        r = _run(f"n{n}", build)
        if build != "world":
            assert r["treelets"] == (1 if n > 3 else 0), (n, r)


@pytest.mark.parametrize("build", ["world", "light_w18"])
def test_flag_off_is_the_old_entry(build):
    """sah = 0: ark_ddgi_debug_lbvh_device_parity's words, and no treelet."""
    rec, class_of, prims = sah_input("n4099")
    sun, w_bits = BUILDS[build]
    rc0, old = D.lbvh_device_parity(rec, class_of, None if sun is None else SUNS[sun], w_bits)
    _no_device_error(rc0, old)
    rc1, new = D.lbvh_device_parity(rec, class_of, None if sun is None else SUNS[sun], w_bits, sah=False)
    _no_device_error(rc1, new)
    assert rc0 == rc1 == 0
    assert {k: new[k] for k in old} == old and new["treelets"] == 0, (old, new)
