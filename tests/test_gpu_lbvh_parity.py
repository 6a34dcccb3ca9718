"""The device LBVH build (csrc/ddgi_bvh_build.hip's kernels, the rocPRIM sort and the refit over
every level, driven by buildLbvhGpu) against its host restatement (build_lbvh_host), bit for
bit and stage by stage: ark_ddgi_debug_lbvh_device_parity runs one traced device build of the
given records, hands the device's compaction order - the only legitimately nondeterministic
quantity - to the host restatement and compares the header, the sorted keys and indices, the
splits and the two trees in canonical form. No tolerance anywhere: equality of bits (== of
floats for the header box, whose zeros' signs the two sides reduce differently).

The inputs are sized for the kernels' edges, not for the workload: the root shapes of
test_lbvh.py, the 256-thread block edge of the prims / keys / hierarchy kernels and the
128-thread edge of the collapse, holes (a whole wave of them), empty and one-record classes,
equal keys, signed zeros and a flat scene box."""
import functools

import numpy as np
import pytest

from arkoserenderer_amd import ddgi as D

from test_lbvh import edge_case, soup

pytestmark = pytest.mark.gpu

THREE_CLASSES = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def case_input(name):
    """(records, class_of, primitives) of a named input, built once"""
    class_of = THREE_CLASSES
    holes = None
    if name[0] == "n" and name[1:].isdigit():  # the first n of one soup, so that the counts nest
        n = int(name[1:])
        tris = soup(65)[:n] if n <= 65 else soup(4099)[:n]
    elif name == "soup":
        tris = soup()
    elif name == "holes":
        # a third of the records holes, interleaved, and records 640 .. 703 - one whole wave of
        # the prims kernels - holes as well
        tris = soup(3000)
        holes = np.arange(3000) % 3 == 1
        holes[640:704] = True
    elif name == "one_record_class":  # class 0 holds one record, class 1 none
        tris = soup(500)
        class_of = (0, 2, 2)
    elif name == "no_opaque":  # no opaque record: no root 0, no opaque nodes
        tris = soup(500)
        class_of = (1, 2, 2)
    elif name == "coincident":  # 200 copies of one triangle: every key equal
        tris = np.tile(soup(1), (200, 1))
    elif name == "signed_zero":
        # the least x of the scene is reached as -0.0 and as +0.0, in two waves and within one
        tris = np.abs(soup(300)).astype(np.float32)
        tris[:, 3] += 1.0
        tris[:, 6] += 1.0
        tris[[5, 200, 210], 0] = np.float32([-0.0, 0.0, -0.0])
    elif name == "flat":  # a scene box of extent 0 along y: key scale 0
        tris = soup(500).astype(np.float32)
        tris[:, [1, 4, 7]] = np.float32(2.5)
    else:
        tris = edge_case(name)
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    n = tris.shape[0]
    if name in ("one_record_class", "no_opaque"):
        instances = np.where(np.arange(n) == 0, 0, 1 + np.arange(n) % 2)
    else:
        instances = np.arange(n) % 3
    rec = D.triangle_records(tris, instances, holes)
    rec.setflags(write=False)
    return rec, class_of, n - (int(holes.sum()) if holes is not None else 0)


INPUTS = ["n1", "n2", "n3", "n4", "n9", "n25", "n65", "n255", "n256", "n257", "n4099", "soup", "holes", "one_record_class", "no_opaque", "degenerate",
          "far", "tiny_far", "coplanar", "coincident", "signed_zero", "flat"]
SUNS = {
    "oblique": tuple(np.float32([0.3, -1.0, -0.4]) / np.linalg.norm(np.float32([0.3, -1.0, -0.4]))),
    "down": (0.0, -1.0, 0.0),
    "grazing": (float(np.cos(np.radians(0.5))), float(-np.sin(np.radians(0.5))), 0.0),  # half a degree below horizontal
}


def _no_device_error(rc, r):
    print(rc, r)
    if r["hip_error"] != 0:
        pytest.exit(f"HIP error {r['hip_error']} from the device build: nothing more is launched ({r})", returncode=3)
    assert rc >= 0, r


def _assert_clean(rc, r, prims):
    _no_device_error(rc, r)
    assert r["why"] == "", r
    for k in D.LBVH_PARITY_MISMATCHES:
        assert r[k] == 0, (k, r)
    assert rc == 0, r
    assert r["prims"] == prims and r["nodes"] == r["host_nodes"] == r["pairs"] and r["nodes"] >= 1, r


@pytest.mark.parametrize("name", INPUTS)
def test_world_build(name):
    rec, class_of, prims = case_input(name)
    rc, r = D.lbvh_device_parity(rec, class_of)
    _assert_clean(rc, r, prims)
    if name in ("n1", "n2", "n3"):
        assert (r["nodes"], r["depth"]) == (int(name[1:]), 1), r  # one record a class: each class's root one leaf slot
    if name in ("n4099", "soup"):
        assert r["depth"] >= 3 and r["nodes"] > 300, r  # levels of more than 128 nodes: several blocks of the collapse


@pytest.mark.parametrize("w_bits", [None, 0, 20])
@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("name", INPUTS)
def test_light_build(name, sun, w_bits):
    rec, class_of, prims = case_input(name)
    rc, r = D.lbvh_device_parity(rec, class_of, SUNS[sun], w_bits)
    _assert_clean(rc, r, prims)


@pytest.mark.parametrize("sun", [None, "oblique"])
def test_unknown_instance_is_left_to_the_host(sun):
    """A record of an instance the build does not know: the kernels' guarded error path. The
    device builds nothing and names the reason; nothing is compared."""
    rec = case_input("n257")[0].copy()
    rec[100, 9] = 3  # instances 0 .. 2 exist
    rc, r = D.lbvh_device_parity(rec, THREE_CLASSES, None if sun is None else SUNS[sun])
    _no_device_error(rc, r)
    assert rc == 2, r
    assert r["why"] == "record of an unknown instance", r
    assert r["nodes"] == 0 and r["records_with_holes"] == 0, r


@pytest.mark.parametrize("sun", [None, "oblique"])
def test_same_input_twice(sun):
    """Two builds of the 20,000 soup in one process: each equals the host restatement in its
    own compaction order, so the two are canonically equal to each other."""
    rec, class_of, prims = case_input("soup")
    runs = []
    for _ in range(2):
        rc, r = D.lbvh_device_parity(rec, class_of, None if sun is None else SUNS[sun])
        _assert_clean(rc, r, prims)
        runs.append((r["nodes"], r["records_with_holes"], r["depth"]))
    assert runs[0] == runs[1], runs
