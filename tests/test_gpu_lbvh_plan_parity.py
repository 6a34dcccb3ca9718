"""The device BVH build with the collapse plan (ARK_DDGI_FLAG_GPU_REBUILD_PLAN on top of the
SAH pass: k_lbvh_hierarchy's second list, the plan instance of k_lbvh_treelet_sah,
k_lbvh_upper_plan, the collapse by lbvh::planCut) against its host restatement, bit for bit
and stage by stage: ark_ddgi_debug_lbvh_device_parity_plan. As test_gpu_lbvh_sah_parity.py,
plus the packed picks at every node index, the eight cost words of every treelet root and
upper node, the upper nodes' boxes and the upper list as a set. No tolerance anywhere.

test_gpu_lbvh_parity.py's inputs (three classes in turn) for the world build and for the light
build under its three suns; the counts sit at the plan's edges: 2 and 3 (treelets that stay
one leaf slot), 4 (the smallest internal member), 64 / 65 (a wave's edge), 255 / 256 (one
treelet, no upper node), 257 and 513 (treelets and single primitives under upper nodes)."""
import pytest

from arkoserenderer_amd import ddgi as D

from test_gpu_lbvh_parity import SUNS, _no_device_error
from test_gpu_lbvh_sah_parity import sah_input

pytestmark = pytest.mark.gpu

INPUTS = ["n64", "n65", "n255", "n256", "n257", "n513", "n4099", "soup", "holes", "one_record_class", "no_opaque", "degenerate", "far", "tiny_far",
          "coplanar", "coincident", "coincident300", "signed_zero", "flat", "one256", "one257", "one513"]
# (sun, w_bits) of the builds: the world's, and the light build under the three suns
BUILDS = {"world": (None, None), "light_oblique": ("oblique", 18), "light_down": ("down", 0), "light_grazing": ("grazing", 20)}


def _assert_clean(rc, r, prims):
    _no_device_error(rc, r)
    assert r["why"] == "", r
    for k in D.LBVH_PARITY_PLAN_MISMATCHES:
        assert r[k] == 0, (k, r)
    assert rc == 0, r
    assert r["prims"] == prims and r["nodes"] == r["host_nodes"] == r["pairs"] and r["nodes"] >= 1, r


def _run(name, build):
    rec, class_of, prims = sah_input(name)
    sun, w_bits = BUILDS[build]
    rc, r = D.lbvh_device_parity(rec, class_of, None if sun is None else SUNS[sun], w_bits, sah=True, plan=True)
    _assert_clean(rc, r, prims)
    return r


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", INPUTS)
def test_parity(name, build):
    r = _run(name, build)
    one_tree = build != "world" or name.startswith("one") or name == "coincident300"
    if one_tree and r["prims"] <= 256:
        assert r["treelets"] == 1 and r["upper_nodes"] == 0, r  # the root itself; nothing above it
    if one_tree and r["prims"] > 256:
        assert r["upper_nodes"] >= 1 and r["upper_rounds"] >= 1, r
    if name in ("n4099", "soup"):
        assert r["treelets"] > 16 and r["upper_nodes"] > 8 and r["depth"] >= 3, r


@pytest.mark.parametrize("build", list(BUILDS))
def test_counts_1_to_9(build):
    """1: no treelet; 2 and 3: a treelet whose root stays one leaf slot; 4 to 9: the smallest trees with a cut to plan."""
    for n in range(1, 10):
        r = _run(f"n{n}", build)
        if build != "world":
            assert r["treelets"] == (1 if n > 1 else 0) and r["upper_nodes"] == 0, (n, r)


@pytest.mark.parametrize("build", ["world", "light_oblique"])
def test_flag_clear_is_the_sah_entry(build):
    """plan = 0: ark_ddgi_debug_lbvh_device_parity_sah's words; the flag without the SAH pass: the plain entry's."""
    rec, class_of, prims = sah_input("n4099")
    sun, w_bits = BUILDS[build]
    sd = None if sun is None else SUNS[sun]
    rc0, old = D.lbvh_device_parity(rec, class_of, sd, w_bits, sah=True)
    _no_device_error(rc0, old)
    rc1, new = D.lbvh_device_parity(rec, class_of, sd, w_bits, sah=True, plan=False)
    _no_device_error(rc1, new)
    assert rc0 == rc1 == 0
    assert {k: new[k] for k in old} == old and new["upper_nodes"] == 0, (old, new)
    rc2, plain = D.lbvh_device_parity(rec, class_of, sd, w_bits, sah=False)
    _no_device_error(rc2, plain)
    rc3, alone = D.lbvh_device_parity(rec, class_of, sd, w_bits, sah=False, plan=True)
    _no_device_error(rc3, alone)
    assert rc2 == rc3 == 0
    assert {k: alone[k] for k in plain} == plain and alone["treelets"] == 0 and alone["upper_nodes"] == 0, (plain, alone)
