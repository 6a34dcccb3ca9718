"""Host-side check of the collapse plan of the device BVH builds (ARK_DDGI_FLAG_GPU_REBUILD_PLAN;
csrc/lbvh_build.h: the treelets down to single primitives, planCosts, the rounds above the
treelets, planCut) restated serially: ark_ddgi_debug_lbvh_check_plan and
ark_ddgi_debug_sun_lbvh_check_plan. test_lbvh_sah.py's inputs and structure checks (every
record the input's bit for bit is among the entries' violations); the quality assertions are
strict inequalities with no margin: the plan searches a superset of the greedy cuts over the
same binary tree. No GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D

from test_lbvh import _assert_valid, soup
from test_lbvh_sah import CASES, COUNTS, SUNS, TABLE_SUNS, city, city_20k, named
from test_sun_lbvh import _assert_clean, origins_on


def _cost_word(word):
    return struct.unpack("<f", struct.pack("<I", word & 0xFFFFFFFF))[0]


def _assert_plan(tris, rc, out):
    """_assert_valid, no internal member of at most 3 triangles, a root cost wherever the root is a node"""
    _assert_valid(tris, rc, out[:8])
    n = np.asarray(tris).reshape(-1, 9).shape[0]
    assert out[10] == 0, out
    assert (out[9] != 0) == (n > 3), out


@pytest.mark.parametrize("name", CASES)
def test_world_structure(name):
    tris = named(name)
    rc, out = D.lbvh_check(tris, sah=True, plan=True)
    _assert_plan(tris, rc, out)
    n = np.asarray(tris).reshape(-1, 9).shape[0]
    assert (out[8] >= 1) == (n > 1), out  # under the plan only single primitives lie outside a treelet
    if name.startswith("coincident"):
        assert out[2] <= 16, out


@pytest.mark.parametrize("n", COUNTS)
def test_world_counts(n):
    """1: the root one leaf slot, no treelet; 2-256: the class root one treelet (2 and 3: still
    one leaf slot); 257 and 511-514: treelets under upper nodes, which the rounds plan."""
    tris = soup(514)[:n]
    rc, out = D.lbvh_check(tris, sah=True, plan=True)
    _assert_plan(tris, rc, out)
    if n <= 3:
        assert (out[0], out[1], out[2], out[8]) == (1, 1, 1, 0 if n == 1 else 1), out
    elif n <= 256:
        assert out[8] == 1, out
    else:
        assert out[8] >= 2, out


@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("name", CASES)
def test_sun_structure_rays_inflation(name, sun):
    tris = named(name)
    rc, r = D.sun_lbvh_check(tris, SUNS[sun], origins_on(tris, 512 if name == "soup" else 128), sah=True, plan=True)
    _assert_clean(tris, rc, r)
    assert r["small_internal"] == 0, r
    if name.startswith("coincident"):
        assert r["depth"] <= 16, r


@pytest.mark.parametrize("w_bits", [18, 0, 20])
@pytest.mark.parametrize("n", COUNTS)
def test_sun_counts(n, w_bits):
    tris = soup(514)[:n]
    rc, r = D.sun_lbvh_check(tris, SUNS["oblique"], origins_on(tris, 64), w_bits=w_bits, sah=True, plan=True)
    _assert_clean(tris, rc, r)
    assert r["small_internal"] == 0, r
    if n <= 256:
        assert r["treelets"] == (0 if n == 1 else 1), r
    else:
        assert r["treelets"] >= 2, r


@pytest.mark.parametrize("name", ["soup", "city", "city_20k"])
def test_world_sah_cost_falls(name):
    """The BVH8 SAH cost of the opaque class (out[7]) with the plan against the SAH pass alone."""
    tris = soup() if name == "soup" else city() if name == "city" else city_20k()[0]
    rc0, sah = D.lbvh_check(tris, sah=True, plan=False)
    rc1, plan = D.lbvh_check(tris, sah=True, plan=True)
    assert rc0 == 0 and rc1 == 0
    _assert_plan(tris, rc1, plan)
    print(f"BVH8 SAH cost, {name} ({tris.shape[0]} triangles): with the SAH pass {sah[7] / 1e6:.3f} ({sah[0]} nodes, depth {sah[2]}), "
          f"with the plan {plan[7] / 1e6:.3f} ({plan[0]} nodes, depth {plan[2]}, {plan[8]} treelets; the plan's own root cost {_cost_word(plan[9]):.6g})")
    assert plan[7] < sah[7], (plan, sah)


def test_world_sah_cost_on_the_soup_is_below_the_host_builds():
    tris = np.ascontiguousarray(soup(), np.float32)
    host = (C.c_uint64 * 8)()
    assert abi.load_library().ark_ddgi_debug_bvh8_check(tris.ctypes.data, tris.shape[0], host) == 0
    rc0, sah = D.lbvh_check(tris, sah=True, plan=False)
    rc1, plan = D.lbvh_check(tris, sah=True, plan=True)
    assert rc0 == 0 and rc1 == 0
    print(f"BVH8 SAH cost, 20,000 soup: with the SAH pass {sah[7] / 1e6:.3f}, with the plan {plan[7] / 1e6:.3f}, host build {host[7] / 1e6:.3f}")
    assert plan[7] < host[7], (plan, list(host))


@pytest.mark.parametrize("name", ["city", "city_20k", "soup"])
def test_sun_shadow_cost_is_reported(name):
    """sun_shadow_cost (any-hit steps per ray, 4,096 origins on the triangles) with the plan: printed,
    not asserted - surface-area criteria can cost the soup's sun rays."""
    if name == "city_20k":
        tris, sun = city_20k()
        suns = {"its own": sun}
    else:
        tris, suns = (city() if name == "city" else soup()), TABLE_SUNS
    org = origins_on(tris, 4096)
    for label, sun in suns.items():
        rc0, sah = D.sun_lbvh_check(tris, sun, org, sah=True, plan=False)
        rc1, plan = D.sun_lbvh_check(tris, sun, org, sah=True, plan=True)
        _assert_clean(tris, rc0, sah)
        _assert_clean(tris, rc1, plan)
        print(f"sun {label}, {name}: any-hit steps per ray with the SAH pass {sah['cost_lbvh']:.2f}, with the plan {plan['cost_lbvh']:.2f}, "
              f"host build {plan['cost_host']:.2f} ({sah['nodes']} / {plan['nodes']} nodes)")


@pytest.mark.parametrize("name", CASES)
def test_flag_clear_is_the_sah_entries_word_for_word(name):
    lib = abi.load_library()
    tris = np.ascontiguousarray(named(name), np.float32).reshape(-1, 9)
    for sah in (0, 1):
        old, new = (C.c_uint64 * 9)(), (C.c_uint64 * 11)()
        rc_old = lib.ark_ddgi_debug_lbvh_check_sah(tris.ctypes.data, tris.shape[0], 1, sah, old)
        rc_new = lib.ark_ddgi_debug_lbvh_check_plan(tris.ctypes.data, tris.shape[0], 1, sah, 0, new)
        assert rc_old == rc_new == 0 and list(old) == list(new)[:9] and new[9] == 0 and new[10] == 0, (list(old), list(new))
    # the flag without the SAH pass does nothing
    plain, alone = (C.c_uint64 * 9)(), (C.c_uint64 * 11)()
    assert lib.ark_ddgi_debug_lbvh_check_sah(tris.ctypes.data, tris.shape[0], 1, 0, plain) == 0
    assert lib.ark_ddgi_debug_lbvh_check_plan(tris.ctypes.data, tris.shape[0], 1, 0, 1, alone) == 0
    assert list(plain) == list(alone)[:9] and alone[9] == 0
    org = origins_on(tris, 128)
    sd = np.asarray(SUNS["oblique"], np.float32)
    for w_bits in (18, 0, 20):
        old, new = (C.c_uint64 * 17)(), (C.c_uint64 * 19)()
        rc_old = lib.ark_ddgi_debug_sun_lbvh_check_sah(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], 1e30, w_bits, 1, old)
        rc_new = lib.ark_ddgi_debug_sun_lbvh_check_plan(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], 1e30, w_bits, 1, 0, new)
        assert rc_old == rc_new == 0 and list(old) == list(new)[:17] and new[17] == 0, (list(old), list(new))


def test_config_flag():
    """DDGIConfig.gpu_rebuild_plan sets ARK_DDGI_FLAG_GPU_REBUILD_PLAN (0x80) and nothing else."""
    grid = D.ProbeGrid((4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert abi.ARK_DDGI_FLAG_GPU_REBUILD_PLAN == 0x80 and not D.DDGIConfig().gpu_rebuild_plan
    off = D.desc_for(grid, 100.0, D.DDGIConfig()).flags
    on = D.desc_for(grid, 100.0, D.DDGIConfig(gpu_rebuild_plan=True)).flags
    assert on == off | 0x80
