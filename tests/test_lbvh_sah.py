"""Host-side check of the SAH pass of the device BVH builds (ARK_DDGI_FLAG_GPU_REBUILD_SAH;
csrc/lbvh_build.h: the treelets of at most 256 primitives, the three-axis sweep, the split
choice, the collapse by the pass's boxes) restated serially: ark_ddgi_debug_lbvh_check_sah
and ark_ddgi_debug_sun_lbvh_check_sah. test_lbvh.py's and test_sun_lbvh.py's inputs and
structure checks (every record the input's bit for bit is among the entries' violations);
the quality assertions are strict inequalities against the same build without the pass,
with no margin. No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S

from test_lbvh import _assert_valid, edge_case, soup
from test_sun_bvh import _world_triangles
from test_sun_lbvh import _assert_clean, origins_on

# test_gpu_lbvh_parity.py's three suns
SUNS = {
    "oblique": tuple(np.float32([0.3, -1.0, -0.4]) / np.linalg.norm(np.float32([0.3, -1.0, -0.4]))),
    "down": (0.0, -1.0, 0.0),
    "grazing": (float(np.cos(np.radians(0.5))), float(-np.sin(np.radians(0.5))), 0.0),
}
# the two suns of EXPERIMENTS.md's light-space key table
TABLE_SUNS = {"oblique": (0.3, -1.0, -0.4), "axis": (0.0, -1.0, 0.0)}
COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 511, 512, 513, 514]


@functools.lru_cache(maxsize=None)
def city():
    t = _world_triangles(S.city_block(512, 40.0))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def city_20k():
    """test_gpu_bvh_build_sah.py's scene: 19,802 triangles, and its sun"""
    sc = S.city_block(1650, 72.0)
    t = _world_triangles(sc)
    t.setflags(write=False)
    return t, tuple(float(x) for x in sc.sun[1])


def named(name):
    if name == "soup":
        return soup()
    if name == "coincident":
        return np.tile(soup(1), (200, 1))
    if name == "coincident_300":  # more than one treelet of equal boxes
        return np.tile(soup(1), (300, 1))
    return edge_case(name)


CASES = ["soup", "single", "degenerate", "far", "tiny_far", "coplanar", "coincident", "coincident_300"]


@pytest.mark.parametrize("name", CASES)
def test_world_structure(name):
    tris = named(name)
    rc, out = D.lbvh_check(tris, sah=True)
    _assert_valid(tris, rc, out[:8])
    n = np.asarray(tris).reshape(-1, 9).shape[0]
    assert (out[8] >= 1) == (n > 3), out  # a treelet wherever the collapse has a node to open
    if name.startswith("coincident"):
        assert out[2] <= 16, out  # the tie rule: equal boxes split in the middle, no 1 | n - 1 chain


@pytest.mark.parametrize("n", COUNTS)
def test_world_counts(n):
    """1-3: the root one leaf slot, no treelet; 4-9: the root one treelet; 255, 256: the class
    root a treelet of its own; 257 and 511-514: treelets under upper nodes of the radix tree."""
    tris = soup(514)[:n]
    rc, out = D.lbvh_check(tris, sah=True)
    _assert_valid(tris, rc, out[:8])
    if n <= 3:
        assert (out[0], out[1], out[2], out[8]) == (1, 1, 1, 0)
    elif n <= 256:
        assert out[8] == 1, out
    else:
        assert out[8] >= 2, out


def test_one_record_class_root_is_no_treelet():
    """A class of one record: its root is one leaf slot and the pass leaves it alone."""
    rc, out = D.lbvh_check(soup(1), sah=True)
    assert rc == 0 and (out[0], out[1], out[8]) == (1, 1, 0), out


@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("name", CASES)
def test_sun_structure_rays_inflation(name, sun):
    tris = named(name)
    rc, r = D.sun_lbvh_check(tris, SUNS[sun], origins_on(tris, 512 if name == "soup" else 128), sah=True)
    _assert_clean(tris, rc, r)
    if name.startswith("coincident"):
        assert r["depth"] <= 16, r


@pytest.mark.parametrize("w_bits", [18, 0, 20])
@pytest.mark.parametrize("n", COUNTS)
def test_sun_counts(n, w_bits):
    tris = soup(514)[:n]
    rc, r = D.sun_lbvh_check(tris, SUNS["oblique"], origins_on(tris, 64), w_bits=w_bits, sah=True)
    _assert_clean(tris, rc, r)
    if n <= 256:
        assert r["treelets"] == (0 if n <= 3 else 1), r
    else:
        assert r["treelets"] >= 2, r


@pytest.mark.parametrize("name", ["soup", "city", "city_20k"])
def test_world_sah_cost_falls(name):
    """The BVH8 SAH cost of the opaque class (out[7]) with the pass against without it."""
    tris = soup() if name == "soup" else city() if name == "city" else city_20k()[0]
    rc0, plain = D.lbvh_check(tris, sah=False)
    rc1, sah = D.lbvh_check(tris, sah=True)
    assert rc0 == 0 and rc1 == 0
    print(f"BVH8 SAH cost, {name} ({tris.shape[0]} triangles): LBVH {plain[7] / 1e6:.3f} ({plain[0]} nodes, depth {plain[2]}), "
          f"with the SAH pass {sah[7] / 1e6:.3f} ({sah[0]} nodes, depth {sah[2]}, {sah[8]} treelets)")
    assert sah[7] < plain[7], (sah, plain)


@pytest.mark.parametrize("sun", list(TABLE_SUNS))
def test_sun_shadow_cost_falls_on_the_city_block(sun):
    """sun_shadow_cost (any-hit steps per ray, 4,096 origins on the triangles) with the pass
    against without it."""
    tris = city()
    org = origins_on(tris, 4096)
    rc0, plain = D.sun_lbvh_check(tris, TABLE_SUNS[sun], org, sah=False)
    rc1, sah = D.sun_lbvh_check(tris, TABLE_SUNS[sun], org, sah=True)
    _assert_clean(tris, rc0, plain)
    _assert_clean(tris, rc1, sah)
    print(f"sun {sun}, city_block(512, 40.0): any-hit steps per ray LBVH {plain['cost_lbvh']:.2f}, with the SAH pass {sah['cost_lbvh']:.2f}, "
          f"host build {sah['cost_host']:.2f} ({plain['nodes']} / {sah['nodes']} nodes)")
    assert sah["cost_lbvh"] < plain["cost_lbvh"], (sah, plain)


def test_sun_shadow_cost_falls_on_the_gpu_tests_scene():
    """city_block(1650, 72.0) under its own sun: what test_gpu_bvh_build_sah.py's shadow rays trace."""
    tris, sun = city_20k()
    org = origins_on(tris, 4096)
    rc0, plain = D.sun_lbvh_check(tris, sun, org, sah=False)
    rc1, sah = D.sun_lbvh_check(tris, sun, org, sah=True)
    _assert_clean(tris, rc0, plain)
    _assert_clean(tris, rc1, sah)
    print(f"city_block(1650, 72.0), its sun: any-hit steps per ray LBVH {plain['cost_lbvh']:.2f}, with the SAH pass {sah['cost_lbvh']:.2f}, host build {sah['cost_host']:.2f}")
    assert sah["cost_lbvh"] < plain["cost_lbvh"], (sah, plain)


@pytest.mark.parametrize("sun", list(TABLE_SUNS))
def test_sun_shadow_cost_on_the_soup_is_reported(sun):
    """The soup's figure for EXPERIMENTS.md's table (no assertion on it is asked for)."""
    tris = soup()
    org = origins_on(tris, 4096)
    _, plain = D.sun_lbvh_check(tris, TABLE_SUNS[sun], org, sah=False)
    rc, sah = D.sun_lbvh_check(tris, TABLE_SUNS[sun], org, sah=True)
    _assert_clean(tris, rc, sah)
    print(f"sun {sun}, 20,000 soup: any-hit steps per ray LBVH {plain['cost_lbvh']:.2f}, with the SAH pass {sah['cost_lbvh']:.2f}, host build {sah['cost_host']:.2f}")


def test_flag_off_is_the_old_entries_word_for_word():
    lib = abi.load_library()
    tris = np.ascontiguousarray(soup(3000), np.float32)
    for criterion in (0, 1):
        old, new = (C.c_uint64 * 8)(), (C.c_uint64 * 9)()
        rc_old = lib.ark_ddgi_debug_lbvh_check_opts(tris.ctypes.data, tris.shape[0], criterion, old)
        rc_new = lib.ark_ddgi_debug_lbvh_check_sah(tris.ctypes.data, tris.shape[0], criterion, 0, new)
        assert rc_old == rc_new == 0 and list(old) == list(new)[:8] and new[8] == 0
    org = origins_on(tris, 256)
    for w_bits in (18, 0, 20):
        sd = np.asarray(SUNS["oblique"], np.float32)
        old, new = (C.c_uint64 * 16)(), (C.c_uint64 * 17)()
        rc_old = lib.ark_ddgi_debug_sun_lbvh_check_opts(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], 1e30, w_bits, old)
        rc_new = lib.ark_ddgi_debug_sun_lbvh_check_sah(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], 1e30, w_bits, 0, new)
        assert rc_old == rc_new == 0 and list(old) == list(new)[:16] and new[16] == 0


def test_config_flag():
    """DDGIConfig.gpu_rebuild_sah sets ARK_DDGI_FLAG_GPU_REBUILD_SAH (0x10) and nothing else."""
    grid = D.ProbeGrid((4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert abi.ARK_DDGI_FLAG_GPU_REBUILD_SAH == 0x10 and not D.DDGIConfig().gpu_rebuild_sah
    off = D.desc_for(grid, 100.0, D.DDGIConfig()).flags
    on = D.desc_for(grid, 100.0, D.DDGIConfig(gpu_rebuild_sah=True)).flags
    assert on == off | 0x10
