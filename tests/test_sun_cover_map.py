"""The sun's cover map is conservative (csrc/sun_cover_map.h; no GPU): the host map's
verdicts - occluded, lit, undecided - against a brute-force any-hit over every triangle
with the kernels' fp32 Moller-Trumbore (ark_ddgi_debug_cover_map_check). No verdict may
disagree; undecided is always allowed."""
import ctypes as C

import numpy as np
import pytest

from arkoserenderer_amd import abi
import cover_map_inputs as I

KEYS = ("rays", "brute_occluded", "occluded", "lit", "wrong", "nx", "ny", "valid", "covered_cells", "undecided", "u0", "v0", "inv_cell")


def cover_map_check(tris, sun_dir, origins, tmax=2.0 * I.Z_FAR, budget=0):
    lib = abi.load_library()
    out = (C.c_uint64 * 13)()
    tris = np.ascontiguousarray(tris, np.float32)
    origins = np.ascontiguousarray(origins, np.float32)
    sd = np.asarray(sun_dir, np.float32)
    rc = lib.ark_ddgi_debug_cover_map_check(tris.ctypes.data, len(tris), sd.ctypes.data, origins.ctypes.data, len(origins), C.c_float(tmax), budget, out)
    assert rc == 0
    r = dict(zip(KEYS, (int(v) for v in out)))
    for k in ("u0", "v0", "inv_cell"):
        r[k] = float(np.array([r[k]], np.uint32).view(np.float32)[0])
    return r


@pytest.fixture(scope="module")
def soup():
    sc = I.soup_scene()
    return sc, I.world_triangles(sc)


def test_soup_verdicts_agree_with_brute_force(soup):
    """20 k triangles at the flagship's density, 200 k origins: 150 k on the triangles (where
    shadow rays start) and 50 k in the volume. Measured here: 0 wrong verdicts; of the surface
    origins 65 % are resolved occluded and 8 % lit (79 % are occluded by brute force)."""
    sc, tris = soup
    origins = np.concatenate([I.surface_origins(tris, 150_000, 1), I.volume_origins(tris, 50_000, 2)])
    r = cover_map_check(tris, sc.sun[1], origins)
    print(r)
    assert r["valid"] == 1 and r["rays"] == 200_000
    assert r["wrong"] == 0
    assert r["occluded"] > 0 and r["lit"] > 0 and r["occluded"] <= r["brute_occluded"]


def test_hand_scene_edges_borders_and_classes():
    """The hand-built scene under a straight sun: origins on the map's cell borders, on the
    roof's edges, diagonal and vertices (each a few ulp either side), just below and above
    the roof and around tmin below it, on the floor, plus random surface and volume points."""
    sc = I.hand_scene()
    tris = I.world_triangles(sc)
    g = cover_map_check(tris, I.HAND_SUN_DIR, tris[:1, :3].copy())
    assert g["valid"] == 1
    origins = np.concatenate([I.hand_edge_origins(g["u0"], g["v0"], g["inv_cell"], g["nx"], g["ny"]), I.surface_origins(tris, 50_000, 3),
                              I.volume_origins(tris, 50_000, 4)])
    assert len(origins) >= 200_000
    r = cover_map_check(tris, I.HAND_SUN_DIR, origins)
    print(r)
    assert r["wrong"] == 0
    assert r["occluded"] > 0 and r["lit"] > 0
    # the quads of the masked and the blend hit-mask class occlude like any other (the sun's
    # any-hit traversal accepts all three classes unconditionally), the vertical wall never does
    # (off the quads' diagonals: a cell that straddles two triangles is covered by neither)
    under = {"masked": (-2.2, 0.7, -2.2), "blend": (2.8, 0.6, -2.7), "roof": (0.1, 1.0, 0.4)}
    for name, p in under.items():
        q = cover_map_check(tris, I.HAND_SUN_DIR, np.array([p], np.float32))
        assert q["brute_occluded"] == 1 and q["occluded"] == 1, name
    open_sky = cover_map_check(tris, I.HAND_SUN_DIR, np.array([(-3.0, 2.2, 2.0), (3.8, 1.2, 3.8)], np.float32))  # above the wall, beside everything
    assert open_sky["brute_occluded"] == 0 and open_sky["lit"] == 2


def test_short_rays_switch_the_map_off(soup):
    """tmax below the scene's extent along the sun: a covering triangle may lie beyond the
    ray's reach, so there is no map and every ray is undecided."""
    sc, tris = soup
    origins = I.surface_origins(tris, 1000, 5)
    r = cover_map_check(tris, sc.sun[1], origins, tmax=1.0)
    assert r["valid"] == 0 and r["occluded"] == 0 and r["lit"] == 0 and r["wrong"] == 0


@pytest.mark.parametrize("budget_mb", [1, 16, 256])
def test_budget_bounds_the_map(soup, budget_mb):
    sc, tris = soup
    r = cover_map_check(tris, sc.sun[1], I.surface_origins(tris, 2000, 6), budget=budget_mb << 20)
    assert r["valid"] == 1 and r["wrong"] == 0
    assert r["nx"] * r["ny"] * 8 <= (budget_mb << 20) * 17 // 16
