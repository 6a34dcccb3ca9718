"""The sun's cover map on the device (csrc/sun_cover_map.h, k_shadow_gen): the device build
equals the host restatement bit for bit; an update with the map gives the same bits as one
without it (ARK_DDGI_FLAG_NO_SUN_COVER_MAP), reflections included; the map resolves what the
host restatement says it resolves - most of the soup's sun rays; and a map made stale by a
moved instance, a turned sun or a new scene is not used."""
import ctypes as C

import numpy as np
import pytest
import torch

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import cover_map_inputs as I
import reflection_inputs as RI

pytestmark = pytest.mark.gpu

RESOURCES = (abi.ARK_DDGI_SURFELS, abi.ARK_DDGI_ATLAS_IRRADIANCE, abi.ARK_DDGI_ATLAS_VISIBILITY, abi.ARK_DDGI_PROBE_OFFSETS)
KW = dict(light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5)


def _soup():
    sc = I.soup_scene()
    sc.spots = [I.S.SpotLight((30.0, 25.0, 20.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.9, 3.5, 1.9), 0.9, -1)]
    grid = D.ProbeGrid((4, 4, 4), (0.8, 0.8, 0.8), (0.5, 0.4, 0.5))
    return sc, grid, dict(eye=(1.9, 2.0, 5.5), target=(1.9, 1.5, 1.9))


def _hand():
    return I.hand_scene(), D.ProbeGrid((4, 4, 4), (1.5, 0.6, 1.5), (-2.25, 0.3, -2.25)), {}


SCENES = {"soup": _soup, "hand": _hand}


@pytest.fixture(scope="module", params=sorted(SCENES))
def scene(request):
    return (request.param,) + SCENES[request.param]()


def _cfg(cover_map, background_rebuild):
    return D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=64, max_rays_per_probe=64, max_probe_updates=64, sun_cover_map=cover_map,
                        background_rebuild=background_rebuild)


def _ctx(sc, grid, cover_map, background_rebuild=True):
    ctx = D.DDGIContext(grid, I.Z_FAR, _cfg(cover_map, background_rebuild))
    ctx.set_scene(sc)
    return ctx


def _update(ctx, grid, frame, counting=False):
    ctx.set_counting(counting)
    ctx.update(D.frame_params(ctx.config, grid, D.AppState(frame), 0, **KW))
    ctx.synchronize()


def _same(a, b, what):
    for which in RESOURCES:
        x, y = a.read(which), b.read(which)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: resource {which} differs in {np.count_nonzero(x != y)} elements"


def _reflections(ctx, cam_kw):
    W, H = 96, 64
    cam = RI.camera(W, H, **cam_kw)
    g, _ = RI.gbuffer(W, H, cam, seed=11)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    rad = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
    dirs = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
    D.RTReflectionsNode().execute(ctx, cam, {k: dev[k] for k in ("depth", "material", "normal_velocity")}, dev["blue_noise"], rad, dirs,
                                  environment_multiplier=0.5, ambient_amount=0.05)
    return rad.cpu().numpy(), dirs.cpu().numpy()


def test_device_map_equals_host(scene):
    name, sc, _, _ = scene
    tris = I.world_triangles(sc)
    out = (C.c_uint64 * 6)()
    sd = np.asarray(sc.sun[1], np.float32)
    rc = abi.load_library().ark_ddgi_debug_cover_map_device(0, tris.ctypes.data, len(tris), sd.ctypes.data, 0, out)
    diff, nx, ny, host_ok, dev_ok, us = (int(v) for v in out)
    print(name, "cells", nx, ny, "device build us", us)
    assert rc == 0 and host_ok == 1 and dev_ok == 1
    assert diff == 0


def test_same_results_with_and_without_the_map(scene):
    """One update with the map and one without (4 x 4 x 4 probes, 64 rays, the sun and a spot
    light: the sun's and the world list coexist), then the reflections of both contexts, then
    a counting update whose counts the host restatement must match exactly. On the soup the
    map must resolve at least half of the sun's rays (measured on the host first: 73 % of
    uniform surface origins, test_sun_cover_map.py; of this update's 1,033 sun rays the host
    restatement resolves 857, 83 %)."""
    name, sc, grid, cam_kw = scene
    on, off = _ctx(sc, grid, True), _ctx(sc, grid, False)
    for f in range(2):
        _update(on, grid, f)
        _update(off, grid, f)
        _same(on, off, f"{name} frame {f}")
    for a, b in zip(_reflections(on, cam_kw), _reflections(off, cam_kw)):
        assert np.array_equal(a, b), f"{name}: reflections differ in {np.count_nonzero(a != b)} values"
    _update(on, grid, 2, counting=True)
    _update(off, grid, 2, counting=True)
    _same(on, off, f"{name} counting frame")
    c, d = on.sun_cover_counts(), off.sun_cover_counts()
    print(name, c, d)
    assert c["in_use"] == 1 and c["map_diff"] == 0
    assert (c["occluded"], c["lit"], c["listed"]) == (c["host_occluded"], c["host_lit"], c["host_listed"])
    assert d["in_use"] == 0 and d["occluded"] == 0 and d["lit"] == 0
    total = c["occluded"] + c["lit"] + c["listed"]
    assert total == d["listed"] and total > 0
    assert on.counters().shadow_rays < off.counters().shadow_rays
    if name == "soup":
        assert 2 * (c["host_occluded"] + c["host_lit"]) >= total
    on.close()
    off.close()


def test_stale_maps_are_not_used(scene):
    """An instance moves, the sun turns, set_scene is called again, each between two updates:
    outputs equal a context without the map, and while no valid map is installed the counts
    show no resolved ray. (No background rebuild after the refit: a finished one would bring
    a map of the moved geometry with it, at a time of its own.)"""
    name, sc, grid, _ = scene
    on, off = _ctx(sc, grid, True, False), _ctx(sc, grid, False, False)

    def step(f, expect_map):
        _update(on, grid, f, counting=True)
        _update(off, grid, f, counting=True)
        _same(on, off, f"{name} frame {f}")
        c = on.sun_cover_counts()
        assert c["in_use"] == (1 if expect_map else 0), c
        if expect_map:
            assert c["occluded"] + c["lit"] > 0 and c["map_diff"] == 0
            assert (c["occluded"], c["lit"], c["listed"]) == (c["host_occluded"], c["host_lit"], c["host_listed"])
        else:
            assert c["occluded"] == 0 and c["lit"] == 0

    step(0, True)
    inst = sc.instances.copy()
    M = inst[0]["object_to_world"].reshape(3, 4).copy()
    M[:, 3] += (0.3, 0.2, -0.25)
    inst[0]["object_to_world"] = M.reshape(-1)
    for ctx in (on, off):
        ctx.set_instances(inst)
    step(1, False)
    sun = (sc.sun[0], tuple(np.array([0.2, -1.0, 0.3]) / np.linalg.norm([0.2, -1.0, 0.3])))
    for ctx in (on, off):
        ctx.set_lights(sun, sc.spots)
    step(2, False)
    for ctx in (on, off):
        ctx.set_scene(sc)
    step(3, True)
    on.close()
    off.close()
