"""The device rebuilds of the world BVH8s and of the sun's light-space BVH8 with the SAH pass
(ARK_DDGI_FLAG_GPU_REBUILD_SAH, DDGIConfig.gpu_rebuild_sah; csrc/ddgi_bvh_build.hip
k_lbvh_treelet_sah): the installed trees are valid device builds over the same records, the
results do not depend on the tree (bit-equal to the run without the pass and to the oracle),
and the rays visit fewer nodes than in the trees built without the pass. The scene is
test_lbvh_sah.py's city_block(1650, 72.0), 19,802 triangles, on which the host restatement
already shows the world BVH8 SAH cost and the sun's any-hit steps falling. Also: the flag alone
does nothing, and the C++ DDGINode's setGpuRebuildSah."""
import functools
import subprocess
import time

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S
import oracle_lib as O
import scenes
from parity import RESOURCES, diff_report
from test_gpu_cpp_node import EXE, _frame_script

pytestmark = pytest.mark.gpu

GRID = D.ProbeGrid((4, 4, 4), (16.0, 3.0, 16.0), (12.0, 1.0, 12.0))
EXPOSURE = dict(light_pre_exposure=1.0, environment_brightness=1.0)
WAIT_S = 60  # wall-clock bound of every polling loop


def _cfg(R=64, K=64, **kw):
    kw.setdefault("sun_bvh", abi.ARK_DDGI_SUN_BVH_LIGHT_SPACE)
    return D.DDGIConfig(rays_per_probe=R, probe_updates_per_frame=K, max_rays_per_probe=R, max_probe_updates=K, compute_probe_offsets=True, **kw)


@functools.lru_cache(maxsize=None)
def city():
    sc0 = S.city_block(box_count=1650, extent=72.0)
    return S.SceneData(**{**{k: v for k, v in sc0.__dict__.items() if not k.startswith("_")}, "spots": []})


def _nudged(inst0, f):
    """Box 0 a millimetre up on odd calls, back in place on even ones: every call refits, and
    whenever a job takes its snapshot the scene is the same to within that millimetre."""
    inst = inst0.copy()
    M = inst["object_to_world"].reshape(-1, 3, 4).copy()
    M[0, 1, 3] += np.float32(0.001 * (f & 1))
    inst["object_to_world"] = M.reshape(len(inst), 12)
    return inst


def _device_trees(sah):
    """Both trees device-built (the pass on or off) and installed under the nudging, then the
    scene back in place and one counted frame: (stats, checks, counters, resources)."""
    sc = city()
    cfg = _cfg(gpu_rebuild=True, gpu_rebuild_sun=True, gpu_rebuild_sah=sah)
    ctx = D.DDGIContext(GRID, 1000.0, cfg)
    try:
        ctx.set_scene(sc)
        assert ctx.bvh_stats().sun_node_count > 0
        f, t0 = 1, time.time()
        while True:
            ctx.set_instances(_nudged(sc.instances, f))  # (a set_instances installs a finished build and starts the next)
            f += 1
            st = ctx.bvh_stats()
            if st.bvh_gpu_rebuilds >= 1 and st.sun_gpu_rebuilds >= 1 and st.bvh_installed_builder == 1 and st.sun_installed_builder == 1 and f % 2 == 1:
                break
            assert time.time() - t0 < WAIT_S, f"device builds installed within {WAIT_S} s: world {st.bvh_gpu_rebuilds}, sun {st.sun_gpu_rebuilds}: {ctx.last_error()}"
        # (the last call was an even one: the scene is in place)
        st = ctx.bvh_stats()
        world, sun = ctx.world_bvh_check(), ctx.sun_bvh_installed_check()
        ctx.set_counting(True)
        p = D.frame_params(cfg, GRID, D.AppState(0), 0, **EXPOSURE)
        ctx.update(p)
        ctx.synchronize()
        c = ctx.counters()
        return st, world, sun, (int(c.primary_node_visits), int(c.shadow_node_visits)), {k: ctx.read(w) for k, w in RESOURCES.items()}, p
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def runs():
    return {sah: _device_trees(sah) for sah in (False, True)}


@pytest.mark.parametrize("sah", [False, True])
def test_installed_trees_are_valid_device_builds(sah):
    st, world, sun, visits, _, _ = runs()[sah]
    print(f"gpu_rebuild_sah={sah}: world {world}, sun {sun}, build {st.bvh_rebuild_ms:.2f} / {st.sun_build_ms:.2f} ms, node visits {visits}")
    assert world["violations"] == 0 and world["installed_builder"] == 1, world
    assert sun["installed"] and sun["violations"] == 0 and sun["installed_builder"] == 1, sun
    assert (sun["records"], sun["record_digest"]) == (world["records"], world["record_digest"])
    assert st.bvh_gpu_fallbacks == 0 and st.sun_gpu_fallbacks == 0 and st.bvh_rebuild_failures == 0 and st.sun_rebuild_failures == 0


def test_results_do_not_depend_on_the_pass():
    """Atlases, offsets and surfels after the installs: bit-equal with and without the pass,
    and to the oracle's frame of the same scene."""
    plain, sah = runs()[False], runs()[True]
    assert (sah[1]["records"], sah[1]["record_digest"]) == (plain[1]["records"], plain[1]["record_digest"])
    for k in RESOURCES:
        assert diff_report(k, sah[4][k], plain[4][k])["mismatch"] == 0, k
    cfg = _cfg(gpu_rebuild=True, gpu_rebuild_sun=True, gpu_rebuild_sah=True)
    orc = O.Oracle(D.desc_for(GRID, 1000.0, cfg))
    try:
        orc.set_scene(city())
        orc.set_instances(city().instances)
        orc.update(sah[5])
        for k, w in RESOURCES.items():
            assert diff_report(k, sah[4][k], orc.read(w))["mismatch"] == 0, k
    finally:
        orc.close()


def test_rays_visit_fewer_nodes_with_the_pass():
    plain, sah = runs()[False][3], runs()[True][3]
    print(f"city_block(1650, 72.0), one frame of 64 probes x 64 rays: primary node visits {plain[0]} -> {sah[0]}, shadow node visits {plain[1]} -> {sah[1]}")
    assert sah[0] < plain[0]
    assert sah[1] < plain[1]


def test_flag_alone_is_inert():
    """gpu_rebuild_sah without a device-rebuild flag: accepted, and the rebuilds stay the host's."""
    sc = S.soup(20_000, extent=7.0)
    grid = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
    cfg = D.DDGIConfig(rays_per_probe=32, probe_updates_per_frame=64, max_rays_per_probe=32, max_probe_updates=64, gpu_rebuild_sah=True)
    assert not cfg.gpu_rebuild and not cfg.gpu_rebuild_sun
    ctx = D.DDGIContext(grid, 10000.0, cfg)
    try:
        ctx.set_scene(sc)
        first, f, t0 = 0, 0, time.time()
        while ctx.bvh_stats().bvh_rebuilds < 1:
            if f < 4:
                inst = sc.instances.copy()
                M = inst["object_to_world"].reshape(-1, 3, 4).copy()
                M[f % len(inst), :, 3] += np.float32(0.02 * (f + 1))
                inst["object_to_world"] = M.reshape(len(inst), 12)
                ctx.set_instances(inst)
            p = D.frame_params(cfg, grid, D.AppState(f), first, **EXPOSURE)
            ctx.update(p)
            ctx.synchronize()
            first = (first + p.probe_updates) % grid.probe_count()
            f += 1
            assert time.time() - t0 < WAIT_S, f"no host rebuild installed within {WAIT_S} s: {ctx.last_error()}"
        st = ctx.bvh_stats()
        assert st.bvh_gpu_rebuilds == 0 and st.sun_gpu_rebuilds == 0 and st.bvh_installed_builder == 0 and st.bvh_gpu_fallbacks == 0
        assert ctx.world_bvh_check()["installed_builder"] == 0
    finally:
        ctx.close()


def test_cpp_node_toggles_the_pass(tmp_path):
    """DDGINode::setGpuRebuild / setGpuRebuildSun / setGpuRebuildSah through ddgi_headless
    --gpu-rebuild: a box moving every frame, the device rebuilds without and with the pass,
    and the pass's flag alone. Every run's atlases and offsets equal the run without a flag."""
    sc = scenes.features_scene()
    scene_path, script = str(tmp_path / "features.arkscn"), str(tmp_path / "frames.arkfrm")
    sc.save_binary(scene_path)
    M0 = sc.instances["object_to_world"].reshape(-1, 3, 4).copy()
    d0 = tuple(float(x) for x in np.array([0.3, -1.0, -0.4]) / np.linalg.norm([0.3, -1.0, -0.4]))
    frames = []
    for f in range(30):
        M = M0.copy()
        M[3, :, 3] += np.float32(0.01 * (f + 1))
        frames.append(dict(exposure=0.5, sun=dict(color=(1.0, 0.95, 0.85), intensity=2.0, forward=d0), spots=[], transforms=M.reshape(-1, 12)))
    _frame_script(script, frames, len(sc.instances))
    outs = {}
    for mask in (0, 3, 7, 4):
        out = str(tmp_path / f"m{mask}")
        cmd = [EXE, "--scene", scene_path, "--grid", "6", "4", "6", "--spacing", "0.7", "0.7", "0.7", "--origin", "-1.75", "0.25", "-1.75",
               "--rays", "64", "--updates", "100", "--frames", str(len(frames)), "--zfar", "100", "--exposure", "0.5", "--env", "0.8",
               "--ambient", "0.1", "--offsets", "1", "--frame-script", script, "--gpu-rebuild", str(mask), "--out", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[mask] = (out, r.stdout)
        if mask:
            line = [ln for ln in r.stdout.splitlines() if f"gpu rebuild mask {mask}:" in ln]
            assert line and "fallbacks 0 / 0, failures 0 / 0" in line[0], r.stdout
            print(line[0])
            if mask == 4:
                assert "installed world 0, sun 0," in line[0], line[0]
    for mask in (3, 7, 4):
        for k, dt in (("irr", np.uint16), ("vis", np.uint16), ("off", np.float32)):
            assert np.array_equal(np.fromfile(outs[mask][0] + "." + k, dtype=dt), np.fromfile(outs[0][0] + "." + k, dtype=dt)), (mask, k)
