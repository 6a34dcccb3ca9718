"""The device rebuilds of the world BVH8s and of the sun's light-space BVH8 with the collapse
plan (ARK_DDGI_FLAG_GPU_REBUILD_PLAN, DDGIConfig.gpu_rebuild_plan; csrc/ddgi_bvh_build.hip: the
plan instance of k_lbvh_treelet_sah, k_lbvh_upper_plan, the collapse by lbvh::planCut): the
installed trees are valid device builds over the same records, the results do not depend on
the tree (bit-equal to the run with the SAH pass alone and to the oracle), the flag without the
SAH pass changes nothing, and on the 20,000 soup the primary rays' node visits plus triangle
tests - what the SAH cost models - fall strictly below the figure with the SAH pass alone.
The scene of the first part is test_gpu_bvh_build_sah.py's city_block(1650, 72.0). Also the C++
DDGINode's setGpuRebuildPlan."""
import functools
import subprocess
import time

import numpy as np
import pytest

from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S
import oracle_lib as O
import scenes
from parity import RESOURCES, diff_report
from test_gpu_bvh_build_sah import EXPOSURE, GRID, WAIT_S, _cfg, _nudged, city
from test_gpu_cpp_node import EXE, _frame_script

pytestmark = pytest.mark.gpu

SOUP_GRID = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))  # test_flag_alone_is_inert's


@functools.lru_cache(maxsize=None)
def soup_scene():
    return S.soup(20_000, extent=7.0)


def _device_trees(scene, sah, plan):
    """Both trees device-built under the flags and installed under the nudging, then the scene
    back in place and one counted frame: (stats, world check, sun check, counters, resources, params)."""
    city_scene = scene == "city"
    sc = city() if city_scene else soup_scene()
    grid = GRID if city_scene else SOUP_GRID
    if city_scene:
        cfg = _cfg(gpu_rebuild=True, gpu_rebuild_sun=True, gpu_rebuild_sah=sah, gpu_rebuild_plan=plan)
    else:
        cfg = D.DDGIConfig(rays_per_probe=32, probe_updates_per_frame=64, max_rays_per_probe=32, max_probe_updates=64, gpu_rebuild=True, gpu_rebuild_sun=True,
                           gpu_rebuild_sah=sah, gpu_rebuild_plan=plan)
    ctx = D.DDGIContext(grid, 1000.0 if city_scene else 10000.0, cfg)
    try:
        ctx.set_scene(sc)
        has_sun = ctx.bvh_stats().sun_node_count > 0
        f, t0 = 1, time.time()
        while True:
            ctx.set_instances(_nudged(sc.instances, f))  # (a set_instances installs a finished build and starts the next)
            f += 1
            st = ctx.bvh_stats()
            sun_done = not has_sun or (st.sun_gpu_rebuilds >= 1 and st.sun_installed_builder == 1)
            if st.bvh_gpu_rebuilds >= 1 and st.bvh_installed_builder == 1 and sun_done and f % 2 == 1:
                break
            assert time.time() - t0 < WAIT_S, f"device builds installed within {WAIT_S} s: world {st.bvh_gpu_rebuilds}, sun {st.sun_gpu_rebuilds}: {ctx.last_error()}"
        st = ctx.bvh_stats()
        world, sun = ctx.world_bvh_check(), ctx.sun_bvh_installed_check()
        ctx.set_counting(True)
        p = D.frame_params(cfg, grid, D.AppState(0), 0, **EXPOSURE)
        ctx.update(p)
        ctx.synchronize()
        c = ctx.counters()
        counted = {k: int(getattr(c, k)) for k in ("primary_node_visits", "primary_tri_tests", "shadow_node_visits", "shadow_tri_tests")}
        return st, world, sun, counted, {k: ctx.read(w) for k, w in RESOURCES.items()}, p
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def run(scene, sah, plan):
    return _device_trees(scene, sah, plan)


def _shape(check):
    return {k: check[k] for k in ("nodes", "leaf_children", "max_depth", "records", "records_with_holes", "record_digest", "installed_builder")}


@pytest.mark.parametrize("sah,plan", [(True, False), (True, True), (False, True)])
def test_installed_trees_are_valid_device_builds(sah, plan):
    st, world, sun, counted, _, _ = run("city", sah, plan)
    print(f"gpu_rebuild_sah={sah}, gpu_rebuild_plan={plan}: world {world}, sun {sun}, build {st.bvh_rebuild_ms:.2f} / {st.sun_build_ms:.2f} ms, {counted}")
    assert world["violations"] == 0 and world["installed_builder"] == 1, world
    assert sun["installed"] and sun["violations"] == 0 and sun["installed_builder"] == 1, sun
    assert (sun["records"], sun["record_digest"]) == (world["records"], world["record_digest"])
    assert st.bvh_gpu_fallbacks == 0 and st.sun_gpu_fallbacks == 0 and st.bvh_rebuild_failures == 0 and st.sun_rebuild_failures == 0


def test_results_do_not_depend_on_the_plan():
    """Atlases, offsets and surfels after the installs: bit-equal with the plan and with the SAH
    pass alone, and to the oracle's frame of the same scene."""
    sah, plan = run("city", True, False), run("city", True, True)
    assert (plan[1]["records"], plan[1]["record_digest"]) == (sah[1]["records"], sah[1]["record_digest"])
    for k in RESOURCES:
        assert diff_report(k, plan[4][k], sah[4][k])["mismatch"] == 0, k
    cfg = _cfg(gpu_rebuild=True, gpu_rebuild_sun=True, gpu_rebuild_sah=True, gpu_rebuild_plan=True)
    orc = O.Oracle(D.desc_for(GRID, 1000.0, cfg))
    try:
        orc.set_scene(city())
        orc.set_instances(city().instances)
        orc.update(plan[5])
        for k, w in RESOURCES.items():
            assert diff_report(k, plan[4][k], orc.read(w))["mismatch"] == 0, k
    finally:
        orc.close()


def test_flag_without_the_sah_pass_is_inert():
    """gpu_rebuild_plan without gpu_rebuild_sah: the device builds are the ones without either -
    the same digest of the trees' records, the same results. (A job's snapshot is taken with
    box 0 in place or a millimetre up, so two runs' tree shapes are printed, not compared; that
    the flag alone leaves every stage of a build as it was is test_gpu_lbvh_plan_parity.py's.)"""
    from test_gpu_bvh_build_sah import runs
    base = runs()[False]
    alone = run("city", False, True)
    print(f"without either flag: world {_shape(base[1])}, sun {_shape(base[2])}; the plan's flag alone: world {_shape(alone[1])}, sun {_shape(alone[2])}")
    for tree in (1, 2):
        assert (alone[tree]["records"], alone[tree]["record_digest"]) == (base[tree]["records"], base[tree]["record_digest"])
    for k in RESOURCES:
        assert diff_report(k, alone[4][k], base[4][k])["mismatch"] == 0, k


def test_primary_rays_do_less_work_on_the_soup_with_the_plan():
    """The 20,000 soup, one counted frame of 64 probes x 32 rays: primary node visits plus triangle
    tests with the plan strictly below the figure with the SAH pass alone (the cost model counts
    both, and predicts -27 %). The city block's and the shadow rays' figures are printed."""
    for scene in ("city", "soup"):
        sah, plan = run(scene, True, False), run(scene, True, True)
        for name, r in (("the SAH pass alone", sah), ("the plan", plan)):
            assert r[1]["violations"] == 0 and r[1]["installed_builder"] == 1, r[1]
            assert r[0].bvh_gpu_fallbacks == 0 and r[0].sun_gpu_fallbacks == 0 and r[0].bvh_rebuild_failures == 0 and r[0].sun_rebuild_failures == 0
            print(f"{scene}, {name}: world {r[1]['nodes']} nodes, sun {r[2]['nodes']} nodes, build {r[0].bvh_rebuild_ms:.2f} / {r[0].sun_build_ms:.2f} ms, {r[3]}")
    sah, plan = run("soup", True, False)[3], run("soup", True, True)[3]
    before, after = sah["primary_node_visits"] + sah["primary_tri_tests"], plan["primary_node_visits"] + plan["primary_tri_tests"]
    print(f"20,000 soup: primary node visits + triangle tests {before} -> {after} ({100.0 * (after - before) / before:+.1f} %)")
    assert after < before, (sah, plan)


def test_cpp_node_toggles_the_plan(tmp_path):
    """DDGINode::setGpuRebuildPlan through ddgi_headless --gpu-rebuild: a box moving every frame,
    all four flags (15) and the plan's flag alone (8). Every run's atlases and offsets equal the
    run without a flag."""
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
    for mask in (0, 15, 8):
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
            if mask == 8:
                assert "installed world 0, sun 0," in line[0], line[0]
    for mask in (15, 8):
        for k, dt in (("irr", np.uint16), ("vis", np.uint16), ("off", np.float32)):
            assert np.array_equal(np.fromfile(outs[mask][0] + "." + k, dtype=dt), np.fromfile(outs[0][0] + "." + k, dtype=dt)), (mask, k)
