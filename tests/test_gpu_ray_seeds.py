"""The probe rays' hit candidates (csrc/seed_cache.h, k_trace): a context keeps, per probe,
a 16 x 16 octahedral map direction -> the triangle record the last ray in that direction hit,
and every probe ray tests its texel's record before it enters the BVH. The record is only a
candidate - tested by the traversal's own triangle step, as the ray's first pending triangle
group - so nothing a context computes may depend on what the cache holds.

Bar, throughout: a context with the cache and one with ARK_DDGI_FLAG_NO_RAY_SEEDS, identical
otherwise, agree bit for bit after every update on the irradiance and visibility atlases, the
probe offsets, the surfels and the hit records (t, u, v and the record index).

The hits reach the cache by one of two writers, and the cases cover both: k_probe_offsets when
probe offsets are computed and the scene has no masked class, else the k_trace instances that
write as their rays retire (offsets off; a masked class)."""
import time

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S
import scenes
from parity import RESOURCES
from test_gpu_refit_sequences import _inward, _instances, _moved, _rest
from test_gpu_refit_sequences import _scene as _city

pytestmark = pytest.mark.gpu

WAIT_S = 60.0
UPDATES = 6
EXPOSURE = dict(light_pre_exposure=1.0, environment_brightness=1.0)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _outputs(ctx):
    out = {k: _bits(ctx.read(w)) for k, w in RESOURCES.items()}
    out["hits"] = _bits(ctx.read(abi.ARK_DDGI_DEBUG_HITS))
    return out


def _assert_same(on, off, label):
    a, b = _outputs(on), _outputs(off)
    for k in a:
        bad = np.flatnonzero(a[k] != b[k])
        assert bad.size == 0, f"{label}: {k} differs in {bad.size} words, first at {bad[:4].tolist()}"
    return a


def _pair(grid, z_far, **cfg):
    return D.DDGIContext(grid, z_far, D.DDGIConfig(**cfg)), D.DDGIContext(grid, z_far, D.DDGIConfig(ray_seeds=False, **cfg))


def _soup_scene():
    return S.soup(20_000, extent=7.0)


SOUP_GRID = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5))


def _soup_cfg(**over):
    cfg = dict(rays_per_probe=64, probe_updates_per_frame=64, compute_probe_offsets=True, max_rays_per_probe=64, max_probe_updates=64)
    cfg.update(over)
    return cfg


def _run_static(sc, grid, z_far, cfg, exposure, label):
    on, off = _pair(grid, z_far, **cfg)
    try:
        assert on.seed_info()["enabled"] and not off.seed_info()["enabled"]
        on.set_scene(sc)
        off.set_scene(sc)
        info = on.seed_info()
        assert info["texels"] == 16 and info["end"] > info["first"], info
        first = 0
        hit_any = False
        for f in range(UPDATES):
            p = D.frame_params(on.config, grid, D.AppState(f), first, **exposure)
            on.update(p)
            off.update(p)
            on.synchronize()
            off.synchronize()
            out = _assert_same(on, off, f"{label}, update {f}")
            hit_any = hit_any or bool(np.any(out["hits"].reshape(-1, 4)[:, 3] != 0xFFFFFFFF))
            first = (first + p.probe_updates) % grid.probe_count()
        assert hit_any and np.count_nonzero(out["irradiance"]) > 0, f"{label}: nothing was hit or lit"
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("offsets", [True, False])
def test_identical_soup(offsets):
    """The 20,000-triangle soup at C4 density, 4 x 4 x 4 probes x 64 rays, K = N, frames in
    flight; with probe offsets (k_probe_offsets writes the cache) and without (k_trace does)."""
    _run_static(_soup_scene(), SOUP_GRID, 10000.0, _soup_cfg(compute_probe_offsets=offsets), EXPOSURE, f"soup, offsets {offsets}")


def test_identical_masked_class():
    """tests/test_gpu_trace_pool.py's masked-pass scene (opaque, masked and blend classes, a
    mirrored instance; a window of 50 of 144 probes): the opaque pass's hit is cached at the
    pass 0 -> 1 transition, and no masked-class record may ever be offered to pass 0."""
    sc = scenes.features_scene()
    grid = D.ProbeGrid((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))
    cfg = dict(rays_per_probe=72, probe_updates_per_frame=50, compute_probe_offsets=True, max_rays_per_probe=72, max_probe_updates=50)
    _run_static(sc, grid, 100.0, cfg, dict(light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5), "features")


def test_identical_rolling_window():
    """K = 24 of N = 64 probes: the window's slots change probes from update to update (the
    cache is indexed by probe, not by slot), and windows wrap past the grid's end."""
    _run_static(_soup_scene(), SOUP_GRID, 10000.0, _soup_cfg(probe_updates_per_frame=24, max_probe_updates=24), EXPOSURE, "soup, rolling window")


def test_identical_across_refits_and_installed_rebuild():
    """The refit tests' city block (97 instances) with props moving every frame and the
    background rebuild on: refits keep the record order (the cache stays), an installed rebuild
    is a new order (the cache starts over, on the traversal stream ahead of the next traversal).
    The two contexts share one scene store, so both trace the same tree in every frame and the
    hit records' indices compare too; the rebuild is installed by whichever context's update
    finds it finished, so the cached context also meets an install that the other made."""
    sc = _city()
    grid = D.ProbeGrid((4, 2, 4), (5.0, 2.0, 5.0), (2.0, 1.0, 2.0))
    on, off = _pair(grid, 1000.0, rays_per_probe=32, probe_updates_per_frame=32, compute_probe_offsets=True, max_rays_per_probe=32, max_probe_updates=32)
    try:
        on.set_scene(sc)
        off.share_scene(on)
        M0 = _rest()
        f, after, t0 = 0, 0, time.time()
        while after < 3 or f < UPDATES:
            M = M0.copy()
            for i in (5, 40, 69):
                M[i] = _moved(M0, i, 0.05 * (f + 1) * _inward(M0, i, 0))
            M[17] = _moved(M0, 17, (2.5 if f % 3 == 1 else 0.0) * _inward(M0, 17, 2))  # a nudge and return
            inst = _instances(M)
            on.set_instances(inst)
            p = D.frame_params(on.config, grid, D.AppState(f), 0, **EXPOSURE)
            # (the contexts take turns at going first: each gets to install)
            for c in ((on, off) if f % 2 == 0 else (off, on)):
                c.update(p)
            on.synchronize()
            off.synchronize()
            st = on.bvh_stats()
            _assert_same(on, off, f"city, frame {f} ({st.bvh_rebuilds} rebuilds installed)")
            after += 1 if st.bvh_rebuilds >= 1 else 0
            f += 1
            assert time.time() - t0 < WAIT_S, f"no rebuild installed within {WAIT_S} s: {on.last_error()}"
        print(f"city: {f} frames, {st.bvh_rebuilds} rebuilds installed")
        assert st.bvh_rebuilds >= 1 and st.bvh_rebuild_failures == 0
    finally:
        off.close()
        on.close()


def test_cache_content_does_not_matter():
    """ark_ddgi_debug_seed_fill overwrites the cache with (a) the sentinel, (b) seeded random
    records of the opaque class, (c) one record everywhere; after each, the next update's
    outputs equal the uncached context's. Only words the guard accepts reach the device: a
    record outside the opaque class is refused on the host."""
    sc = _soup_scene()
    on, off = _pair(SOUP_GRID, 10000.0, **_soup_cfg())
    try:
        on.set_scene(sc)
        off.set_scene(sc)
        info = on.seed_info()

        def step(f, label):
            p = D.frame_params(on.config, SOUP_GRID, D.AppState(f), 0, **EXPOSURE)
            on.update(p)
            off.update(p)
            on.synchronize()
            off.synchronize()
            return _assert_same(on, off, label)

        step(0, "before any fill")
        out = step(1, "before any fill")
        tri = out["hits"].reshape(-1, 4)[:, 3]
        some = int(tri[tri != 0xFFFFFFFF][0])
        assert info["first"] <= some < info["end"]
        f = 2
        for mode, value, what in ((0, 0, "sentinel"), (1, 12345, "random records"), (1, 777, "random records, another seed"), (2, some, "one hit record everywhere"),
                                  (2, info["first"], "the first record everywhere"), (2, info["end"] - 1, "the last opaque record everywhere")):
            on.seed_fill(mode, value)
            step(f, f"after fill: {what}")
            step(f + 1, f"one update after fill: {what}")
            f += 2
        for bad in (info["end"], 0xFFFFFFFF, 0x80000000):
            with pytest.raises(abi.ArkDdgiError):
                on.seed_fill(2, bad)
        with pytest.raises(abi.ArkDdgiError):
            off.seed_fill(0)  # no cache to fill
        step(f, "after the refused fills")
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("offsets", [True, False])
def test_seeding_saves_node_visits(offsets):
    """What it is for (with either writer of the cache): on the soup, from the third update on, a counting update visits strictly
    fewer nodes with the cache than without; on the first update after set_scene the cache is
    empty and the two counts are equal."""
    sc = _soup_scene()
    on, off = _pair(SOUP_GRID, 10000.0, **_soup_cfg(compute_probe_offsets=offsets))
    try:
        on.set_scene(sc)
        off.set_scene(sc)
        on.set_counting(True)
        off.set_counting(True)
        for f in range(UPDATES):
            p = D.frame_params(on.config, SOUP_GRID, D.AppState(f), 0, **EXPOSURE)
            on.update(p)
            off.update(p)
            on.synchronize()
            off.synchronize()
            a, b = on.counters(), off.counters()
            accepted = on.seed_info()["candidate_hits"]
            print(f"update {f}: primary_node_visits {int(a.primary_node_visits)} with the cache, {int(b.primary_node_visits)} without; "
                  f"triangle tests {int(a.primary_tri_tests)} / {int(b.primary_tri_tests)}; candidates hit {accepted} of {int(a.rays)} rays "
                  f"({accepted / max(1, int(a.rays)):.3f})")
            _assert_same(on, off, f"counting update {f}")
            assert off.seed_info()["candidate_hits"] == 0
            if f == 0:
                assert int(a.primary_node_visits) == int(b.primary_node_visits) and int(a.primary_tri_tests) == int(b.primary_tri_tests) and accepted == 0
            if f >= 2:
                assert int(a.primary_node_visits) < int(b.primary_node_visits)
                assert 0 < accepted <= int(a.rays)
    finally:
        on.close()
        off.close()
