"""k_trace's wave-private ray pool: a wave sets up the rays of a grabbed chunk once,
with every lane, parks the records in LDS, and its refills read them back. The
shapes here are the smallest at which that bookkeeping can go wrong (short chunks,
pools that straddle partition ends, empty partitions, fewer rays than lanes, the
masked pass, both frame modes, the list source of the reflections). The pipelined
contexts run the 32-slot instance of the kernel (windows that grab 32 rays), the
serial one and the reflections the 64-slot instance.

Bar: bit-exact against the CPU oracle, as tests/test_gpu_parity.py (surfels, atlases,
offsets; non-trivial oracle output), and as tests/test_gpu_reflections.py for the
ray-list source."""
import numpy as np
import pytest

from arkoserenderer_amd import abi  # noqa: F401
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S
import scenes
from parity import RESOURCES, diff_report, run_pair
from test_gpu_parity import _assert_exact

pytestmark = pytest.mark.gpu


def _cornell_exposure(ex):
    return dict(light_pre_exposure=ex["light_pre_exposure"], environment_brightness=ex["environment_brightness"])


# The cases as data (scene factory, grid, config, frames, z_far, exposure, offsets
# expected), so that the oracle side can be run alone on the CPU.
def case_cornell_short_chunks():
    """1,080 rays, not a multiple of 64; 27 probes over the 8 partitions: chunks end
    inside a pool (fewer than 64 rays) and pools straddle partition ends."""
    sc, ex = S.cornell_box()
    grid = D.ProbeGrid((3, 3, 3), (0.8, 0.8, 0.8), (-0.8, 0.2, -0.8))
    cfg = D.DDGIConfig(rays_per_probe=40, probe_updates_per_frame=27, compute_probe_offsets=False, max_rays_per_probe=40, max_probe_updates=27)
    return sc, grid, cfg, 3, ex["z_far"], _cornell_exposure(ex), False


def case_cornell_few_probes():
    """5 probes, fewer than partitions (empty partitions, stealing): 80 rays in two
    short chunks, R = 16 in records strided by Rmax = 32, offsets on. The windows start
    at probe 505 of 512, so the second one wraps past the grid's end."""
    sc, ex = S.cornell_box()
    grid = D.ProbeGrid((8, 8, 8), (0.257, 0.257, 0.257), (-0.9, 0.1, -0.9))
    cfg = D.DDGIConfig(rays_per_probe=16, probe_updates_per_frame=5, compute_probe_offsets=True, max_rays_per_probe=32, max_probe_updates=5)
    return sc, grid, cfg, 4, ex["z_far"], _cornell_exposure(ex), True


def case_cornell_one_probe():
    """16 rays, fewer than lanes: every lane idle with a 16-record chunk, and the
    supply is exhausted at the first grab after it. The windows start at the grid's
    centre probe (the corner probe 0 gathers no light in two frames)."""
    sc, ex = S.cornell_box()
    grid = D.ProbeGrid((3, 3, 3), (0.8, 0.8, 0.8), (-0.8, 0.2, -0.8))
    cfg = D.DDGIConfig(rays_per_probe=16, probe_updates_per_frame=1, compute_probe_offsets=False, max_rays_per_probe=16, max_probe_updates=1)
    return sc, grid, cfg, 2, ex["z_far"], _cornell_exposure(ex), False


def case_features():
    """Masked pass restarted from the lane's in-register ray (the pool is not read
    again), alpha test, mirrored instance; R = 72 is no multiple of 8."""
    sc = scenes.features_scene()
    grid = D.ProbeGrid((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))
    cfg = D.DDGIConfig(rays_per_probe=72, probe_updates_per_frame=50, compute_probe_offsets=True, max_rays_per_probe=72, max_probe_updates=50)
    return sc, grid, cfg, 3, 100.0, dict(light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5), True


def case_soup(serial):
    """6,144 rays in 96 full chunks on a scene whose rays differ widely in length
    (lanes of a wave finish far apart), frames in flight and serial frames. The
    traversal grid is sized by the device (thousands of waves), so here, as in every
    case of this file, a wave that gets a chunk mostly hands all of it out in its
    first refill and finds the supply exhausted at the second; refills that take the
    pool's leftover and a fresh chunk together need more chunks than waves and are
    covered by tests/test_gpu_fullsize.py (8.4 M rays, a probe subset against the
    oracle)."""
    sc = S.soup(64_000, extent=7.0)
    grid = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5))
    cfg = D.DDGIConfig(rays_per_probe=96, probe_updates_per_frame=64, compute_probe_offsets=False, max_rays_per_probe=128, max_probe_updates=64,
                       serial_frames=serial)
    return sc, grid, cfg, 2, 10000.0, dict(light_pre_exposure=1.0, environment_brightness=1.0), False


FIRST_PROBE = {"few_probes": 505, "one_probe": 13}
CASES = {
    "short_chunks": case_cornell_short_chunks,
    "few_probes": case_cornell_few_probes,
    "one_probe": case_cornell_one_probe,
    "features": case_features,
    "soup_pipelined": lambda: case_soup(False),
    "soup_serial": lambda: case_soup(True),
}


def _run_pair_from(first, scene, grid, cfg, frames, z_far, exposure, threads=8):
    """parity.run_pair with the first window at probe `first` (run_pair starts at 0):
    the same updates, reads and reports, every frame."""
    import oracle_lib as O

    ctx = D.DDGIContext(grid, z_far, cfg)
    ctx.set_scene(scene)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(scene, threads)
    node_idx = first
    reports = []
    try:
        for f in range(frames):
            p = D.frame_params(cfg, grid, D.AppState(f), node_idx, **exposure)
            ctx.update(p)
            ctx.synchronize()
            orc.update(p, threads)
            node_idx = (node_idx + p.probe_updates) % grid.probe_count()
            rep = []
            for k, w in RESOURCES.items():
                g, o = ctx.read(w), orc.read(w)
                r = diff_report(k, g, o)
                r["nonzero"] = int(np.count_nonzero(o))
                rep.append(r)
            reports.append(rep)
    finally:
        ctx.close()
        orc.close()
    return reports


@pytest.mark.parametrize("name", list(CASES))
def test_pool_parity(name):
    sc, grid, cfg, frames, z_far, exposure, offsets = CASES[name]()
    if name in FIRST_PROBE:
        first = FIRST_PROBE[name]
        if name == "few_probes":  # the second window wraps
            assert first + cfg.probe_updates_per_frame < grid.probe_count() < first + 2 * cfg.probe_updates_per_frame
        reps = _run_pair_from(first, sc, grid, cfg, frames, z_far, exposure)
    else:
        reps = run_pair(sc, grid, cfg, frames, z_far, exposure)
    assert len(reps) == frames
    _assert_exact(reps, offsets_expected=offsets)


REFL_SIZE = (37, 23)
REFL_CAMERA = dict(eye=(3.5, 3.5, 9.0), target=(3.5, 3.5, 3.5))
REFL_KW = dict(environment_multiplier=1.0, ambient_amount=0.0)


def reflections_inputs():
    sc = S.soup(64_000, extent=7.0)
    grid = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.5, 0.5, 0.5))
    cfg = D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=64, compute_probe_offsets=False, max_rays_per_probe=64, max_probe_updates=64)
    return sc, grid, cfg


def test_pool_list_rays_reflections():
    """The ray-list source: 37 x 23 pixels, a ray count that is no multiple of 64, on
    the small soup; checked as tests/test_gpu_reflections.py checks the raygen."""
    import torch

    import oracle_lib as O
    import reflection_inputs as RI

    z_far = 100.0
    sc, grid, cfg = reflections_inputs()
    ctx = D.DDGIContext(grid, z_far, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    try:
        for f in range(2):
            p = D.frame_params(cfg, grid, D.AppState(f), 0, light_pre_exposure=1.0, environment_brightness=1.0)
            ctx.update(p)
            orc.update(p)
        ctx.synchronize()
        W, H = REFL_SIZE
        cam = RI.camera(W, H, **REFL_CAMERA)
        g, _ = RI.gbuffer(W, H, cam, seed=11)
        want_rad, want_dir = orc.rt_reflections(W, H, cam, g, **REFL_KW)
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
        rad = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
        dirs = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
        node = D.RTReflectionsNode()
        node.execute(ctx, cam, {k: dev[k] for k in ("depth", "material", "normal_velocity")}, dev["blue_noise"], rad, dirs, **REFL_KW)
        got_rad, got_dir = rad.cpu().numpy().view(np.uint16), dirs.cpu().numpy().view(np.uint16)
        for name, got, want in (("radiance", got_rad, want_rad), ("direction", got_dir, want_dir)):
            bad = np.argwhere(np.any(got != want, axis=-1))
            assert bad.size == 0, f"{name}: {len(bad)} pixels differ, first {bad[:4].tolist()}: got {got[tuple(bad[0])].view(np.float16)} want {want[tuple(bad[0])].view(np.float16)}"
        traced = np.any(want_dir != 0, axis=-1)
        assert traced.sum() > W * H // 2 and traced.sum() % 64 != 0
        rl = want_rad.view(np.float16)[..., 3].astype(np.float32)[traced]
        miss_t = min(z_far + 1.0, 10000.0)
        assert (rl < miss_t).any() and (rl == np.float32(np.float16(miss_t))).any()  # both hits and misses
        rough = (g["material"][..., 0] / 255.0 >= 0.6) & (g["depth"] < 1.0 - 1e-6)
        assert ((g["material"][..., 0] == 160) & rough).any() and (got_rad[rough] == 0).all() and (got_dir[rough] == 0).all()
    finally:
        ctx.close()
        orc.close()
