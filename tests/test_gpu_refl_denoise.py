"""The reflection denoiser passes on the device (ark_ddgi_rt_reflections_denoise:
k_refl_history_copy, k_refl_reproject, k_refl_prefilter, k_refl_resolve_temporal) against
the host restatement of the same functions (csrc/refl_denoise.h), byte for byte, on all nine
written planes after every frame of refl_denoise_inputs' three-frame sequence."""
import numpy as np
import pytest
import torch

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import compose_inputs as CI
import reflection_inputs as RI
import refl_denoise_inputs as I
import scenes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (9, 7), (29, 19), (64, 40), (136, 72)]  # 136 x 72: 153 tiles = 39 workgroups, a row of partial tiles


def _context(scene=False):
    grid = D.ProbeGrid((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))
    cfg = D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=144, max_rays_per_probe=64, max_probe_updates=144)
    ctx = D.DDGIContext(grid, 100.0, cfg)
    if scene:
        ctx.set_scene(scenes.features_scene())
    return ctx, grid, cfg


def _to_device(planes):
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if v.dtype == np.uint16 else np.ascontiguousarray(v)).cuda() for k, v in planes.items()}


def _to_host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _differing(got, want):
    """texels whose bytes differ"""
    g, w = got.reshape(got.shape[0], got.shape[1], -1), want.reshape(want.shape[0], want.shape[1], -1)
    return np.argwhere(np.any(g.view(np.uint8) != w.view(np.uint8), axis=-1))


def _run_device(ctx, w, h, state, frame, f, stream=None):
    cam, planes = frame
    dev_in = _to_device(planes)
    addr = {k: t.data_ptr() for k, t in {**dev_in, **state}.items()}
    torch.cuda.synchronize()
    ctx.rt_reflections_denoise(D.refl_denoise_desc(w, h, cam, addr, I.frame_flags(f)), stream)
    ctx.synchronize()
    return dev_in


@pytest.fixture(scope="module")
def ctx():
    c, _, _ = _context()
    yield c
    c.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_sequence_equals_host_restatement(ctx, w, h):
    """No scene is set: the entry needs none."""
    want = I.host_sequence(w, h)
    state = _to_device(I.fresh_planes(w, h))
    for f, frame in enumerate(I.sequence(w, h)):
        _run_device(ctx, w, h, state, frame, f)
        for k in I.WRITTEN:
            bad = _differing(_to_host(state[k]), want[f][k])
            assert bad.size == 0, f"{w}x{h} frame {f} {k}: {len(bad)} texels differ, first {bad[:4].tolist()}"


def test_poison_shows_what_is_written(ctx):
    """From poisoned planes: the non-glossy pixels of reproject's three planes keep the
    pattern, every texel of the other six is written; and the bytes are the host's from the
    same poisoned start."""
    w, h = 29, 19
    frame = I.sequence(w, h)[0]
    host = I.fresh_planes(w, h, poison=True)
    D.refl_denoise_host(w, h, frame[0], dict(frame[1], **host), abi.ARK_REFL_DENOISE_FIRST_FRAME)
    state = _to_device(I.fresh_planes(w, h, poison=True))
    _run_device(ctx, w, h, state, frame, 0)
    g = I.glossy(frame[1])
    assert g.any() and (~g).any()
    for k in I.WRITTEN:
        got = _to_host(state[k])
        assert _differing(got, host[k]).size == 0, k
        poisoned = np.all(got.reshape(got.shape[0], got.shape[1], -1) == (I.POISON16 if got.dtype == np.uint16 else I.POISON32), axis=-1)
        if k in I.PARTIAL:
            assert poisoned[~g].all() and not poisoned[g].any(), k
        else:
            assert not poisoned.any(), k


def test_disabled_copies_radiance(ctx):
    w, h = 29, 19
    frame = I.sequence(w, h)[1]
    state = _to_device(I.fresh_planes(w, h, poison=True))
    dev_in = _to_device(frame[1])
    addr = {k: t.data_ptr() for k, t in {**dev_in, **state}.items()}
    ctx.rt_reflections_denoise(D.refl_denoise_desc(w, h, frame[0], addr, abi.ARK_REFL_DENOISE_DISABLED))
    ctx.synchronize()
    assert np.array_equal(_to_host(state["resolved"]), frame[1]["radiance"])
    for k in I.WRITTEN:
        if k != "resolved":
            assert np.array_equal(_to_host(state[k]), I.fresh_planes(w, h, poison=True)[k]), k


def test_side_stream_interleaved_with_updates():
    """The denoiser on a torch side stream between updates of the same context queued on
    another, no host synchronisation in between: the same bytes."""
    ctx, grid, cfg = _context(scene=True)
    w, h = 64, 40
    want = I.host_sequence(w, h)
    seq = I.sequence(w, h)
    state = _to_device(I.fresh_planes(w, h))
    dev_in = [_to_device(planes) for _, planes in seq]
    s_upd, s_dn = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for f, (cam, _) in enumerate(seq):
        ctx.update(D.frame_params(cfg, grid, D.AppState(f), 0, light_pre_exposure=1.0, environment_brightness=0.5), s_upd.cuda_stream)
        addr = {k: t.data_ptr() for k, t in {**dev_in[f], **state}.items()}
        ctx.rt_reflections_denoise(D.refl_denoise_desc(w, h, cam, addr, I.frame_flags(f)), s_dn.cuda_stream)
    ctx.synchronize()
    for k in I.WRITTEN:
        assert _differing(_to_host(state[k]), want[2][k]).size == 0, k
    ctx.close()


def test_raygen_denoise_compose_end_to_end():
    """The features scene after two updates: the node's raygen then denoise on the device;
    `resolved` equals the host denoise of the device's raygen output, and the compose of it
    equals the compose of that host plane. With its old arguments (a camera without the
    denoiser's fields) the node runs the raygen alone and writes the same radiance."""
    ctx, grid, cfg = _context(scene=True)
    for f in range(2):
        ctx.update(D.frame_params(cfg, grid, D.AppState(f), 0, light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5))
    w, h = 48, 32
    cam = I.cameras(w, h)[0]
    g, _ = RI.gbuffer(w, h, cam, seed=11)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    gb = {k: dev[k] for k in ("depth", "material", "normal_velocity")}
    kw = dict(environment_multiplier=0.5, ambient_amount=0.05)
    rad, dirs = (torch.zeros((h, w, 4), dtype=torch.int16, device="cuda") for _ in range(2))
    old_rad, old_dirs = (torch.zeros((h, w, 4), dtype=torch.int16, device="cuda") for _ in range(2))
    old_cam = {k: cam[k] for k in ("world_from_view", "view_from_projection")}
    assert D.RTReflectionsNode().execute(ctx, old_cam, gb, dev["blue_noise"], old_rad, old_dirs, **kw) is None
    node = D.RTReflectionsNode()
    assert node.denoise_enabled and node.temporal_stability == 0.7 and node.relative_first_frame
    resolved = node.execute(ctx, cam, gb, dev["blue_noise"], rad, dirs, **kw)
    ctx.synchronize()
    assert resolved is node.denoise_planes["resolved"] and not node.relative_first_frame
    assert torch.equal(rad, old_rad) and torch.equal(dirs, old_dirs) and np.count_nonzero(_to_host(rad)) > 0
    host = I.fresh_planes(w, h)
    planes = {"radiance": _to_host(rad), "depth": g["depth"], "material": g["material"], "normal_velocity": g["normal_velocity"]}
    D.refl_denoise_host(w, h, cam, dict(planes, **host), abi.ARK_REFL_DENOISE_FIRST_FRAME)
    for k in I.WRITTEN:
        assert _differing(_to_host(node.denoise_planes[k].view(torch.int16) if node.denoise_planes[k].dtype == torch.float16 else node.denoise_planes[k]), host[k]).size == 0, k
    assert np.any(host["resolved"] != planes["radiance"])  # the prefilter did something
    ccam = CI.camera(w, h, eye=I.EYES[0], target=I.TARGETS[0])
    cg = dict(CI.gbuffer(w, h, seed=3), depth=g["depth"], material=g["material"], normal_velocity=g["normal_velocity"])
    cdev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in cg.items()}
    outs = []
    for refl in (resolved.view(torch.int16), torch.from_numpy(host["resolved"].view(np.int16)).cuda()):
        out = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
        addr = {k: t.data_ptr() for k, t in cdev.items()}
        addr.update(reflections=refl.data_ptr(), reflection_direction=dirs.data_ptr())
        ctx.lighting_compose(w, h, abi.ARK_COMPOSE_DEFAULT_FLAGS, ccam, addr, out.data_ptr())
        ctx.synchronize()
        outs.append(_to_host(out))
    assert np.array_equal(outs[0], outs[1]) and np.count_nonzero(outs[0]) > 0
    # a resize allocates anew and is a relative first frame again
    node.allocate_denoise_planes(16, 8, "cuda")
    assert node.relative_first_frame and all(int(t.count_nonzero()) == 0 for t in node.denoise_planes.values())
    ctx.close()
