"""Ray-traced local-light shadow masks (RTLocalShadowNode, rt-shadow/raygen.rgen) through
ark_ddgi_rt_local_shadows against the host restatement over the records of the context's
front copy (rt_shadows_host_ctx, opaque class only), byte for byte: the features scene
(masked and translucent geometry that must not shadow), partial tiles, batches against
single-light calls, the empty ray list, 16 lights, a refit, DDGI updates in between."""
import ctypes as C

import numpy as np
import pytest
import torch

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import reflection_inputs as RI
import rt_shadow_inputs as I
from test_rt_shadows_host import MAX_DIFF, model_masks

pytestmark = pytest.mark.gpu

GRID = ((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))


def _context(counting=False):
    grid = D.ProbeGrid(*GRID)
    cfg = D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=144, max_rays_per_probe=64, max_probe_updates=144)
    ctx = D.DDGIContext(grid, 100.0, cfg)
    ctx.set_scene(I.scene())
    if counting:
        ctx.set_counting(True)
    return ctx


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


def _device(ctx, cam, depth, lights, frame, node=True, stream=None, fill=0x55):
    """The masks of one call as uint8 [L, h, w] (prefilled: every byte must be written)."""
    h, w = depth.shape
    dev_depth = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    masks = [torch.full((h, w), fill, dtype=torch.uint8, device="cuda") for _ in lights]
    if node:
        D.RTLocalShadowNode().execute(ctx, cam, dev_depth, lights, masks, frame, stream)
    else:
        ctx.rt_local_shadows(D.rt_shadows_desc(w, h, cam, dev_depth.data_ptr(), lights, [m.data_ptr() for m in masks], frame), stream)
    ctx.synchronize()
    return np.stack([m.cpu().numpy() for m in masks]) if lights else np.zeros((0, h, w), np.uint8)


def _host(ctx, cam, depth, lights, frame, class_mask=1):
    h, w = depth.shape
    masks, counts = D.rt_shadows_host_ctx(ctx, class_mask, w, h, cam, depth, lights, frame)
    return np.stack(masks), counts


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first (light, y, x) {bad[:4].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("size", I.SIZES)
@pytest.mark.parametrize("frame", [0, 5])
def test_features_scene_parity(ctx, size, frame):
    w, h = size
    cam, depth = I.case(w, h)
    got = _device(ctx, cam, depth, I.lights(), frame)
    want, counts = _host(ctx, cam, depth, I.lights(), frame)
    _same(got, want, f"{w}x{h} frame {frame}")
    assert sum(c["occluded"] for c in counts) >= 300 and sum(c["culled"] for c in counts) >= 1000 and counts[0]["sky"] >= 500
    # the opaque-only traversal: what the DDGI path's shadow rays (all classes) would give is another image
    all_classes, _ = _host(ctx, cam, depth, I.lights(), frame, 7)
    assert int(np.count_nonzero(all_classes != got)) >= 1000


def test_single_light_calls_equal_the_batch(ctx):
    w, h = I.SIZES[1]
    cam, depth = I.case(w, h)
    batch = _device(ctx, cam, depth, I.lights(), 5)
    for l, light in enumerate(I.lights()):
        one = _device(ctx, cam, depth, [light], 5)
        _same(one[0], batch[l], f"light {l} alone")


def test_one_pixel(ctx):
    cam = RI.camera(1, 1)
    depth = np.full((1, 1), 0.97, np.float32)
    got = _device(ctx, cam, depth, I.lights(), 2)
    want, _ = _host(ctx, cam, depth, I.lights(), 2)
    _same(got, want, "1x1")


def test_all_sky_is_an_empty_ray_list(ctx):
    cam = RI.camera(8, 8)
    depth = np.ones((8, 8), np.float32)
    got = _device(ctx, cam, depth, I.lights(), 1)
    assert got.shape == (3, 8, 8) and not got.any()
    want, counts = _host(ctx, cam, depth, I.lights(), 1)
    _same(got, want, "all sky")
    assert all(c["sky"] == 64 for c in counts)


def test_no_lights_and_empty_image(ctx):
    cam = RI.camera(8, 8)
    assert _device(ctx, cam, np.full((8, 8), 0.97, np.float32), [], 0).shape == (0, 8, 8)
    d = D.rt_shadows_desc(0, 0, cam, 0x1000, I.lights(), [0x2000, 0x3000, 0x4000], 0)  # nothing is enqueued: the pointers are not followed
    ctx.rt_local_shadows(d)
    ctx.synchronize()


def test_sixteen_lights(ctx):
    """Owner bits 0-3 and result bit 31."""
    cam = RI.camera(16, 16)
    tris, inst, cls, _ = I.world(I.scene())
    depth = I.depth_plane(16, 16, cam, tris[cls[inst] == 0])
    lights = I.perturbed_lights(16)
    got = _device(ctx, cam, depth, lights, 6)
    want, counts = _host(ctx, cam, depth, lights, 6)
    _same(got, want, "16 lights")
    assert counts[15]["lit"] > 0 and sum(c["occluded"] for c in counts) > 0


def test_two_batches(ctx):
    """16 lights at 1280 x 820: 1,049,600 pixels x 16 lights x 32 B is just over the 512 MiB
    ray-list budget of one traversal launch, so the lights go in two batches (15 and 1) and
    the second batch adds its bits to the result words of the first."""
    w, h = 1280, 820
    assert w * h * 16 * 32 > 512 << 20 >= (w * h - 2048) * 16 * 32
    cam = RI.camera(w, h)
    g, _ = RI.gbuffer(w, h, cam, seed=23, sky_frac=0.75)  # (the batches are sized by the worst case; the sky keeps the host side short)
    lights = I.perturbed_lights(16, seed=4)
    got = _device(ctx, cam, g["depth"], lights, 7, node=False)
    want, counts = _host(ctx, cam, g["depth"], lights, 7)
    _same(got, want, "two batches")
    assert all(c["lit"] > 0 for c in counts) and sum(c["occluded"] for c in counts[:8]) > 0 and sum(c["occluded"] for c in counts[8:]) > 0


def test_refusals_and_no_scene(ctx):
    cam, depth = I.case(*I.SIZES[0])
    dev = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    h, w = depth.shape
    m = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(3)]
    for change in ("size", "depth", "mask", "repeat", "nan"):
        d = D.rt_shadows_desc(w, h, cam, dev.data_ptr(), I.lights(), [t.data_ptr() for t in m], 0)
        rc_size = C.sizeof(abi.ArkRtShadowsDesc)
        if change == "size":
            rc_size -= 8
        elif change == "depth":
            d.depth = None
        elif change == "mask":
            d.lights[2].out_mask = None
        elif change == "repeat":
            d.lights[2].out_mask = d.lights[1].out_mask
        else:
            d.lights[0].position[1] = float("nan")
        d.struct_size = rc_size
        assert ctx.lib.ark_ddgi_rt_local_shadows(ctx.h, C.byref(d), None) == abi.ARK_DDGI_E_INVALID_ARGUMENT, change
    ctx.synchronize()
    assert not any(t.any().item() for t in m)  # nothing was enqueued
    bare = D.DDGIContext(D.ProbeGrid(*GRID), 100.0, D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=144, max_rays_per_probe=64, max_probe_updates=144))
    d = D.rt_shadows_desc(w, h, cam, dev.data_ptr(), I.lights(), [t.data_ptr() for t in m], 0)
    assert bare.lib.ark_ddgi_rt_local_shadows(bare.h, C.byref(d), None) == abi.ARK_DDGI_E_NO_SCENE
    bare.close()
    with pytest.raises(ValueError):
        D.RTLocalShadowNode().execute(ctx, cam, dev, I.lights(), [t.to(torch.int8) for t in m], 0)


def test_after_a_refit():
    """set_instances moves the plain box by (-0.6, 0, 0.5): the next call traces the refitted BVH."""
    c = _context()
    w, h = I.SIZES[1]
    # The shared depth plane, as for every case: a plane rendered from the moved scene would put
    # shading points on the box face that the move lays exactly in light A's plane z = 0, where
    # the rays run inside the face's plane and the hit test is ill-conditioned in any precision.
    cam, depth = I.case(w, h)
    before = _device(c, cam, depth, I.lights(), 3)
    _same(before, _host(c, cam, depth, I.lights(), 3)[0], "before the move")
    sc = I.scene()
    moved = I.moved_instances(sc)
    c.set_instances(moved)
    after = _device(c, cam, depth, I.lights(), 3)
    _same(after, _host(c, cam, depth, I.lights(), 3)[0], "after the move")
    assert int(np.count_nonzero(after != before)) > 0
    tris, inst, cls, _ = I.world(I.scene_with(sc, moved))
    want, _ = model_masks(tris[cls[inst] == 0], w, h, cam, depth, I.lights(), 3)
    diffs = [int(np.count_nonzero(after[l] != want[l])) for l in range(3)]
    print("after the move: differing bytes per mask against the float64 model", diffs)
    assert max(diffs) <= MAX_DIFF, diffs
    c.close()


def test_interleaved_with_ddgi_updates():
    """update, shadows, update, shadows on one stream: the atlases and the counters are those
    of a run without the shadow calls (they share the spill area and the work streams)."""
    a, b = _context(True), _context(True)
    w, h = I.SIZES[0]
    cam, depth = I.case(w, h)
    dev = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    masks = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    node = D.RTLocalShadowNode()
    for f in range(2):
        p = D.frame_params(a.config, a.grid, D.AppState(f), 0, light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5)
        a.update(p, s.cuda_stream)
        node.execute(a, cam, dev, I.lights(), masks, f, s.cuda_stream)
        b.update(p, s.cuda_stream)
    a.synchronize()
    b.synchronize()
    for which in (abi.ARK_DDGI_ATLAS_IRRADIANCE, abi.ARK_DDGI_ATLAS_VISIBILITY, abi.ARK_DDGI_SURFELS, abi.ARK_DDGI_PROBE_OFFSETS):
        assert np.array_equal(a.read(which), b.read(which)), which
    ca, cb = a.counters(), b.counters()
    assert bytes(ca) == bytes(cb)
    got = np.stack([m.cpu().numpy() for m in masks])
    _same(got, _host(a, cam, depth, I.lights(), 1)[0], "the second call's masks")
    a.close()
    b.close()


def test_larger_image_four_lights(ctx):
    """640 x 360 on the features scene, depth random in [0.95, 0.9995] as
    reflection_inputs.gbuffer makes it (shading points scattered through the frustum)."""
    w, h = 640, 360
    cam = RI.camera(w, h)
    g, _ = RI.gbuffer(w, h, cam, seed=17)
    lights = I.lights() + I.perturbed_lights(1, seed=9)
    got = _device(ctx, cam, g["depth"], lights, 4, node=False)
    want, counts = _host(ctx, cam, g["depth"], lights, 4)
    _same(got, want, "640x360")
    assert sum(c["occluded"] for c in counts) > 1000 and sum(c["lit"] for c in counts) > 1000
