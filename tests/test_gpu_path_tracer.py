"""The path tracer (PathTracerNode, pathtracer/*.rgen|rchit|rahit|rmiss) through
ark_ddgi_path_trace against the host restatement over the context's own scene
(path_tracer_host_ctx), byte for byte in the RGBA16F image and the RGBA32F accumulation plane.
The planes are prefilled with a pattern: every texel must be written.

The 48 x 32 cases from inside the room also assert, from the restatement's vertex counts, that
their ground was reached: at least 200 glass vertices, 200 candidates refused by the alpha
test, 100 killed paths, 50 paths with a segment 8, 300 occluded and 300 lit shadow rays. Every
parity case runs at 48 x 32 and asserts them, except where the case itself rules a count out
(no lights: no shadow rays; no masked or blend class: no glass, no alpha test), which keeps
the others, and the 33 x 17 and 1 x 1 frames of test_room_parity, which have too few pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import path_tracer_inputs as I

pytestmark = pytest.mark.gpu

GRID = ((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))
CFG = dict(rays_per_probe=64, probe_updates_per_frame=144, max_rays_per_probe=64, max_probe_updates=144)
GROUND = {"glass": 200, "alpha_rejected": 200, "killed": 100, "segment8": 50, "occluded": 300, "lit": 300}
IMAGE_FILL, ACC_FILL = 0x5555, 123.25


def _context(scene=None, counting=False):
    ctx = D.DDGIContext(D.ProbeGrid(*GRID), I.Z_FAR, D.DDGIConfig(**CFG))
    ctx.set_scene(scene if scene is not None else I.scene())
    if counting:
        ctx.set_counting(True)
    return ctx


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


def _device(ctx, w, h, cam, frame=0, flags=0, accumulated=0, acc=None, batch=0, stream=None):
    """(image uint16 [h, w, 4], accumulation float32 [h, w, 4] or None) of one call."""
    image = torch.full((h, w, 4), IMAGE_FILL, dtype=torch.int16, device="cuda")
    dev_acc = None
    if flags:
        dev_acc = torch.from_numpy(np.ascontiguousarray(acc, np.float32)).cuda() if acc is not None else torch.full((h, w, 4), ACC_FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    d = D.path_tracer_desc(w, h, cam, image.data_ptr(), dev_acc.data_ptr() if dev_acc is not None else None, flags, frame, accumulated, I.ENVIRONMENT_MULTIPLIER, batch)
    ctx.path_trace(d, stream)
    ctx.synchronize()
    return image.cpu().numpy().view(np.uint16), (dev_acc.cpu().numpy() if dev_acc is not None else None)


def _host(ctx, w, h, cam, frame=0, flags=0, accumulated=0, acc=None):
    image, out, _, counts = D.path_tracer_host_ctx(ctx, w, h, cam, flags, frame, accumulated, I.ENVIRONMENT_MULTIPLIER, acc)
    return image, out, counts


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bits = np.uint16 if got.dtype == np.uint16 else np.uint32
    bad = np.argwhere(got.view(bits) != want.view(bits))
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first (y, x, c) {bad[:4].tolist()}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}"


def _ground(counts, what, without=()):
    short = {k: (counts[k], v) for k, v in GROUND.items() if k not in without and counts[k] < v}
    assert not short, f"{what}: ground not reached (count, wanted) {short}"


@pytest.mark.parametrize("size", I.SIZES)
@pytest.mark.parametrize("frame", [0, 7])
def test_room_parity(ctx, size, frame):
    w, h = size
    cam = I.case_camera("inside", w, h)
    got, _ = _device(ctx, w, h, cam, frame)
    want, _, counts = _host(ctx, w, h, cam, frame)
    _same(got, want, f"{w}x{h} frame {frame}")
    assert not np.any(got[..., 3])  # alpha 0
    if size == I.SIZES[0]:
        _ground(counts, f"{w}x{h} frame {frame}")


def test_grazing_the_glass(ctx):
    w, h = I.SIZES[0]
    cam = I.case_camera("grazing", w, h)
    got, _ = _device(ctx, w, h, cam, 3)
    want, _, counts = _host(ctx, w, h, cam, 3)
    _same(got, want, "grazing")
    _ground(counts, "grazing")


@pytest.mark.parametrize("batch", [64, 192])
def test_batches_do_not_change_the_image(ctx, batch):
    """48 x 32 is 6 x 4 tiles = 1,536 slots: batches of 64 (24 of them) and 192 (8) against one."""
    w, h = I.SIZES[0]
    cam = I.case_camera("inside", w, h)
    whole, _ = _device(ctx, w, h, cam, 2)
    parts, _ = _device(ctx, w, h, cam, 2, batch=batch)
    _same(parts, whole, f"batches of {batch}")
    want, _, counts = _host(ctx, w, h, cam, 2)
    _same(whole, want, "one batch")
    _ground(counts, "batches")


def test_all_sky_leaves_an_empty_list(ctx):
    w, h = I.SIZES[0]
    cam = I.case_camera("sky", w, h)
    got, _ = _device(ctx, w, h, cam, 1)
    want, _, counts = _host(ctx, w, h, cam, 1)
    _same(got, want, "all sky")
    assert counts["missed"] == w * h == counts["vertices"]


def test_one_pixel(ctx):
    cam = I.case_camera("inside", 1, 1)
    for frame in (0, 5):
        _same(_device(ctx, 1, 1, cam, frame)[0], _host(ctx, 1, 1, cam, frame)[0], f"1x1 frame {frame}")


def test_zero_lights_and_sun_only():
    c = _context()
    w, h = I.SIZES[0]
    cam = I.case_camera("inside", w, h)
    sc = I.scene()
    for sun, spots, what in ((None, (), "no lights"), (sc.sun, (), "sun only"), (None, sc.spots, "the two spots")):
        c.set_lights(sun, spots)
        got, _ = _device(c, w, h, cam, 4)
        want, _, counts = _host(c, w, h, cam, 4)
        _same(got, want, what)
        lights = sun is not None or len(spots) > 0
        assert (counts["occluded"] + counts["lit"] > 0) == lights, what
        _ground(counts, what, () if lights else ("occluded", "lit"))
    c.close()


def test_scene_without_masked_and_blend_classes():
    c = _context(I.scene_opaque_only())
    w, h = I.SIZES[0]
    cam = I.case_camera("inside", w, h)
    got, _ = _device(c, w, h, cam, 6)
    want, _, counts = _host(c, w, h, cam, 6)
    _same(got, want, "opaque class only")
    assert counts["glass"] == 0 and counts["alpha_rejected"] == 0
    _ground(counts, "opaque class only", ("glass", "alpha_rejected"))
    c.close()


def test_three_accumulated_frames_then_a_reset(ctx):
    """PathTracerNode's sequence: reset (first frame), accumulate x 3, reset (camera changed)."""
    w, h = I.SIZES[0]
    cam = I.case_camera("inside", w, h)
    node = D.PathTracerNode()
    image = torch.full((h, w, 4), IMAGE_FILL, dtype=torch.int16, device="cuda").view(torch.float16)
    acc = torch.full((h, w, 4), ACC_FILL, dtype=torch.float32, device="cuda")
    host_acc, counted = None, []
    for frame, changed in enumerate((False, False, False, False, True)):
        flags = node.plan(frame == 0, changed, False)
        n = node.current_accumulated_frames
        node.execute(ctx, D.AppState(frame), cam, image, acc, I.ENVIRONMENT_MULTIPLIER, camera_changed=changed)
        ctx.synchronize()
        counted.append(node.current_accumulated_frames)
        want_image, host_acc, counts = _host(ctx, w, h, cam, frame, flags, n, host_acc)
        _ground(counts, f"accumulated frame {frame}")
        _same(image.cpu().numpy().view(np.uint16), want_image, f"frame {frame} image")
        _same(acc.cpu().numpy(), host_acc, f"frame {frame} accumulation")
        alpha = acc[..., 3].cpu().numpy()
        assert np.all(alpha == (0.0 if flags == abi.ARK_PATH_TRACER_RESET else 1.0))
    assert counted == [1, 2, 3, 4, 1]


def test_after_a_refit():
    c = _context()
    w, h = I.SIZES[0]
    cam = I.case_camera("inside", w, h)
    before, _ = _device(c, w, h, cam, 3)
    _same(before, _host(c, w, h, cam, 3)[0], "before the move")
    c.set_instances_async(I.moved_instances(I.scene()), None)
    after, _ = _device(c, w, h, cam, 3)
    want, _, counts = _host(c, w, h, cam, 3)
    _same(after, want, "after the move")
    _ground(counts, "after the move")
    assert int(np.count_nonzero(after != before)) > 0
    c.close()


def test_interleaved_with_a_ddgi_update():
    """update, path trace, update on one non-null stream: the atlases are those of a run without
    the path tracer (they share the traversal stack space), and the image is the restatement's."""
    a, b = _context(), _context()
    w, h = I.SIZES[0]
    cam = I.case_camera("inside", w, h)
    image = torch.full((h, w, 4), IMAGE_FILL, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for f in range(2):
        p = D.frame_params(a.config, a.grid, D.AppState(f), 0, light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5)
        a.update(p, s.cuda_stream)
        a.path_trace(D.path_tracer_desc(w, h, cam, image.data_ptr(), None, 0, f, 0, I.ENVIRONMENT_MULTIPLIER), s.cuda_stream)
        b.update(p, s.cuda_stream)
    a.synchronize()
    b.synchronize()
    for which in (abi.ARK_DDGI_ATLAS_IRRADIANCE, abi.ARK_DDGI_ATLAS_VISIBILITY, abi.ARK_DDGI_SURFELS, abi.ARK_DDGI_PROBE_OFFSETS):
        assert np.array_equal(a.read(which), b.read(which)), which
    want, _, counts = _host(a, w, h, cam, 1)
    _same(image.cpu().numpy().view(np.uint16), want, "the second call's image")
    _ground(counts, "between updates")
    a.close()
    b.close()


def test_refusals_enqueue_nothing(ctx):
    w, h = I.SIZES[1]
    cam = I.case_camera("inside", w, h)
    image = torch.full((h, w, 4), IMAGE_FILL, dtype=torch.int16, device="cuda")
    acc = torch.full((h, w, 4), ACC_FILL, dtype=torch.float32, device="cuda")
    for change in ("size", "flag", "both", "no accumulation", "no image", "misaligned", "overlap", "nan"):
        d = D.path_tracer_desc(w, h, cam, image.data_ptr(), acc.data_ptr(), abi.ARK_PATH_TRACER_RESET, 0, 0, I.ENVIRONMENT_MULTIPLIER)
        if change == "size":
            d.struct_size -= 8
        elif change == "flag":
            d.flags = 4
        elif change == "both":
            d.flags = 3
        elif change == "no accumulation":
            d.accumulation = None
        elif change == "no image":
            d.image = None
        elif change == "misaligned":
            d.image = image.data_ptr() + 2
        elif change == "overlap":
            d.accumulation = image.data_ptr()
        else:
            d.world_from_view[5] = float("nan")
        assert ctx.lib.ark_ddgi_path_trace(ctx.h, C.byref(d), None) == abi.ARK_DDGI_E_INVALID_ARGUMENT, change
    ctx.synchronize()
    assert torch.all(image == IMAGE_FILL).item() and torch.all(acc == ACC_FILL).item()
    bare = D.DDGIContext(D.ProbeGrid(*GRID), I.Z_FAR, D.DDGIConfig(**CFG))
    d = D.path_tracer_desc(w, h, cam, image.data_ptr(), None, 0, 0, 0, 1.0)
    assert bare.lib.ark_ddgi_path_trace(bare.h, C.byref(d), None) == abi.ARK_DDGI_E_NO_SCENE
    bare.close()
    ctx.path_trace(D.path_tracer_desc(0, 0, cam, 0x1000, None, 0, 0, 0, 1.0))  # an empty image: OK, the pointer is not followed
    ctx.synchronize()
