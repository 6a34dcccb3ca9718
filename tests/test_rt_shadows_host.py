"""The host restatement of the ray-traced local-light shadow masks (csrc/rt_shadows.h,
rt_shadows_host.cpp through ark_ddgi_debug_rt_shadows_host) without a GPU: known answers of
the shared generator functions, the masks against a float64 numpy model of
rt-shadow/raygen.rgen:33-80 written from the shader text, the opaque-only cull mask, the
node's frameIndex % 8 and the entry's argument checks."""
import ctypes as C

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import oracle_lib as O
import rt_shadow_inputs as I

FRAMES = (0, 3, 13)
MAX_DIFF = 4  # differing bytes per mask of ~6,000 pixels (fp32 restatement against the float64 model)


# ---- the float64 model ------------------------------------------------------------------
def _wang_hash(seed):
    seed = (seed ^ np.uint32(61)) ^ (seed >> np.uint32(16))
    seed = seed * np.uint32(9)
    seed = seed ^ (seed >> np.uint32(4))
    seed = seed * np.uint32(0x27D4EB2D)
    return seed ^ (seed >> np.uint32(15))


def _xorshift(state):
    state = state ^ (state << np.uint32(13))
    state = state ^ (state >> np.uint32(17))
    return state ^ (state << np.uint32(5))


def model_masks(tris, width, height, cam, depth, lights, frame_index, dtype=np.float64):
    """raygen.rgen main() per pixel and light in `dtype` arithmetic, the trace by brute force
    against `tris` ((T, 9) world triangles). Returns uint8 [L, h, w]: 0 sky / outside the
    cone / occluded, 255 lit; and the category per pixel [L, h, w]: 0 sky, 1 culled, 2 lit,
    3 occluded."""
    f = dtype
    Wv = np.asarray(cam["world_from_view"], f).reshape(4, 4).T
    Pv = np.asarray(cam["view_from_projection"], f).reshape(4, 4).T
    ys, xs = np.mgrid[0:height, 0:width]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    d = np.asarray(depth, np.float32).reshape(-1)
    sky = d >= np.float32(1.0) - np.float32(1e-6)
    uv = np.stack([(xs.astype(f) + f(0.5)) / f(width), (ys.astype(f) + f(0.5)) / f(height)], -1)
    ndc = np.concatenate([uv * f(2) - f(1), d.astype(f)[:, None], np.ones((d.size, 1), f)], 1)
    sp = ndc @ (Wv @ Pv).T
    P = sp[:, :3] / sp[:, 3:]
    with np.errstate(over="ignore"):
        state = _wang_hash((np.uint32(frame_index) + np.uint32(1)) * (xs.astype(np.uint32) + ys.astype(np.uint32) * np.uint32(4000)))
        state = _xorshift(state)
        theta = f(2 * np.pi) * (state.astype(f) * f(1.0 / 4294967296.0))
        state = _xorshift(state)
        r = np.sqrt(state.astype(f) * f(1.0 / 4294967296.0))
    disk = np.stack([r * np.cos(theta), r * np.sin(theta)], -1)
    t = np.asarray(tris, f).reshape(-1, 3, 3)
    v0, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    masks = np.zeros((len(lights), height * width), np.uint8)
    cat = np.zeros((len(lights), height * width), np.uint8)
    for li, l in enumerate(lights):
        lp, ld = np.asarray(np.float32(l.position), f), np.asarray(np.float32(l.direction), f)
        cone, radius = f(np.float32(l.outer_cone_angle_cos)), f(np.float32(l.source_radius))
        n = lp - P
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        zs = np.sign(n[:, 2])
        a = f(-1) / (zs + n[:, 2])
        b = n[:, 0] * n[:, 1] * a
        b1 = np.stack([f(1) + zs * n[:, 0] * n[:, 0] * a, zs * b, -zs * n[:, 0]], -1)
        b2 = np.stack([b, zs + n[:, 1] * n[:, 1] * a, -n[:, 1]], -1)
        dk = disk * radius
        to = (lp + dk[:, :1] * b1 + dk[:, 1:] * b2) - P
        dist = np.linalg.norm(to, axis=1)
        L = to / dist[:, None]
        culled = (-L @ ld) < cone
        # any hit in [0.025, dist]
        p = np.cross(L[:, None, :], e2[None])
        det = np.einsum("tk,ptk->pt", e1, p)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = f(1) / det
            s = P[:, None, :] - v0[None]
            u = np.einsum("ptk,ptk->pt", s, p) * inv
            q = np.cross(s, e1[None])
            v = np.einsum("pk,ptk->pt", L, q) * inv
            tt = np.einsum("tk,ptk->pt", e2, q) * inv
        occluded = ((u >= 0) & (v >= 0) & (u + v <= 1) & (tt >= f(0.025)) & (tt <= dist[:, None])).any(axis=1)
        c = np.where(sky, 0, np.where(culled, 1, np.where(occluded, 3, 2))).astype(np.uint8)
        cat[li] = c
        masks[li] = np.where(c == 2, 255, 0)
    return masks.reshape(len(lights), height, width), cat.reshape(len(lights), height, width)


# ---- (a) the shared functions ---------------------------------------------------------------
@pytest.mark.parametrize("frame", [0, 7])
def test_generator_known_answers(frame):
    """pixelSeed / pointInDisk against the oracle's wang_hash, rand_xorshift and fmath: pixel
    (0, 0) (seed 0), and rows whose py * 4000 term wraps uint32 together with frame + 1."""
    lib, orc = abi.load_library(), O.load()
    for px, py in ((0, 0), (5, 3), (95, 63), (1919, 1079), (7, 1073741), (4001, 1073742), (123, 4294967)):
        st = (C.c_uint32 * 3)()
        disk = (C.c_float * 2)()
        assert lib.ark_ddgi_debug_rt_shadows_sample(frame, px, py, st, disk) == 0
        seed = ((frame + 1) * (px + py * 4000)) & 0xFFFFFFFF
        if py > 1073741:
            assert (px + py * 4000) >= 1 << 32  # the wrap-around is exercised
        s0 = orc.oracle_wang_hash(seed)
        s1 = orc.oracle_rand_xorshift(s0)
        s2 = orc.oracle_rand_xorshift(s1)
        assert (st[0], st[1], st[2]) == (s0, s1, s2), (px, py)
        two_pi = np.float32(np.float32(2.0) * np.float32(np.pi))
        theta = np.float32(two_pi * np.float32(np.float32(s1) * np.float32(1.0 / 4294967296.0)))
        r = np.sqrt(np.float32(np.float32(s2) * np.float32(1.0 / 4294967296.0)), dtype=np.float32)
        sin = np.float32(O.fmath(0, np.array([theta], np.float32))[0])
        cos = np.float32(O.fmath(1, np.array([theta], np.float32))[0])
        want = np.array([r * cos, r * sin], np.float32)
        got = np.array([disk[0], disk[1]], np.float32)
        assert got.tobytes() == want.tobytes(), (px, py, got, want)


# ---- (b), (c) the masks ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    return I.world(I.scene())


@pytest.fixture(scope="module")
def host_images(world):
    """{(size, frame): (masks class_mask 1, counts, masks class_mask 7)} computed once."""
    tris, inst, cls, rec = world
    out = {}
    for (w, h) in I.SIZES:
        cam, depth = I.case(w, h)
        for frame in FRAMES:
            m1, c1 = D.rt_shadows_host(rec, cls, 1, w, h, cam, depth, I.lights(), frame)
            m7, _ = D.rt_shadows_host(rec, cls, 7, w, h, cam, depth, I.lights(), frame)
            out[(w, h), frame] = (np.stack(m1), c1, np.stack(m7))
    return out


@pytest.mark.parametrize("size", I.SIZES)
@pytest.mark.parametrize("frame", FRAMES)
def test_host_against_float64_model(world, host_images, size, frame):
    tris, inst, cls, _ = world
    w, h = size
    cam, depth = I.case(w, h)
    got, counts, _ = host_images[size, frame]
    want, cat = model_masks(tris[cls[inst] == 0], w, h, cam, depth, I.lights(), frame)
    diffs = [int(np.count_nonzero(got[l] != want[l])) for l in range(3)]
    print(f"{w}x{h} frame {frame}: differing bytes per mask {diffs}, host counts {counts}")
    assert max(diffs) <= MAX_DIFF, diffs
    assert set(np.unique(got)) <= {0, 255}
    # the counts are the masks'
    for l in range(3):
        c = counts[l]
        assert sum(c.values()) == w * h
        assert c["lit"] == int(np.count_nonzero(got[l] == 255))
        assert c["sky"] == int(np.count_nonzero(depth >= np.float32(1.0) - np.float32(1e-6)))
    # every class is present
    assert sum(c["occluded"] for c in counts) >= 300
    assert sum(c["culled"] for c in counts) >= 1000
    assert counts[0]["sky"] >= 500
    assert all(c["lit"] > 0 for c in counts)
    assert all(abs(int(np.count_nonzero(cat[l] == 3)) - counts[l]["occluded"]) <= MAX_DIFF for l in range(3))


@pytest.mark.parametrize("size", I.SIZES)
def test_float32_model_agrees_with_float64(world, size):
    """Where the 4-byte cap comes from: the model itself in float32 differs from float64 in
    no more bytes than that on these inputs."""
    tris, inst, cls, _ = world
    w, h = size
    cam, depth = I.case(w, h)
    for frame in FRAMES:
        a, _ = model_masks(tris[cls[inst] == 0], w, h, cam, depth, I.lights(), frame)
        b, _ = model_masks(tris[cls[inst] == 0], w, h, cam, depth, I.lights(), frame, np.float32)
        assert max(int(np.count_nonzero(a[l] != b[l])) for l in range(3)) <= MAX_DIFF


@pytest.mark.parametrize("size", I.SIZES)
@pytest.mark.parametrize("frame", FRAMES)
def test_masked_and_translucent_geometry_does_not_shadow(host_images, size, frame):
    """cullMask RT_HIT_MASK_OPAQUE: tracing all three classes (what the DDGI path's shadow
    rays do) gives other masks. Fails if the opaque-only mode is skipped."""
    m1, _, m7 = host_images[size, frame]
    assert int(np.count_nonzero(m1 != m7)) >= 1000
    assert not np.any((m7 == 255) & (m1 == 0))  # more occluders never light a pixel


# ---- (d) the node's frame parameter ---------------------------------------------------------
def test_node_frame_index_modulo_8(world):
    tris, inst, cls, rec = world
    w, h = I.SIZES[0]
    cam, depth = I.case(w, h)
    node = D.RTLocalShadowNode()
    m3, _ = node.execute_host(rec, cls, 1, cam, depth, I.lights(), 3)
    m11, _ = node.execute_host(rec, cls, 1, cam, depth, I.lights(), 11)
    m4, _ = node.execute_host(rec, cls, 1, cam, depth, I.lights(), 4)
    assert all(np.array_equal(a, b) for a, b in zip(m3, m11))
    assert any(not np.array_equal(a, b) for a, b in zip(m3, m4))
    # the raw descriptor does not fold: 11 is another frame than 3
    raw, _ = D.rt_shadows_host(rec, cls, 1, w, h, cam, depth, I.lights(), 11)
    assert any(not np.array_equal(a, b) for a, b in zip(m3, raw))


# ---- (e) the argument checks ----------------------------------------------------------------
def _desc(n_lights=2, w=8, h=8):
    cam, _ = I.case(*I.SIZES[0])
    ls = I.perturbed_lights(n_lights)
    return D.rt_shadows_desc(w, h, cam, 0x1000, ls, [0x2000 + 0x100 * k for k in range(n_lights)], 0)


def test_argument_checks():
    lib = abi.load_library()
    ok, bad = abi.ARK_DDGI_OK, abi.ARK_DDGI_E_INVALID_ARGUMENT
    check = lambda d: lib.ark_ddgi_debug_rt_shadows_check_desc(C.byref(d))  # noqa: E731
    assert lib.ark_ddgi_debug_rt_shadows_check_desc(None) == bad
    assert check(_desc()) == ok
    assert check(_desc(16)) == ok
    assert check(_desc(0)) == ok
    d = _desc()
    d.struct_size -= 4
    assert check(d) == bad
    d = _desc()
    d.depth = None
    assert check(d) == bad
    d = _desc()
    d.lights[1].out_mask = None
    assert check(d) == bad
    d = _desc(3)
    d.lights[2].out_mask = d.lights[0].out_mask
    assert check(d) == bad
    d = _desc(16)
    d.light_count = 17
    assert check(d) == bad
    d = _desc()
    d.lights = None
    assert check(d) == bad
    for field in ("position", "direction"):
        for v in (np.nan, np.inf, -np.inf):
            d = _desc()
            getattr(d.lights[1], field)[2] = v
            assert check(d) == bad, (field, v)
    for field in ("outer_cone_angle_cos", "source_radius"):
        d = _desc()
        setattr(d.lights[0], field, np.nan)
        assert check(d) == bad, field
    for field in ("world_from_view", "view_from_projection"):
        d = _desc()
        getattr(d, field)[5] = np.inf
        assert check(d) == bad, field
    d = _desc(2, 1 << 14, 1 << 14)  # 2^28 pixels: the owner word is (pixel << 4) | light
    assert check(d) == bad
    d = _desc(2, 1 << 14, (1 << 14) - 1)
    assert check(d) == ok
    # the host entries refuse the same
    d = _desc()
    d.depth = None
    assert lib.ark_ddgi_debug_rt_shadows_host(None, 0, None, 0, 1, C.byref(d), None) == bad


def test_empty_calls_are_ok(world):
    _, _, cls, rec = world
    cam, _ = I.case(*I.SIZES[0])
    masks, counts = D.rt_shadows_host(rec, cls, 1, 8, 8, cam, np.ones((8, 8), np.float32), [], 0)
    assert masks == [] and counts == []
    masks, counts = D.rt_shadows_host(rec, cls, 1, 0, 0, cam, np.zeros((0, 0), np.float32), I.lights(), 0)
    assert [m.shape for m in masks] == [(0, 0)] * 3 and all(sum(c.values()) == 0 for c in counts)
