"""The host restatement of the path tracer (csrc/path_tracer_host.cpp over csrc/path_tracer.h,
no GPU) against what can be stated exactly or independently:

- the RNG seed, the two jitter draws and the camera ray of every pixel against numpy (the
  integers exactly, the ray within float32 rounding of a float64 evaluation);
- the all-sky camera: every texel equals multiplier x the bilinear environment fetch, restated
  in numpy float32 over the recorded ray directions (acos and atan2 through the library's own
  ark_fmath entry), bit for bit;
- the primary hit triangle against a float64 brute-force Möller–Trumbore, on at least 99 % of
  the pixels;
- the accumulate step and the reset copy against numpy float32, byte for byte;
- PathTracerNode's frame counts over reset / accumulate / maximum reached / camera change;
- the vertex list's own consistency: the RNG advances by the shader's draw counts per branch,
  a segment starts where the one before ended, radiance only grows by attenuation x something
  finite, the image is the last vertex's radiance rounded to fp16.

- the numpy model of the shaders (tests/path_tracer_model.py, float32 and float64) per path
  vertex: radiance and attenuation in fp16 ulps, the scattered direction absolutely, the RNG
  state after and the decisions exactly, within twice the float32-against-float64 maximum
  measured on the same vertices; vertices where the two models decide differently are left
  out (at most 1 %); nine one-line mutations of the model must each differ on >= 1 %."""
import ctypes as C

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import path_tracer_inputs as I

W, H = I.SIZES[0]


@pytest.fixture(scope="module")
def inside():
    cam = I.case_camera("inside", W, H)
    image, _, vtx, counts = D.path_tracer_host(I.scene(), W, H, cam, frame_index=7, environment_multiplier=I.ENVIRONMENT_MULTIPLIER, vertices=True)
    return cam, image, vtx, counts


def _wang(seed):
    seed = np.asarray(seed, np.uint32)
    seed = (seed ^ np.uint32(61)) ^ (seed >> np.uint32(16))
    seed = seed * np.uint32(9)
    seed = seed ^ (seed >> np.uint32(4))
    seed = seed * np.uint32(0x27D4EB2D)
    return seed ^ (seed >> np.uint32(15))


def _xorshift(s):
    s = np.asarray(s, np.uint32)
    s = s ^ (s << np.uint32(13))
    s = s ^ (s >> np.uint32(17))
    return s ^ (s << np.uint32(5))


def test_seed_jitter_and_camera_ray(inside):
    cam, _, vtx, _ = inside
    ys, xs = np.mgrid[0:H, 0:W].astype(np.uint32)
    with np.errstate(over="ignore"):
        seed = _wang(xs + ys * np.uint32(W) + np.uint32(7) * np.uint32(W * H))
        s1 = _xorshift(seed)
        s2 = _xorshift(s1)
    assert np.array_equal(vtx["rng_before"][:, :, 0], s2)  # two draws before the first segment
    jx, jy = seed.astype(np.float64) / 2.0**32, s1.astype(np.float64) / 2.0**32  # the state BEFORE each step
    Wv = np.asarray(cam["world_from_view"], np.float64).reshape(4, 4).T
    Pv = np.asarray(cam["view_from_projection"], np.float64).reshape(4, 4).T
    dx = (xs + 0.5 + jx) / W * 2 - 1  # the jitter on top of pixel + 0.5: [0.5, 1.5)
    dy = (ys + 0.5 + jy) / H * 2 - 1
    t = np.stack([dx, dy, np.ones_like(dx), np.ones_like(dx)], -1) @ Pv.T
    dv = t[..., :3] / t[..., 3:]
    dv /= np.linalg.norm(dv, axis=-1, keepdims=True)
    want = dv @ Wv[:3, :3].T
    assert np.max(np.abs(vtx["direction"][:, :, 0] - want)) < 4e-7
    assert np.array_equal(vtx["origin"][:, :, 0], np.broadcast_to(Wv[:3, 3].astype(np.float32), (H, W, 3)))
    assert np.all(vtx["tmin"][:, :, 0] == np.float32(I.Z_NEAR))
    later = vtx["status"][:, :, 1:] != abi.PATH_VERTEX_NONE
    assert later.any() and np.all(vtx["tmin"][:, :, 1:][later] == np.float32(1e-4))
    # the library's own sample entry agrees
    lib = abi.load_library()
    st, ray = (C.c_uint32 * 2)(), (C.c_float * 6)()
    wv = np.ascontiguousarray(cam["world_from_view"], np.float32)
    pv = np.ascontiguousarray(cam["view_from_projection"], np.float32)
    assert lib.ark_ddgi_debug_path_tracer_sample(5, 9, W, H, 7, wv.ctypes.data, pv.ctypes.data, st, ray) == 0
    assert (st[0], st[1]) == (int(seed[9, 5]), int(s2[9, 5])) and np.array_equal(np.float32(ray[3:6]), vtx["direction"][9, 5, 0])


def _fmath(op, x, y=None):
    lib = abi.load_library()
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), np.float32)
    out = np.empty_like(x)
    assert lib.ark_ddgi_debug_fmath_host(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size) == 0
    return out


def _env_bilinear(direction):
    """multiplier x texture(environmentMap, sphericalUvFromDirection(d)).rgb in float32, in the
    library's operation order (spherical.glsl:6-13; sampleTexture: repeat wrap, lerp a + (b - a) t)."""
    f = np.float32
    d = direction.reshape(-1, 3).astype(f)
    two_pi, pi = f(6.2831854820251465), f(3.1415927410125732)
    phi = _fmath(3, d[:, 2], d[:, 0])
    theta = _fmath(2, np.clip(d[:, 1], f(-1), f(1)))
    phi = np.where(phi < 0, phi + two_pi, phi).astype(f)
    u, v = phi / two_pi, theta / pi
    tex = I.scene().textures[4]
    texels = np.asarray(tex.data, f).reshape(tex.height, tex.width, 4)
    x, y = u * f(tex.width) - f(0.5), v * f(tex.height) - f(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0).astype(f), (y - y0).astype(f)
    xa, xb = x0.astype(np.int64) % tex.width, (x0.astype(np.int64) + 1) % tex.width
    ya, yb = y0.astype(np.int64) % tex.height, (y0.astype(np.int64) + 1) % tex.height
    lerp = lambda a, b, t: (a + (b - a) * t[:, None]).astype(f)  # noqa: E731
    c = lerp(lerp(texels[ya, xa], texels[ya, xb], fx), lerp(texels[yb, xa], texels[yb, xb], fx), fy)
    return (f(I.ENVIRONMENT_MULTIPLIER) * c[:, :3]).astype(f)


def test_all_sky_is_the_environment():
    for w, h in I.SIZES[:2]:
        cam = I.case_camera("sky", w, h)
        image, _, vtx, counts = D.path_tracer_host(I.scene(), w, h, cam, frame_index=1, environment_multiplier=I.ENVIRONMENT_MULTIPLIER, vertices=True)
        assert counts["missed"] == w * h == counts["vertices"]
        assert np.all(vtx["status"][:, :, 0] == abi.PATH_VERTEX_MISS) and np.all(vtx["status"][:, :, 1:] == abi.PATH_VERTEX_NONE)
        want = _env_bilinear(vtx["direction"][:, :, 0])  # attenuation 1, radiance 0: 0 + 1 * (multiplier * texel)
        assert np.array_equal(vtx["radiance_after"][:, :, 0].reshape(-1, 3).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(image[..., :3].reshape(-1, 3), want.astype(np.float16).view(np.uint16)) and not image[..., 3].any()


def _brute_force_primary(cam, w, h, origin, direction):
    tris, _ = I.world_triangles(I.scene())
    o, d = origin.reshape(-1, 3).astype(np.float64), direction.reshape(-1, 3).astype(np.float64)
    v0, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    p = np.cross(d[:, None, :], e2[None])
    det = np.einsum("tk,ptk->pt", e1, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o[:, None, :] - v0[None]
        u = np.einsum("ptk,ptk->pt", s, p) * inv
        q = np.cross(s, e1[None])
        v = np.einsum("pk,ptk->pt", d, q) * inv
        t = np.einsum("tk,ptk->pt", e2, q) * inv
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= I.Z_NEAR) & (t <= I.Z_FAR)
    return np.where(ok, t, np.inf), u, v


def test_primary_hits_against_float64(inside):
    """The closest triangle of the float64 test whose alpha the masked material passes is the
    restatement's on >= 99 % of the pixels. Records of the host scene are in (instance,
    primitive) order, i.e. world_triangles' order."""
    cam, _, vtx, _ = inside
    t, u, v = _brute_force_primary(cam, W, H, vtx["origin"][:, :, 0], vtx["direction"][:, :, 0])
    sc = I.scene()
    _, owner = I.world_triangles(sc)
    # the alpha test of the masked material (instance 2): the checker's bilinear alpha against 0.5, in float64
    tex = sc.textures[1]
    alpha = np.asarray(tex.data, np.float64).reshape(tex.height, tex.width, 4)[..., 3] / 255.0
    masked = np.flatnonzero(owner == 2)
    first = masked[0]
    for tri in masked:
        hit = np.isfinite(t[:, tri])
        # uv of the quad's corners: (0,0) (1,0) (1,1) (0,1); triangles (0,1,2) and (0,2,3)
        uv = np.array([[0, 0], [1, 0], [1, 1]], np.float64) if (tri - first) % 2 == 0 else np.array([[0, 0], [1, 1], [0, 1]], np.float64)
        bu, bv = u[hit, tri], v[hit, tri]
        tc = (1 - bu - bv)[:, None] * uv[0] + bu[:, None] * uv[1] + bv[:, None] * uv[2]
        x, y = tc[:, 0] * 16 - 0.5, tc[:, 1] * 16 - 0.5
        x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
        fx, fy = x - x0, y - y0
        cl = lambda i: np.clip(i, 0, 15)  # noqa: E731
        a = (alpha[cl(y0), cl(x0)] * (1 - fx) + alpha[cl(y0), cl(x0 + 1)] * fx) * (1 - fy) + (alpha[cl(y0 + 1), cl(x0)] * (1 - fx) + alpha[cl(y0 + 1), cl(x0 + 1)] * fx) * fy
        rows = np.flatnonzero(hit)
        t[rows[a < 0.5], tri] = np.inf
    want = np.where(np.isfinite(t.min(axis=1)), t.argmin(axis=1), 0xFFFFFFFF).reshape(H, W)
    got = vtx["tri"][:, :, 0].astype(np.int64)
    agree = float(np.mean(got == want))
    print(f"primary hits agreeing with float64: {agree:.4f}")
    assert agree >= 0.99


def test_accumulate_and_reset_are_numpy_float32():
    rng = np.random.default_rng(5)
    w, h = 33, 17
    image = rng.uniform(0, 8, (h, w, 4)).astype(np.float16)
    image[0, 0, :3] = (np.inf, np.float16(6e-8), 65504.0)
    image[..., 3] = 0
    acc0 = rng.uniform(0, 8, (h, w, 4)).astype(np.float32)
    lib = abi.load_library()
    for flags, n in ((abi.ARK_PATH_TRACER_RESET, 5), (abi.ARK_PATH_TRACER_ACCUMULATE, 1), (abi.ARK_PATH_TRACER_ACCUMULATE, 2), (abi.ARK_PATH_TRACER_ACCUMULATE, 999)):
        acc = acc0.copy()
        d = D.path_tracer_desc(w, h, I.case_camera("inside", w, h), image.ctypes.data, acc.ctypes.data, flags, 0, n, 1.0)
        assert lib.ark_ddgi_debug_path_tracer_accumulate_host(C.byref(d)) == 0
        frame = image.astype(np.float32)
        if flags == abi.ARK_PATH_TRACER_RESET:
            want = frame  # alpha 0 included
        else:
            want = np.concatenate([(acc0[..., :3] * np.float32(n) + frame[..., :3]) / np.float32(n + 1), np.ones((h, w, 1), np.float32)], -1).astype(np.float32)
        assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), (flags, n)


def test_node_frame_counts():
    node = D.PathTracerNode()
    assert (node.should_accumulate, node.current_accumulated_frames, node.max_accumulated_frames) == (True, 0, 1000)
    R, A = abi.ARK_PATH_TRACER_RESET, abi.ARK_PATH_TRACER_ACCUMULATE
    seen = []

    def frame(first=False, camera=False, uploads=False):
        flags = node.plan(first, camera, uploads)
        seen.append((flags, node.current_accumulated_frames))  # the call's flags and its frameCount
        node.advance(flags)

    frame(first=True)
    frame()
    frame()
    frame(camera=True)
    frame()
    frame(uploads=True)
    assert seen == [(R, 0), (A, 1), (A, 2), (R, 3), (A, 1), (R, 2)] and node.current_accumulated_frames == 1
    node.max_accumulated_frames = 3
    seen.clear()
    for _ in range(4):
        frame()
    assert seen == [(A, 1), (A, 2), (-1, 3), (-1, 3)] and node.current_accumulated_frames == 3  # the maximum reached: no trace
    frame(camera=True)
    assert seen[-1] == (R, 3) and node.current_accumulated_frames == 1
    node.should_accumulate = False
    seen.clear()
    frame()
    frame()
    assert seen == [(R, 1), (R, 1)] and node.current_accumulated_frames == 1


DRAWS_AFTER = {abi.PATH_VERTEX_MISS: (0,), abi.PATH_VERTEX_KILLED: (0, 2, 4), abi.PATH_VERTEX_SCATTERED: (4,), abi.PATH_VERTEX_LAST: (4,)}


def test_vertex_list_is_consistent(inside):
    _, image, vtx, counts = inside
    st = vtx["status"]
    live = st != abi.PATH_VERTEX_NONE
    assert counts["vertices"] == int(live.sum()) and counts["killed"] == int((st == abi.PATH_VERTEX_KILLED).sum())
    assert counts["glass"] == int(vtx["glass"][live].sum()) and counts["alpha_rejected"] == int(vtx["alpha_rejected"][live].sum())
    assert counts["segment8"] == int(live[:, :, 8].sum())
    bits = vtx["shadow_bits"][live]
    lit, occ = bits & 0xFFFF, bits >> 16
    assert np.all(occ & ~lit == 0) and np.all(lit < 8)  # three lights; only a cast ray can be occluded
    pop = lambda a: sum(((a >> k) & 1).astype(np.int64) for k in range(16))  # noqa: E731
    assert counts["occluded"] == int(pop(occ).sum()) and counts["occluded"] + counts["lit"] == int(pop(lit).sum())
    # the draws of each branch: opaque 4 (metal draw, reflect draw, two sample draws) or 2 (absorbed metal),
    # glass 4 or 4 (absorbed after all four draws), V.z <= 0: none; a miss: none
    for status, allowed in DRAWS_AFTER.items():
        sel = st == status
        s = vtx["rng_before"][sel]
        steps = np.full(s.shape, -1)
        cur = s.copy()
        for k in range(5):
            steps[(steps < 0) & (cur == vtx["rng_after"][sel])] = k
            cur = _xorshift(cur)
        assert np.all(np.isin(steps, allowed)), (status, np.unique(steps))
    # a segment starts where the one before ended
    nxt = live[:, :, 1:]
    assert np.all((st[:, :, :-1] == abi.PATH_VERTEX_SCATTERED) == nxt)
    prev = vtx[:, :, :-1][nxt]
    cur = vtx[:, :, 1:][nxt]
    assert np.array_equal(cur["rng_before"], prev["rng_after"]) and np.array_equal(cur["direction"], prev["scattered"])
    assert np.array_equal(cur["attenuation_before"].view(np.uint32), prev["attenuation_after"].view(np.uint32))
    assert np.array_equal(cur["radiance_before"].view(np.uint32), prev["radiance_after"].view(np.uint32))
    want_origin = (prev["origin"] + prev["t"][:, None] * prev["direction"]).astype(np.float32)
    assert np.array_equal(cur["origin"], want_origin)
    # killed paths end with a zero attenuation; the loop's threshold ends the others
    killed = vtx[st == abi.PATH_VERTEX_KILLED]
    assert not killed["attenuation_after"].any()
    last = st == abi.PATH_VERTEX_LAST
    seg = np.broadcast_to(np.arange(16), st.shape)
    a = vtx["attenuation_after"][last].astype(np.float32)
    assert np.all((seg[last] == 15) | ~((a * a).sum(-1) > np.float32(1e-5)))
    # the image is the last vertex's radiance, rounded to nearest even
    depth = live.sum(-1) - 1
    final = np.take_along_axis(vtx["radiance_after"], depth[:, :, None, None], 2)[:, :, 0]
    with np.errstate(over="ignore"):
        assert np.array_equal(image[..., :3], final.astype(np.float16).view(np.uint16)) and not image[..., 3].any()


# ---- the numpy model of the shaders (tests/path_tracer_model.py) against the restatement ------
import path_tracer_model as PM  # noqa: E402

HIT = (abi.PATH_VERTEX_SCATTERED, abi.PATH_VERTEX_KILLED, abi.PATH_VERTEX_LAST)


def _half_ulps(value, reference):
    """|value - reference| in fp16 ulps at the reference's magnitude (the image's format)."""
    ref = np.abs(reference.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.where(ref > 0, ref, 1.0)))
    ulp = np.exp2(np.clip(e, -14, 15) - 10)
    d = np.abs(value.astype(np.float64) - reference.astype(np.float64)) / ulp
    return np.where(np.isfinite(d), d, np.where(np.isnan(value.astype(np.float64)) == np.isnan(reference.astype(np.float64)), 0.0, np.inf)).max(axis=-1)


def _errors(got, ref):
    """Per vertex: fp16 ulps of radiance and attenuation, absolute error of the direction (where
    both sides scatter), and whether the integers (RNG after, killed) differ."""
    both = ~got["killed"] & ~ref["killed"]
    return {"radiance": _half_ulps(got["radiance_after"], ref["radiance_after"]), "attenuation": _half_ulps(got["attenuation_after"], ref["attenuation_after"]),
            "direction": np.where(both, np.abs(got["scattered"].astype(np.float64) - ref["scattered"].astype(np.float64)).max(-1), 0.0),
            "integers": (got["rng_after"] != ref["rng_after"]) | (got["killed"] != ref["killed"]) | (got["goes_on"] != ref["goes_on"])}


@pytest.fixture(scope="module")
def modelled(inside):
    _, _, vtx, _ = inside
    sel = np.isin(vtx["status"], HIT)
    vx = vtx[sel]
    seg = np.broadcast_to(np.arange(16), vtx.shape)[sel]
    pix = np.broadcast_to(np.arange(vtx.shape[0] * vtx.shape[1]).reshape(vtx.shape[0], vtx.shape[1], 1), vtx.shape)[sel]
    m32, m64 = PM.Scene(I.scene(), np.float32), PM.Scene(I.scene(), np.float64)
    f32, f64 = PM.shade(m32, vx, seg, I.Z_FAR), PM.shade(m64, vx, seg, I.Z_FAR)
    host = {"radiance_after": vx["radiance_after"], "attenuation_after": vx["attenuation_after"], "scattered": vx["scattered"], "rng_after": vx["rng_after"],
            "killed": vx["status"] == abi.PATH_VERTEX_KILLED, "goes_on": vx["status"] == abi.PATH_VERTEX_SCATTERED, "shadow_bits": vx["shadow_bits"]}
    flips = (f32["decisions"] != f64["decisions"]).any(-1) | (f32["shadow_bits"] != f64["shadow_bits"])
    return {"vx": vx, "seg": seg, "pix": pix, "m64": m64, "f32": f32, "f64": f64, "host": host, "flips": flips}


# measured on the 48 x 32 inside camera, frame 7 (EXPERIMENTS.md): float32 model against float64 model
# (radiance and attenuation in fp16 ulps, the direction absolute; rounded up in the sixth digit). The bound of
# the restatement is twice these. The attenuation's maximum sits on a vertex whose pdf is 3e-4.
MEASURED = {"radiance": 0.085158, "attenuation": 1.841284, "direction": 4.4e-06}
MEASURED_FLIP_SHARE = 0.0


def _bounds(m):
    keep = ~m["flips"]
    e = _errors(m["f32"], m["f64"])
    for k, v in MEASURED.items():
        assert float(e[k][keep].max()) <= v, (k, float(e[k][keep].max()), v)  # the constants are the measurement
    return {k: 2.0 * v for k, v in MEASURED.items()}, e


def test_restatement_against_the_model_per_vertex(modelled):
    m = modelled
    share = float(m["flips"].mean())
    bounds, e32 = _bounds(m)
    print(f"vertices {len(m['vx'])}, decision flips float32 / float64 {share:.4%}, float32 against float64 maxima "
          f"{ {k: float(e32[k][~m['flips']].max()) for k in bounds} }, integers differing {int(e32['integers'][~m['flips']].sum())}")
    assert share <= 0.01 and share <= MEASURED_FLIP_SHARE + 0.002
    keep = ~m["flips"]
    e = _errors(m["host"], m["f64"])
    worst = {k: float(e[k][keep].max()) for k in bounds}
    print(f"restatement against float64 maxima {worst}, bounds {bounds}; shadow words differing {int((m['host']['shadow_bits'] != m['f64']['shadow_bits'])[keep].sum())}")
    assert not e["integers"][keep].any(), int(e["integers"][keep].sum())
    assert np.array_equal(m["host"]["shadow_bits"][keep], m["f64"]["shadow_bits"][keep])
    for k in bounds:
        assert worst[k] <= bounds[k], (k, worst[k], bounds[k])


def _differing(m, mutated):
    bounds, _ = _bounds(m)
    e = _errors(m["host"], mutated)
    bad = e["integers"] | (m["host"]["shadow_bits"] != mutated["shadow_bits"])
    for k in bounds:
        bad |= e[k] > bounds[k]
    return float((bad & ~m["flips"]).mean())


@pytest.mark.parametrize("mut", ["white_default_normal", "blend_shadows", "masked_alpha_in_shadow", "a2_passed", "normalised_h", "inside_glass_toggles"])
def test_model_catches_shading_mutation(modelled, mut):
    m = modelled
    inside_flag = None
    if mut == "inside_glass_toggles":
        # insideGlass before each vertex if refractions toggled it: the parity of the path's earlier refractions
        refr = m["f64"]["refracted"]
        inside_flag = np.zeros(len(refr), bool)
        state = {}
        for k in np.lexsort((m["seg"], m["pix"])):
            inside_flag[k] = state.get(m["pix"][k], False)
            if refr[k]:
                state[m["pix"][k]] = not inside_flag[k]
    share = _differing(m, PM.shade(m["m64"], m["vx"], m["seg"], I.Z_FAR, inside_flag, mut))
    print(f"{mut}: {share:.2%} of the vertices differ")
    assert share >= 0.01


def test_model_catches_hit_t_on_killed(modelled):
    """A hit program that wrote hitT before returning would let a killed path go on."""
    m = modelled
    mutated = dict(m["f64"])
    mutated["goes_on"] = m["f64"]["goes_on"] | (m["f64"]["killed"] & (m["seg"] + 1 < 16))
    mutated["killed"] = np.zeros_like(m["f64"]["killed"])
    assert _differing(m, mutated) >= 0.01
    assert _differing(m, m["f64"]) == 0.0


def test_model_catches_centred_jitter(inside):
    cam, _, vtx, counts = inside
    bound = 4e-7  # test_seed_jitter_and_camera_ray's
    for mut, want in (("", False), ("jitter_centred", True)):
        _, _, d = PM.camera_rays(cam, W, H, 7, np.float64, mut)
        differ = np.abs(vtx["direction"][:, :, 0] - d).max(-1) > bound
        assert (differ.sum() / counts["vertices"] >= 0.01) == want, (mut, int(differ.sum()))


NEAR_CAMERA = ((0.7, 0.9, 0.66), (0.7, 0.9, -1.0))  # 6 cm in front of the pane, looking through it


def test_primary_hits_one_ulp_and_first_segment_tmin(inside):
    """The float64 closest hit against itself with one-ulp-perturbed rays (the camera's choice),
    and the tmin mutation: from 6 cm in front of the pane, tmin = z_near = 0.1 starts most rays
    behind it; tmin 1e-4 would hit it."""
    _, _, vtx, _ = inside
    m64 = PM.Scene(I.scene(), np.float64)
    o, d = vtx["origin"][:, :, 0].reshape(-1, 3), vtx["direction"][:, :, 0].reshape(-1, 3)
    a = PM.closest_hit(m64, o.astype(np.float64), d.astype(np.float64), I.Z_NEAR, I.Z_FAR)
    b = PM.closest_hit(m64, o.astype(np.float64), np.nextafter(d, np.float32(2.0)).astype(np.float64), I.Z_NEAR, I.Z_FAR)
    assert np.mean(a == b) >= 0.99
    assert np.mean(a == vtx["tri"][:, :, 0].reshape(-1).astype(np.int64)) >= 0.99
    cam = I.camera(W, H, *NEAR_CAMERA)
    _, _, near, _ = D.path_tracer_host(I.scene(), W, H, cam, frame_index=2, environment_multiplier=I.ENVIRONMENT_MULTIPLIER, vertices=True)
    o, d = near["origin"][:, :, 0].reshape(-1, 3).astype(np.float64), near["direction"][:, :, 0].reshape(-1, 3).astype(np.float64)
    got = np.where(near["status"][:, :, 0].reshape(-1) == abi.PATH_VERTEX_MISS, -1, near["tri"][:, :, 0].reshape(-1).astype(np.int64))
    right = np.mean(PM.closest_hit(m64, o, d, I.Z_NEAR, I.Z_FAR) == got)
    mutated = np.mean(PM.closest_hit(m64, o, d, 1e-4, I.Z_FAR) == got)
    print(f"near camera: primary hits agreeing with tmin = z_near {right:.4f}, with tmin = 1e-4 {mutated:.4f}")
    assert right >= 0.99 and mutated <= 0.99


def test_random_float_returns_one_for_the_top_states():
    lib = abi.load_library()
    value, nxt = C.c_float(), C.c_uint32()
    for state, want in ((0xFFFFFFFF, 1.0), (0xFFFFFF80, 1.0), (0xFFFFFF7F, float(np.float32(0xFFFFFF00) / np.float32(2.0**32))), (1, 2.0**-32), (0, 0.0)):
        assert lib.ark_ddgi_debug_path_tracer_random(state, C.byref(value), C.byref(nxt)) == 0
        assert value.value == want, (hex(state), value.value)
        assert nxt.value == int(_xorshift(np.uint32(state)))
