"""Planted inputs for the probe path's hit shading (test infrastructure): hit records, lights,
materials and previous-frame atlases built to reach every term of tests/hit_shading_model.py,
in windows of at most 2 * 1024 + 37 rays.

A planted hit names a triangle of the scene and barycentrics inside it, but it need not lie
where its ray meets that triangle: the shaders take the hit point from the ray (origin + t dir)
and everything else from the triangle, and so do the model, the oracle and the kernels. That
is what lets a case put a hit point on a spot light's axis or a normal across a ray.

The scene is scenes.features_scene() (opaque room, masked quads, a translucent quad, a box and
its mirrored, non-uniformly scaled twin; sRGB, UNORM, R32F and RGBA32F textures) plus, outside
the room: a non-uniformly scaled box and a rotated one, one flat +y quad per material variant with uvs from -0.75
to 1.75 (mirrored, clamped and per-axis wraps), a triangle whose vertex normals cancel, one whose vertex normals are the three axes, and
triangles whose first vertex's u puts u W - 0.5 on an integer and one fp32 step to either side.

The grid is sampling_inputs.G1 (5, 3, 4), anisotropic like the write side's (3, 2, 4): atlases a
and b of sampling_inputs.py are made for it and are planted unchanged; `b_inf` is b with some
irradiance texels +inf (metallic 1 over them: 0 * inf).

Every case carries `reach`: minimum values of the model's own counts, asserted by
tests/test_hit_shading_model.py, so that a case that stops reaching its edge fails instead of
passing empty. `reach32` is the same for counts that hold in fp32 only (a light placed at a ray's fp32 hit
point). `class_only` marks rays whose value is not compared (only NaN for NaN), `flip_rays` the
rays whose decisions may differ between the float32 and the float64 model.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from arkoserenderer_amd import abi
from arkoserenderer_amd import scene as S
import hit_shading_model as H
import sampling_inputs as SI
import scenes

GRID = SI.G1
N_PROBES = 60
Z_FAR = 100.0

# material variants of the flat patches: name -> fields
VARIANTS = {
    "plain": dict(roughness_factor=0.5, metallic_factor=0.3),
    "rough0": dict(roughness_factor=0.0, metallic_factor=0.2),
    "rough1": dict(roughness_factor=1.0, metallic_factor=0.0),
    "metal1": dict(roughness_factor=0.6, metallic_factor=1.0),
    "coat1": dict(roughness_factor=0.4, metallic_factor=0.1, clearcoat=1.0, clearcoat_roughness=0.05),
    "coat_rough_above": dict(roughness_factor=0.4, metallic_factor=0.1, clearcoat=0.7, clearcoat_roughness=1.5),
    "emissive_only": dict(roughness_factor=0.5, metallic_factor=0.0, color_tint=(0.0, 0.0, 0.0, 1.0), emissive_factor=(0.7, 0.4, 0.2)),
    "tint0": dict(roughness_factor=0.5, metallic_factor=0.5, color_tint=(0.0, 0.0, 0.0, 1.0)),
}


@functools.lru_cache(maxsize=None)
def scene():
    """(SceneData, names): names maps "box_scaled", "box_rotated", "cancel", "uv_edge", "octant" and every VARIANTS key
    to its instance index."""
    sc = scenes.features_scene()
    rng = np.random.default_rng(31)
    pos, vtx, idx = [sc.positions], [sc.vertices], [sc.indices]
    meshes, mats, insts, tex = list(sc.meshes), list(sc.materials), list(sc.instances), list(sc.textures)
    names = {}

    def add_instance(mesh, tris, mask, M):
        inst = np.zeros((), dtype=S.INSTANCE_DTYPE)
        inst["object_to_world"] = np.asarray(M, np.float32).reshape(-1)
        inst["rt_mesh_index"], inst["triangle_count"], inst["hit_mask"] = mesh, tris, mask
        insts.append(inst)
        return len(insts) - 1

    def add_mesh(P, Nn, UV, tris, mat, M=np.eye(3, 4)):
        fv, fi = sum(len(p) for p in pos), sum(i.size for i in idx)
        pos.append(np.asarray(P, np.float32))
        vx = np.zeros(len(P), dtype=S.VERTEX_DTYPE)
        vx["normal"], vx["tex_coord"], vx["tangent"] = Nn, UV, (1, 0, 0, 1)
        vtx.append(vx)
        idx.append(np.asarray(tris, np.uint32).reshape(-1))
        meshes.append(np.array((fv, fi, mat), dtype=S.MESH_DTYPE))
        return add_instance(len(meshes) - 1, len(tris), abi.ARK_RT_HIT_MASK_OPAQUE, M)

    # the box once more, scaled (2, 0.5, 1.5) without a mirror
    names["box_scaled"] = add_instance(3, 12, abi.ARK_RT_HIT_MASK_OPAQUE, [[2, 0, 0, 4.0], [0, 0.5, 0, 0.0], [0, 0, 1.5, 3.0]])
    # and rotated about z with a scale: a normal matrix that is not its own transpose
    c30, s30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
    names["box_rotated"] = add_instance(3, 12, abi.ARK_RT_HIT_MASK_OPAQUE, [[1.3 * c30, -0.7 * s30, 0, 6.0], [1.3 * s30, 0.7 * c30, 0, 0.0], [0, 0, 1, 3.0]])
    # textures: 5 base colour 16 x 16 UNORM mirrored, 6 emissive 5 x 3 RGBA32F clamp s / mirrored t,
    # 7 base colour 16 x 16 sRGB clamp, 8 IES LUT 16 x 16 R32F varying along both axes
    t5 = rng.integers(30, 255, size=(16, 16, 4)).astype(np.uint8)
    tex.append(S.Texture(16, 16, abi.ARK_TEX_RGBA8_UNORM, t5, abi.ARK_WRAP_MIRRORED_REPEAT))
    t6 = rng.uniform(0.1, 1.5, size=(3, 5, 4)).astype(np.float32)
    tex.append(S.Texture(5, 3, abi.ARK_TEX_RGBA32F, t6, abi.ark_wrap_axes(abi.ARK_WRAP_CLAMP_TO_EDGE, abi.ARK_WRAP_MIRRORED_REPEAT)))
    t7 = rng.integers(30, 255, size=(16, 16, 4)).astype(np.uint8)
    tex.append(S.Texture(16, 16, abi.ARK_TEX_RGBA8_SRGB, t7, abi.ARK_WRAP_CLAMP_TO_EDGE))
    yy, xx = np.mgrid[0:16, 0:16]
    ies = (0.25 + 0.5 * np.cos(xx / 15.0 * 1.4) ** 2 + 0.03 * yy).astype(np.float32)
    tex.append(S.Texture(16, 16, abi.ARK_TEX_R32F, ies, abi.ARK_WRAP_CLAMP_TO_EDGE))
    # one flat +y quad per material variant, uv over [-0.75, 1.75]^2
    for k, (name, fields) in enumerate(VARIANTS.items()):
        m = S.default_material()
        m["base_color"], m["emissive"] = (5, 7, 0)[k % 3], 6
        m["emissive_factor"] = (0.05, 0.04, 0.03)
        m["color_tint"] = (0.9, 0.8, 0.7, 1.0)
        for f, v in fields.items():
            m[f] = v
        mats.append(m)
        c = np.array([4.0 + 0.7 * k, 0.0, -1.0], np.float32)
        P = [c + (-0.3, 0, 0.3), c + (0.3, 0, 0.3), c + (0.3, 0, -0.3), c + (-0.3, 0, -0.3)]
        UV = [(-0.75, -0.75), (1.75, -0.75), (1.75, 1.75), (-0.75, 1.75)]
        names[name] = add_mesh(P, [(0, 1, 0)] * 4, UV, [(0, 1, 2), (0, 2, 3)], len(mats) - 1)
    # vertex normals that cancel at (u, v) = (0.5, 0): b = (0.5, 0.5, 0)
    P = [(4, 0, 1), (4.5, 0, 1), (4.25, 0, 0.6)]
    names["cancel"] = add_mesh(P, [(0, 1, 0), (0, -1, 0), (1, 0, 0)], [(0, 0), (1, 0), (0, 1)], [(0, 1, 2)], len(mats) - len(VARIANTS))
    # u W - 0.5 on an integer (W = 16: u = 3.5 / 16) and one fp32 step to either side, at each
    # triangle's first vertex (b = (1, 0, 0): uv = v0.uv exactly); the same for v
    e = np.float32(3.5 / 16)
    us = [e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1))]
    P, UV, T = [], [], []
    for k, u in enumerate(us):
        P += [(5 + k, 0, 1), (5.3 + k, 0, 1), (5 + k, 0, 0.7)]
        UV += [(u, us[(k + 1) % 3]), (0.9, 0.1), (0.2, 0.8)]
        T.append((3 * k, 3 * k + 1, 3 * k + 2))
    names["uv_edge"] = add_mesh(P, [(0, 1, 0)] * len(P), UV, T, len(mats) - len(VARIANTS))
    # vertex normals e_x, e_y, e_z: the shading normal sweeps the positive octant with (u, v)
    mats.append(S.default_material())
    mats[-1]["roughness_factor"], mats[-1]["metallic_factor"] = 0.5, 0.2
    names["octant"] = add_mesh([(7, 0, 1), (7.5, 0, 1), (7.25, 0, 0.6)], [(1, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 0), (1, 0), (0, 1)], [(0, 1, 2)], len(mats) - 1)
    out = S.SceneData(positions=np.concatenate(pos), vertices=np.concatenate(vtx), indices=np.concatenate(idx),
                      meshes=np.array(meshes, dtype=S.MESH_DTYPE), materials=np.array(mats, dtype=S.MATERIAL_DTYPE),
                      instances=np.array(insts, dtype=S.INSTANCE_DTYPE), textures=tex, sun=sc.sun, spots=sc.spots,
                      environment_texture=sc.environment_texture)
    return out, names


IES = 8
DEFAULT_SPOTS = (S.SpotLight((30.0, 25.0, 20.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 2.9, 0.0), 0.8, IES),
                 S.SpotLight((10.0, 20.0, 30.0), (0.6, -0.8, 0.0), (0.0, 0.0, 1.0), (0.8, 0.6, 0.0), (-1.8, 2.5, 0.2), 0.6, IES))
DEFAULT_SUN = ((2.0, 1.9, 1.7), tuple(float(x) for x in np.array([0.3, -1.0, -0.4]) / np.linalg.norm([0.3, -1.0, -0.4])))


def scene_with(sun, spots):
    return dataclasses.replace(scene()[0], sun=sun, spots=list(spots))


@functools.lru_cache(maxsize=None)
def atlases_b_inf():
    rng = np.random.default_rng(2026)
    irr, vis = (x.copy() for x in SI.atlases_b())
    irr = irr.reshape(-1, 4)
    irr[rng.random(len(irr)) < 0.03, :3] = 0x7C00
    return irr.reshape(-1), vis


ATLASES = {"a": SI.atlases_a, "b": SI.atlases_b, "b_inf": atlases_b_inf}


def model_grid():
    return H.SM.Grid(GRID.grid_dimensions, GRID.probe_spacing, GRID.offset_to_first)


def rays32(case):
    """The window's fp32 ray origins [W * R, 3] and directions (the float32 model's)."""
    o, d = H.rays(model_grid(), case["offsets"], case["params"], np.float32, case["shard"])
    return np.broadcast_to(o, d.shape).reshape(-1, 3), d.reshape(-1, 3)


def _random_hits(rng, sc, n, back=0.15, miss=0.15, instances=None):
    hits = np.zeros(n, H.HIT_DTYPE)
    pool = np.arange(len(sc.instances)) if instances is None else np.asarray(instances)
    inst = pool[rng.integers(0, len(pool), n)]
    hits["instance"] = inst
    hits["primitive"] = (rng.random(n) * sc.instances["triangle_count"][inst]).astype(np.uint32)
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    hits["u"], hits["v"] = (u * 0.98 + 0.005).astype(np.float32), (v * 0.98 + 0.005).astype(np.float32)
    t = (0.2 + 2.8 * rng.random(n)).astype(np.float32)
    kind = rng.random(n)
    hits["t"] = np.where(kind < back, -t, t)
    hits["instance"] = np.where(kind > 1 - miss, H.MISS, hits["instance"])
    return hits


def _case(name, *, K, R, first=0, frame=3, rmax=None, atlas="a", sun=DEFAULT_SUN, spots=DEFAULT_SPOTS, z_far=Z_FAR, ambient=0.15, env=0.5, shard=(0, 1),
          seed=1, back=0.15, miss=0.15, instances=None, plant=None, reach=None, reach32=None):
    sc = scene_with(sun, spots)
    rng = np.random.default_rng(seed)
    grid = model_grid()
    probes = H.window_probes(grid, first, K, shard)
    W = len(probes)
    off = np.zeros((N_PROBES, 4), np.float32)
    off[:, :3] = (rng.random((N_PROBES, 3)) - 0.5) * 0.1
    case = dict(name=name, scene=sc, sun=sun, spots=list(spots), atlas=atlas, z_far=float(z_far), shard=shard, probes=probes, W=W, kmax=max(K, 1),
                rmax=int(rmax or R), offsets=off, class_only=np.zeros(W * R, bool), reach=dict(reach or {}), reach32=dict(reach32 or {}), flip_rays=set(),
                params=dict(frame=int(frame), first=int(first), K=int(K), R=int(R), ambient=float(ambient), environment_multiplier=float(env),
                            z_far=float(z_far)))
    case["hits"] = _random_hits(rng, sc, W * R, back, miss, instances)
    if plant is not None:
        plant(case, rng)
        case["scene"] = scene_with(case["sun"], case["spots"])
    return case


def _front(case, rays, name, prim=0, u=0.3, v=0.3, t=None):
    """Plants front hits on instance `name` at the given rays."""
    h = case["hits"]
    rays = np.atleast_1d(rays)
    h["instance"][rays] = scene()[1][name] if isinstance(name, str) else name
    h["primitive"][rays] = prim
    h["u"][rays], h["v"][rays] = u, v
    h["t"][rays] = np.abs(h["t"][rays]) if t is None else t
    return rays


def _hit_points(case):
    o, d = rays32(case)
    return o + case["hits"]["t"][:, None] * d


# --- the cases' plants ------------------------------------------------------------

def _plant_bary(case, rng):
    n = len(case["hits"])
    pts = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.5)]
    for i in range(n):
        u, v = pts[i % len(pts)]
        inst = (0, 3, 4, scene()[1]["box_scaled"], 1, scene()[1]["box_rotated"])[(i // len(pts)) % 6]
        _front(case, i, inst, prim=i % 2, u=u, v=v)


def _plant_uv(case, rng):
    n = len(case["hits"])
    names = list(VARIANTS)
    for i in range(n):
        if i % 3 == 0:
            _front(case, i, "uv_edge", prim=(i // 3) % 3, u=0.0, v=0.0)  # the first vertex: uv exact
        else:
            _front(case, i, names[i % len(names)], prim=i % 2, u=float(rng.random() * 0.5), v=float(rng.random() * 0.5))


def _plant_materials(case, rng):
    names = list(VARIANTS)
    for i in range(len(case["hits"])):
        _front(case, i, names[i % len(names)], prim=i % 2, u=float(rng.random() * 0.5), v=float(rng.random() * 0.5))


def _plant_cancel(case, rng):
    r = np.arange(0, len(case["hits"]), 4)
    _front(case, r, "cancel", u=0.5, v=0.0)
    case["class_only"][r] = True  # NaN for NaN


def _plant_flat(case, rng):
    names = list(VARIANTS)
    for i in range(len(case["hits"])):
        _front(case, i, names[i % len(names)], prim=i % 2, u=0.3, v=0.3)


def _plant_sun_along_ray(case, rng):
    _plant_flat(case, rng)
    _, d = rays32(case)
    j = int(np.argmax(d[:, 1]))  # the ray most along +y: L = d gives LdotN > 0 on the +y patches
    case["sun"] = (DEFAULT_SUN[0], tuple(float(x) for x in -d[j]))
    case["ray"] = j


def spot(position, direction=(0.0, -1.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), half=0.8, color=(3.0, 2.5, 2.0)):
    return S.SpotLight(color, tuple(float(x) for x in direction), right, up, tuple(float(x) for x in position), float(half), IES)


def _plant_spots(case, rng):
    """Ten spots, each placed relative to the fp32 hit point of one ray on a +y patch."""
    _plant_flat(case, rng)
    P = _hit_points(case)
    up1 = np.float32(1.0)
    spots = [
        spot(P[0] + (0, up1, 0)),                                   # on the axis: angleV = 1, hx = hy = 0
        spot(P[1] + (0, up1, 0), direction=(0.0, -1.0000001, 0.0)),  # angleV above 1: acos = NaN
        spot(P[2] - (0, up1, 0)),                                   # behind the light: angleV <= 0
        spot(P[3] + (np.float32(0.5), up1, np.float32(0.3)), half=float(np.arccos(np.float32(1.0) / np.sqrt(np.float32(1.34))) / 2)),  # the cone's edge: lx ~ 1
        spot(P[4] + (np.float32(2.0), up1, np.float32(0.3)), half=0.3),  # outside the cone: lx above 1
        spot(P[5] + (np.float32(0.25), up1, 0)),                    # hy = 0, hx < 0: the angleH seam
        spot(P[6] + (np.float32(0.25), up1, np.float32(1e-6))),     # just across the seam
        spot(P[7] + (np.float32(-0.25), up1, np.float32(0.3)), half=0.5),
        spot(P[8] + (0, np.float32(0.5), np.float32(0.4)), direction=(0.0, -0.8, -0.6), right=(1.0, 0.0, 0.0), up=(0.0, -0.6, 0.8)),
        spot(P[9] + (np.float32(0.1), np.float32(2.0), 0), half=1.2),
    ]
    case["spots"] = spots
    # ray 1: NaN for NaN. Rays 0, 1 and 5 sit on discontinuities of the lookup (the azimuth on the
    # axis, the angleH seam) that hold exactly in fp32 only, where the spots were placed: the float64
    # model lands beside them, so their decisions may flip and their values are not compared
    case["class_only"][[0, 1, 5]] = True
    case["flip_rays"] = {0, 1, 5}


def _plant_spot_at_hit(case, rng):
    """A spot at a ray's own fp32 hit point: distance 0, inf attenuation, NaN direction; its
    shadow ray has a NaN tmax and counts as lit (hazard 15). `exact_point` must be filled in
    by the test from the oracle's own ray before use (the float32 model's may differ by an ulp)."""
    _plant_flat(case, rng)
    case["spot_at_ray"] = 5
    case["spots"] = [spot(_hit_points(case)[5])]
    case["class_only"][:] = True


def _plant_grazing_highlights(case, rng):
    """Ten rays, each with a spot of its own: the shading normal N (the octant triangle at a
    solved (u, v)) stands across the ray with N.V = c ~ 1e-3, and the spot shines along the
    mirror direction L = 2 (N.V) N - V, so H = normalize(L + V) = N: a grazing specular highlight
    whose V_SmithGGXCorrelated is ~ 1 / c, the one place where NdotV's + 1e-5 shows."""
    _plant_flat(case, rng)
    _, d = rays32(case)
    P = _hit_points(case)
    spots, used = [], []
    for j in range(len(d)):
        V = -d[j].astype(np.float64)
        order = np.argsort(V)
        lo, hi = order[0], order[-1]  # the most negative and the most positive component
        if not (V[lo] < -0.2 and V[hi] > 0.2):
            continue
        s = V[hi] - V[lo]
        b = np.zeros(3)
        b[hi], b[lo] = -V[lo] / s, V[hi] / s  # b.V = 0
        tau = 1e-3 * np.linalg.norm(b) / s
        b[hi], b[lo] = b[hi] + tau, b[lo] - tau
        _front(case, j, "octant", u=np.float32(b[1]), v=np.float32(b[2]))
        N = b / np.linalg.norm(b)
        L = 2 * (N @ V) * N - V
        side = np.cross(L, N)
        side /= np.linalg.norm(side)
        up = np.cross(side, -L)
        # beside the axis and away from the angleH seam (hy = 0, hx < 0)
        spots.append(spot(P[j].astype(np.float64) + 2.0 * L + 0.3 * (0.6 * side + 0.8 * up), direction=-L, right=tuple(side), up=tuple(up), half=0.8,
                          color=(30.0, 25.0, 20.0)))
        used.append(j)
        if len(spots) == 10:
            break
    assert len(spots) == 10
    case["spots"] = spots
    case["rays_planted"] = used


def _plant_backs(case, rng):
    h = case["hits"]
    # t whose 0.2 t lies next to an fp16 rounding boundary (half-way between two fp16 values)
    h16 = np.float16(0.3)
    mid = (np.float32(h16) + np.float32(np.nextafter(h16, np.float16(1)))) / np.float32(2)
    for k, cand in enumerate((mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1)))):
        h["t"][k] = -(np.float32(cand) * np.float32(5))


def _plant_lights_11(case, rng):
    dirs = rng.normal(size=(10, 3))
    dirs[:, 1] = -np.abs(dirs[:, 1]) - 0.3
    spots = []
    for k in range(10):
        d = dirs[k] / np.linalg.norm(dirs[k])
        r = np.cross(d, (0.0, 0.0, 1.0))
        r /= np.linalg.norm(r)
        u = np.cross(r, d)
        spots.append(S.SpotLight((8.0 + k, 9.0, 10.0 - k), tuple(d), tuple(r), tuple(u), tuple(rng.uniform(-1.5, 1.5, 3) + (0, 2.0, 0)), 0.5 + 0.05 * k, IES))
    case["spots"] = spots


def _sun(direction):
    return (DEFAULT_SUN[0], direction)


TINY = float(2.0 ** -100)  # normalize((1, +-TINY, 0)) = (1, +-TINY, 0) exactly: LdotN = -+TINY


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        _case("mixed_r16_a", K=20, first=7, R=16, atlas="a", seed=11, reach=dict(front=150, back=20, miss=20, lit_lights=100)),
        _case("mixed_r37_b_wrapping", K=9, first=55, R=37, rmax=40, atlas="b", seed=12, reach=dict(front=150, back=20, miss=20)),
        _case("mixed_r64_zfar_inf", K=6, first=20, R=64, atlas="a", seed=13, z_far=70000.0, reach=dict(miss=20, inf_channels=20)),
        _case("r1", K=24, first=50, R=1, atlas="a", seed=14, reach=dict(rays=24)),
        _case("zslab_rank1", K=40, first=10, R=16, atlas="b", seed=15, shard=(1, 2), reach=dict(front=50)),
        _case("barycentrics", K=8, R=16, atlas="a", seed=16, plant=_plant_bary, reach=dict(bary_corner=30, bary_edge=30, front=128)),
        _case("uv_edges_wraps", K=8, R=16, atlas="a", seed=17, plant=_plant_uv,
              reach=dict(material_on_texel_boundary=10, material_coordinate_below_0=20, material_coordinate_above_1=1)),
        _case("materials_b_inf", K=8, R=16, atlas="b_inf", seed=18, plant=_plant_materials,
              reach=dict(roughness_zero=10, roughness_one=10, metallic_one=10, metallic_zero=10, clearcoat_one=10, clearcoat_zero=50,
                         clearcoat_roughness_below_clamp=10, clearcoat_roughness_above_clamp=10, emissive_only=10, tint_zero=20)),
        _case("normals_cancel", K=4, R=16, atlas="a", seed=19, plant=_plant_cancel, reach=dict(normal_sum_zero=16, nan_surfels=16)),
        _case("sun_ldotn_zero", K=4, R=16, atlas="a", seed=20, sun=_sun((1.0, 0.0, 0.0)), spots=(), plant=_plant_flat, reach=dict(sun_ldotn_zero=64)),
        _case("sun_ldotn_plus", K=4, R=16, atlas="a", seed=20, sun=_sun((1.0, -TINY, 0.0)), spots=(), plant=_plant_flat,
              reach=dict(sun_ldotn_tiny_positive=64, lit_lights=64)),
        _case("sun_ldotn_minus", K=4, R=16, atlas="a", seed=20, sun=_sun((1.0, TINY, 0.0)), spots=(), plant=_plant_flat,
              reach=dict(sun_ldotn_tiny_negative=64)),
        _case("sun_grazing_ndotv", K=30, R=64, atlas="a", seed=21, spots=(), plant=_plant_flat, reach=dict(grazing_ndotv=1)),
        _case("grazing_highlights", K=4, R=16, atlas="a", seed=36, sun=None, plant=_plant_grazing_highlights, reach=dict(grazing_ndotv=10)),
        _case("sun_along_ray", K=8, R=16, atlas="a", seed=22, spots=(), plant=_plant_sun_along_ray, reach=dict(half_vector_short=1)),
        _case("spots_edges", K=4, R=16, atlas="a", seed=23, sun=None, plant=_plant_spots,
              reach=dict(spot_angle_v_above_1=1, spot_behind=1, spot_lx_above_1=1, spot_ly_near_seam=2, ies_nan_coordinate=1),
              reach32=dict(spot_angle_v_ge_1=2, spot_h_zero=1, spot_ly_clamped=1, spot_lx_near_1=1)),
        _case("lights_none", K=4, R=16, atlas="a", seed=24, sun=None, spots=(), reach=dict(front=30)),
        _case("lights_sun", K=4, R=16, atlas="b", seed=25, spots=(), reach=dict(lit_lights=10)),
        _case("lights_spots", K=4, R=16, atlas="a", seed=26, sun=None, reach=dict(lit_lights=10)),
        _case("lights_11", K=4, R=16, atlas="a", seed=27, plant=_plant_lights_11, reach=dict(lit_lights=200, light_count=11)),
        _case("misses_seam", K=16, R=64, atlas="a", seed=28, miss=1.0, back=0.0, reach=dict(miss=1024, environment_wraps=20)),
        _case("backs", K=16, R=64, atlas="a", seed=29, miss=0.0, back=1.0, plant=_plant_backs, reach=dict(back=1024)),
        _case("fronts", K=16, R=64, atlas="b", seed=30, miss=0.0, back=0.0, reach=dict(front=1024)),
        _case("window_1", K=1, first=59, R=1, atlas="a", seed=31, reach=dict(rays=1)),
        _case("window_1023", K=33, first=40, R=31, atlas="a", seed=32, reach=dict(rays=1023)),
        _case("window_1025", K=25, first=3, R=41, atlas="b", seed=33, reach=dict(rays=1025)),
        _case("window_2085", K=15, first=50, R=139, atlas="a", seed=34, reach=dict(rays=2085)),
    ]
    return {c["name"]: c for c in out}


def spot_at_hit_case():
    return _case("spot_at_hit", K=2, R=16, atlas="a", seed=35, sun=None, plant=_plant_spot_at_hit)


def frame_params(case):
    """The ArkDdgiFrameParams of a case (library and oracle)."""
    import ctypes as C

    q = case["params"]
    p = abi.ArkDdgiFrameParams()
    p.struct_size = C.sizeof(abi.ArkDdgiFrameParams)
    p.frame_index, p.first_probe_index, p.probe_updates, p.rays_per_probe = q["frame"], q["first"], q["K"], q["R"]
    p.hysteresis_irradiance = p.hysteresis_visibility = 0.98
    p.visibility_sharpness = 50.0
    p.ambient_amount, p.environment_multiplier = q["ambient"], q["environment_multiplier"]
    p.delta_time = 1.0 / 60.0
    p.update_offsets = 0
    return p


def config(case):
    from arkoserenderer_amd import ddgi as D

    return D.DDGIConfig(rays_per_probe=case["params"]["R"], probe_updates_per_frame=case["params"]["K"], max_rays_per_probe=case["rmax"],
                        max_probe_updates=case["kmax"])
