"""Inputs of the ray-traced local-light shadow tests (test_rt_shadows_host.py,
test_gpu_rt_shadows.py): the features scene seen by the reflections tests' camera, a depth
plane computed from the scene's opaque triangles (no rasteriser) with a seeded tenth of the
texels set to sky, and three spot lights. Deterministic; computed once per size and shared."""
from __future__ import annotations

import functools

import numpy as np

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
import cover_map_inputs as CI
import reflection_inputs as RI
import scenes

SIZES = ((96, 64), (97, 61))  # whole 8 x 8 tiles; partial tiles on both edges


def lights():
    """A, B, C as (position, direction, cone half-angle, radius): A and B stand where the
    features scene's spots do, C looks across the room from beside the open wall."""
    c = np.array([-0.75, -0.1, -0.65])
    c /= np.linalg.norm(c)
    spec = (((0.0, 2.9, 0.0), (0.0, -1.0, 0.0), 0.8, 0.025),
            ((-1.8, 2.5, 0.2), (0.6, -0.8, 0.0), 0.6, 0.2),
            ((1.9, 0.6, 1.6), tuple(c), 1.0, 0.1))
    return [D.RTShadowLight(p, d, 2.0 * half, r) for p, d, half, r in spec]


def perturbed_lights(n: int = 16, seed: int = 3):
    """n seeded perturbations of A, B, C."""
    rng = np.random.default_rng(seed)
    base = lights()
    out = []
    for k in range(n):
        b = base[k % 3]
        d = np.asarray(b.direction) + rng.uniform(-0.15, 0.15, 3)
        d /= np.linalg.norm(d)
        out.append(D.RTShadowLight(np.asarray(b.position) + rng.uniform(-0.1, 0.1, 3), d, b.outer_cone_angle * rng.uniform(0.8, 1.2), b.source_radius * rng.uniform(0.5, 2.0)))
    return out


@functools.lru_cache(maxsize=None)
def scene():
    return scenes.features_scene()


def instance_classes(sc) -> np.ndarray:
    """instance -> hit-mask class (0 opaque, 1 masked, 2 translucent)."""
    cls = {abi.ARK_RT_HIT_MASK_OPAQUE: 0, abi.ARK_RT_HIT_MASK_MASKED: 1, abi.ARK_RT_HIT_MASK_BLEND: 2}
    return np.array([cls[int(i["hit_mask"])] for i in sc.instances], np.int32)


def triangle_instances(sc) -> np.ndarray:
    """The instance of every world triangle, in cover_map_inputs.world_triangles' order."""
    return np.concatenate([np.full(int(i["triangle_count"]), k, np.uint32) for k, i in enumerate(sc.instances)])


def moved_instances(sc, instance: int = 3, by=(-0.6, 0.0, 0.5)):
    """The scene's instances with the plain box (instance 3) translated."""
    inst = sc.instances.copy()
    M = inst[instance]["object_to_world"].reshape(3, 4).copy()
    M[:, 3] += np.asarray(by, np.float32)
    inst[instance]["object_to_world"] = M.reshape(-1)
    return inst


def scene_with(sc, instances):
    import copy

    out = copy.copy(sc)
    out.instances = instances
    return out


def world(sc):
    """(triangles (T, 9) float32, instance per triangle, class per instance, records)."""
    tris = CI.world_triangles(sc)
    inst = triangle_instances(sc)
    return tris, inst, instance_classes(sc), D.triangle_records(tris, inst)


def _mat(cam, key):
    return np.asarray(cam[key], np.float64).reshape(4, 4).T  # column-major -> matrix


def depth_plane(width: int, height: int, cam: dict, tris: np.ndarray, sky_frac: float = 0.1, seed: int = 21) -> np.ndarray:
    """The non-linear depth of the closest triangle of `tris` along each pixel's camera ray
    (float64 Möller–Trumbore by brute force; 1.0 where none is hit), then a seeded sky_frac of
    the texels set to 1.0."""
    Wv, Pv = _mat(cam, "world_from_view"), _mat(cam, "view_from_projection")
    ys, xs = np.mgrid[0:height, 0:width]
    ndc = np.stack([(xs + 0.5) / width * 2 - 1, (ys + 0.5) / height * 2 - 1, np.full(xs.shape, 0.5), np.ones(xs.shape)], -1).reshape(-1, 4)
    far = ndc @ (Wv @ Pv).T
    far = far[:, :3] / far[:, 3:]
    eye = Wv[:3, 3]
    d = far - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = tris.astype(np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    p = np.cross(d[:, None, :], e2[None])
    det = np.einsum("tk,ptk->pt", e1, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = eye[None, None, :] - v0[None]
        u = np.einsum("ptk,ptk->pt", np.broadcast_to(s, p.shape), p) * inv
        q = np.cross(np.broadcast_to(s, p.shape), e1[None])
        v = np.einsum("pk,ptk->pt", d, q) * inv
        tt = np.einsum("tk,ptk->pt", e2, q) * inv
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 1e-6)
    tt = np.where(ok, tt, np.inf).min(axis=1)
    hit = np.isfinite(tt)
    X = eye + d * np.where(hit, tt, 1.0)[:, None]
    clip = np.concatenate([X, np.ones((X.shape[0], 1))], 1) @ np.linalg.inv(Wv @ Pv).T
    depth = np.where(hit, clip[:, 2] / clip[:, 3], 1.0).reshape(height, width).astype(np.float32)
    rng = np.random.default_rng(seed)
    depth[rng.random((height, width)) < sky_frac] = 1.0
    return depth


@functools.lru_cache(maxsize=None)
def case(width: int, height: int):
    """(camera, depth plane [h, w] float32) over the scene's opaque triangles. Cached: copy
    before writing to the plane."""
    tris, inst, cls, _ = world(scene())
    cam = RI.camera(width, height)
    return cam, depth_plane(width, height, cam, tris[cls[inst] == 0])
