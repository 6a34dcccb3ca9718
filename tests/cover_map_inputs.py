"""Inputs of the sun cover-map tests (test_sun_cover_map.py, test_gpu_sun_cover_map.py):
the soup at the flagship's density, a hand-built scene, and ray origins. Deterministic."""
from __future__ import annotations

import numpy as np

from arkoserenderer_amd import abi
from arkoserenderer_amd import scene as S

# The flagship soup (BASELINE C4): 10 M triangles in a 31 m cube. 20 k triangles at the same
# number per cubic metre fill a cube of 31 * (20e3 / 10e6)^(1/3) m.
SOUP_TRIANGLES = 20_000
SOUP_EXTENT = 31.0 * (SOUP_TRIANGLES / 10_000_000) ** (1.0 / 3.0)
Z_FAR = 100.0  # the tests' contexts: shadow rays reach 2 zFar


def soup_scene() -> S.SceneData:
    return S.soup(SOUP_TRIANGLES, extent=SOUP_EXTENT)


def world_triangles(sc: S.SceneData) -> np.ndarray:
    """(T, 9) float32 world-space triangles of every instance (set_scene's flattening)."""
    out = []
    for inst in sc.instances:
        mesh = sc.meshes[inst["rt_mesh_index"]]
        idx = sc.indices[int(mesh["first_index"]): int(mesh["first_index"]) + 3 * int(inst["triangle_count"])].astype(np.int64)
        p = sc.positions[int(mesh["first_vertex"]) + idx].astype(np.float32)
        M = inst["object_to_world"].reshape(3, 4).astype(np.float32)
        w = (p @ M[:, :3].T + M[:, 3]).astype(np.float32)
        out.append(w.reshape(-1, 9))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def _quad(center, u, v):
    c, u, v = (np.asarray(a, np.float32) for a in (center, u, v))
    return np.stack([c - u - v, c + u - v, c + u + v, c - u + v]).astype(np.float32)


HAND_SUN_DIR = (0.0, -1.0, 0.0)  # straight down: light space is (u, v, w) = (z, x, y)
ROOF_Y = 2.5
ROOF = ((-1.5, 1.5), (-1.0, 2.0))  # x range, z range of the opaque roof quad


def hand_scene() -> S.SceneData:
    """Quads under a sun that shines straight down: a floor, an opaque roof, a quad of the
    masked hit-mask class and one of the blend class (the sun's any-hit traversal accepts
    every class unconditionally: Opaque flag, no alpha test, cull mask 0xff - both must act
    as occluders), a tilted quad, an exactly vertical wall (edge-on: never hit) and a field
    of small tilted quads that sets the cell size. One spot light beside the sun."""
    pos, vtx, idx, meshes, insts = [], [], [], [], []

    def add(P, tris, mat, mask):
        P = np.asarray(P, np.float32)
        fv = sum(p.shape[0] for p in pos)
        fi = sum(i.size for i in idx)
        pos.append(P)
        vx = np.zeros(len(P), dtype=S.VERTEX_DTYPE)
        n = np.cross(P[1] - P[0], P[2] - P[0])
        vx["normal"] = n / np.linalg.norm(n)
        vx["tangent"] = (1, 0, 0, 1)
        vtx.append(vx)
        idx.append(np.asarray(tris, np.uint32).reshape(-1))
        meshes.append((fv, fi, mat))
        inst = np.zeros((), dtype=S.INSTANCE_DTYPE)
        inst["object_to_world"] = np.eye(3, 4, dtype=np.float32).reshape(-1)
        inst["rt_mesh_index"] = len(meshes) - 1
        inst["triangle_count"] = len(tris)
        inst["hit_mask"] = mask
        insts.append(inst)

    Q = [(0, 1, 2), (0, 2, 3)]
    up = lambda c, hx, hz: _quad(c, (0, 0, hz), (hx, 0, 0))  # normal +y
    add(up((0, 0, 0), 4, 4), Q, 0, abi.ARK_RT_HIT_MASK_OPAQUE)  # floor
    (x0, x1), (z0, z1) = ROOF
    add(up(((x0 + x1) / 2, ROOF_Y, (z0 + z1) / 2), (x1 - x0) / 2, (z1 - z0) / 2), Q, 0, abi.ARK_RT_HIT_MASK_OPAQUE)
    add(up((-2.5, 1.5, -2.0), 0.8, 0.8), Q, 1, abi.ARK_RT_HIT_MASK_MASKED)
    add(up((2.5, 1.0, -2.5), 0.8, 0.8), Q, 2, abi.ARK_RT_HIT_MASK_BLEND)
    add(_quad((2.5, 1.8, 2.0), (0, 0.5, 0.9), (0.9, 0.3, 0)), Q, 0, abi.ARK_RT_HIT_MASK_OPAQUE)  # tilted
    add(_quad((-3.0, 1.0, 2.0), (0, 1.0, 0), (0, 0, 1.0)), Q, 0, abi.ARK_RT_HIT_MASK_OPAQUE)  # vertical wall
    rng = np.random.default_rng(11)
    P, T = [], []
    for i in range(12):
        for j in range(12):
            c = (-3.3 + 0.6 * i, 0.3 + 0.2 * rng.random(), -3.3 + 0.6 * j)
            t = rng.uniform(-0.08, 0.08, 2)
            b = len(P)
            P.extend(_quad(c, (0, t[0], 0.15), (0.15, t[1], 0)))
            T.extend([(b, b + 1, b + 2), (b, b + 2, b + 3)])
    add(P, T, 0, abi.ARK_RT_HIT_MASK_OPAQUE)
    m0 = S.default_material()
    m0["color_tint"] = (0.8, 0.7, 0.6, 1.0)
    m1 = S.default_material()
    m1["blend_mode"] = abi.ARK_BLEND_MODE_MASKED
    m1["mask_cutoff"] = 0.5
    m2 = S.default_material()
    m2["blend_mode"] = abi.ARK_BLEND_MODE_TRANSLUCENT
    m2["color_tint"] = (0.2, 0.4, 0.9, 0.5)
    return S.SceneData(
        positions=np.concatenate(pos), vertices=np.concatenate(vtx), indices=np.concatenate(idx),
        meshes=np.array(meshes, dtype=S.MESH_DTYPE), materials=np.array([m0, m1, m2], dtype=S.MATERIAL_DTYPE),
        instances=np.array(insts, dtype=S.INSTANCE_DTYPE), sun=((2.0, 1.9, 1.7), HAND_SUN_DIR),
        spots=[SPOT])


SPOT = S.SpotLight((30.0, 25.0, 20.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.5, 3.4, 0.2), 0.9, -1)


def surface_origins(tris: np.ndarray, n: int, seed: int) -> np.ndarray:
    """n points on the triangles (uniform barycentrics on uniformly chosen triangles): where
    probe rays end and shadow rays start."""
    rng = np.random.default_rng(seed)
    t = tris[rng.integers(0, len(tris), n)].reshape(n, 3, 3)
    a, b = rng.random(n, np.float32), rng.random(n, np.float32)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    p = t[:, 0] + a[:, None] * (t[:, 1] - t[:, 0]) + b[:, None] * (t[:, 2] - t[:, 0])
    return np.ascontiguousarray(p, np.float32)


def volume_origins(tris: np.ndarray, n: int, seed: int, pad: float = 0.05) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0) - pad, v.max(0) + pad
    return np.ascontiguousarray(lo + (hi - lo) * rng.random((n, 3), np.float32), np.float32)


def hand_edge_origins(u0: float, v0: float, inv_cell: float, nx: int, ny: int) -> np.ndarray:
    """Origins of the hand-built scene chosen to sit on the map's cell borders (the grid's
    u0, v0 and cells per metre as the check reports them; u = z, v = x under the straight
    sun), on the roof's edges, diagonal and vertices, each within a few ulp either side, at
    heights just below and above the roof, around tmin below it, and on the floor."""
    cell = 1.0 / np.float32(inv_cell)
    ulp = lambda x, k: np.nextafter(np.float32(x), np.float32(np.inf if k > 0 else -np.inf)) if k else np.float32(x)

    def around(x):
        x = np.float32(x)
        out = [x]
        for k in (1, -1):
            y = x
            for _ in range(3):
                y = ulp(y, k)
                out.append(y)
        return out + [x + np.float32(1e-5), x - np.float32(1e-5), x + np.float32(3e-4), x - np.float32(3e-4)]

    (x0, x1), (z0, z1) = ROOF
    xs, zs = [], []
    for k in range(0, ny + 1, max(1, ny // 24)):
        xs += around(np.float32(v0) + np.float32(k) * cell)
    for k in range(0, nx + 1, max(1, nx // 24)):
        zs += around(np.float32(u0) + np.float32(k) * cell)
    xs += around(x0) + around(x1) + [np.float32(0.123), np.float32(-0.77)]
    zs += around(z0) + around(z1) + [np.float32(0.456), np.float32(1.31)]
    heights = [0.0, 1e-6, ROOF_Y - 0.5, ROOF_Y - 0.026, ROOF_Y - 0.0251, ROOF_Y - 0.025, ROOF_Y - 0.0249, ROOF_Y - 1e-3, ROOF_Y - 1e-6, ROOF_Y,
               ROOF_Y + 1e-6, ROOF_Y + 1e-3, ROOF_Y + 0.5, 1.5 - 0.03, 1.5 + 1e-4, 1.0 - 0.03, 1.0 + 1e-4]
    X, Zc, Y = np.meshgrid(np.array(xs, np.float32), np.array(zs, np.float32), np.array(heights, np.float32), indexing="ij")
    grid = np.stack([X.ravel(), Y.ravel(), Zc.ravel()], 1)
    # the roof's diagonal (its two triangles' shared edge) and its vertices
    t = np.linspace(0, 1, 257, dtype=np.float32)
    diag = np.stack([np.float32(x0) + t * np.float32(x1 - x0), np.zeros_like(t), np.float32(z0) + t * np.float32(z1 - z0)], 1)
    diag2 = np.stack([np.float32(x0) + t * np.float32(x1 - x0), np.zeros_like(t), np.float32(z1) - t * np.float32(z1 - z0)], 1)
    extra = []
    for d in (diag, diag2):
        for h in (0.0, ROOF_Y - 0.5, ROOF_Y - 0.03, ROOF_Y + 1e-4):
            e = d.copy()
            e[:, 1] = h
            extra.append(e)
    return np.ascontiguousarray(np.concatenate([grid] + extra), np.float32)
