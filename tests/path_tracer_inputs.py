"""Inputs of the path tracer tests (test_path_tracer_host.py, test_gpu_path_tracer.py): a room
of 166 triangles with every surface kind the path tracer tells apart, three cameras and three
image sizes. Deterministic; made once and shared (copy before writing).

The room is [-2, 2] x [0, 3] x [-2, 2] with the +z wall open to an HDR environment. Floor:
a normal-mapped grid. Walls and ceiling: the default normal map. In it: three checker-alpha
masked quads, a quad of the masked class whose material is opaque (its texture's alpha must not
be tested), two glass panes one behind the other (blend class, texture alpha and tint alpha below 1), a box of metallic
1, the same box mesh under a second RT mesh entry with metallic 0.6 and a metallic-roughness
texture, a mirrored instance of the first (negative determinant), an emissive ceiling panel.
Lights: a sun and two IES spot lights. Every vertex has a unit tangent along its face's u
direction with the handedness that makes w * cross(n, t) point along v."""
from __future__ import annotations

import functools

import numpy as np

from arkoserenderer_amd import abi
from arkoserenderer_amd import scene as S

SIZES = ((48, 32), (33, 17), (1, 1))  # whole tiles; partial tiles on both edges; one pixel
Z_NEAR, Z_FAR = 0.1, 100.0
ENVIRONMENT_MULTIPLIER = 0.75


def camera(width: int, height: int, eye, target, fov_y: float = 1.1) -> dict:
    """CameraState of a right-handed look-at camera with a [0, 1]-depth perspective
    projection: world_from_view and view_from_projection column-major float32[16], z_near, z_far."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, (0.0, 1.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    world_from_view = np.eye(4)
    world_from_view[:3, 0], world_from_view[:3, 1], world_from_view[:3, 2], world_from_view[:3, 3] = s, u, -f, eye
    t = 1.0 / np.tan(fov_y / 2)
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1] = t * height / width, t
    proj[2, 2], proj[2, 3] = Z_FAR / (Z_NEAR - Z_FAR), Z_FAR * Z_NEAR / (Z_NEAR - Z_FAR)
    proj[3, 2] = -1.0
    col = lambda m: np.asarray(m, np.float32).T.reshape(16)  # noqa: E731
    return {"world_from_view": col(world_from_view), "view_from_projection": col(np.linalg.inv(proj)), "z_near": Z_NEAR, "z_far": Z_FAR}


CAMERAS = {
    "inside": ((0.15, 1.45, 1.85), (0.1, 1.05, -1.0)),   # in the room, looking at the back wall past the pane
    "sky": ((0.0, 1.5, 4.0), (0.3, 4.0, 12.0)),          # outside, looking away: every pixel is sky
    "grazing": ((1.55, 0.9, 1.6), (0.35, 0.85, 0.2)),    # along the pane
}


def case_camera(name: str, width: int, height: int) -> dict:
    eye, target = CAMERAS[name]
    return camera(width, height, eye, target)


class _Builder:
    def __init__(self):
        self.pos, self.vtx, self.idx, self.meshes, self.insts = [], [], [], [], []

    def mesh(self, P, N, T, UV, tris, material: int) -> int:
        fv, fi = sum(len(p) for p in self.pos), sum(i.size for i in self.idx)
        self.pos.append(np.asarray(P, np.float32))
        vx = np.zeros(len(P), dtype=S.VERTEX_DTYPE)
        vx["normal"], vx["tangent"], vx["tex_coord"] = N, T, UV
        self.vtx.append(vx)
        self.idx.append(np.asarray(tris, np.uint32).reshape(-1))
        self.meshes.append((fv, fi, material))
        return len(self.meshes) - 1

    def alias(self, mesh: int, material: int) -> int:
        """Another RT mesh entry over the same vertices and indices."""
        fv, fi, _ = self.meshes[mesh]
        self.meshes.append((fv, fi, material))
        return len(self.meshes) - 1

    def instance(self, mesh: int, triangles: int, mask: int, M=None):
        inst = np.zeros((), dtype=S.INSTANCE_DTYPE)
        inst["object_to_world"] = (np.eye(3, 4) if M is None else np.asarray(M)).astype(np.float32).reshape(-1)
        inst["rt_mesh_index"], inst["triangle_count"], inst["hit_mask"] = mesh, triangles, mask
        self.insts.append(inst)


def _grid(center, a, b, n, cells: int, uv_scale: float):
    """A face centre +- a +- b cut into cells x cells quads, counter-clockwise seen against n;
    u runs along a, v along b. Returns (P, N, T, UV, tris)."""
    c, a, b, n = (np.asarray(x, np.float64) for x in (center, a, b, n))
    t = a / np.linalg.norm(a)
    w = 1.0 if np.dot(np.cross(n, t), b) > 0 else -1.0
    P, UV, tris = [], [], []
    for j in range(cells + 1):
        for i in range(cells + 1):
            fu, fv = i / cells, j / cells
            P.append(c + (2 * fu - 1) * a + (2 * fv - 1) * b)
            UV.append((fu * uv_scale, fv * uv_scale))
    flip = np.dot(np.cross(a, b), n) < 0
    for j in range(cells):
        for i in range(cells):
            q = [j * (cells + 1) + i, j * (cells + 1) + i + 1, (j + 1) * (cells + 1) + i + 1, (j + 1) * (cells + 1) + i]
            if flip:
                q = [q[0], q[3], q[2], q[1]]
            tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    k = len(P)
    return np.array(P), np.tile(n, (k, 1)), np.tile(np.append(t, w), (k, 1)), np.array(UV), tris


def _merge(parts):
    P, N, T, UV, tris = [], [], [], [], []
    for p, n, t, uv, tr in parts:
        base = sum(len(x) for x in P)
        P.append(p), N.append(n), T.append(t), UV.append(uv)
        tris += [tuple(base + v for v in tri) for tri in tr]
    return np.concatenate(P), np.concatenate(N), np.concatenate(T), np.concatenate(UV), tris


def _box(half, height):
    """Six faces with their own normals and tangents, base on y = 0."""
    hx, hz = half
    h = height / 2
    faces = [((0, h, hz), (hx, 0, 0), (0, h, 0), (0, 0, 1)), ((0, h, -hz), (-hx, 0, 0), (0, h, 0), (0, 0, -1)),
             ((hx, h, 0), (0, 0, -hz), (0, h, 0), (1, 0, 0)), ((-hx, h, 0), (0, 0, hz), (0, h, 0), (-1, 0, 0)),
             ((0, height, 0), (hx, 0, 0), (0, 0, -hz), (0, 1, 0)), ((0, 0, 0), (hx, 0, 0), (0, 0, hz), (0, -1, 0))]
    return _merge([_grid(c, a, b, n, 1, 1.0) for c, a, b, n in faces])


def _materials():
    def mat(**kw):
        m = S.default_material()
        for k, v in kw.items():
            m[k] = v
        return m

    return [
        mat(base_color=0, normal_map=5, roughness_factor=0.6, metallic_factor=0.0, color_tint=(0.85, 0.8, 0.75, 1.0)),           # 0 floor
        mat(base_color=0, roughness_factor=0.8, metallic_factor=0.0, color_tint=(0.8, 0.8, 0.85, 1.0)),                          # 1 walls
        mat(base_color=1, blend_mode=abi.ARK_BLEND_MODE_MASKED, mask_cutoff=0.5, metallic_factor=0.0, roughness_factor=0.4),     # 2 masked
        mat(base_color=1, metallic_factor=0.0, roughness_factor=0.5),                                                            # 3 opaque material in the masked class
        mat(base_color=6, blend_mode=abi.ARK_BLEND_MODE_TRANSLUCENT, roughness_factor=0.25, metallic_factor=0.0,
            color_tint=(0.9, 0.95, 1.0, 0.6)),                                                                                   # 4 glass
        mat(metallic_factor=1.0, roughness_factor=0.35, color_tint=(0.95, 0.7, 0.35, 1.0)),                                      # 5 metal
        mat(metallic_factor=0.6, roughness_factor=0.5, metallic_roughness=3, clearcoat=0.4, clearcoat_roughness=0.2,
            color_tint=(0.6, 0.8, 0.5, 1.0)),                                                                                    # 6 part metal
        mat(metallic_factor=0.0, roughness_factor=0.9, emissive_factor=(4.0, 3.5, 3.0)),                                         # 7 emissive
    ]


def _textures(rng):
    tex = [S.Texture(8, 8, abi.ARK_TEX_RGBA8_SRGB, rng.integers(120, 255, size=(8, 8, 4)).astype(np.uint8))]
    a = np.zeros((16, 16, 4), np.uint8)
    yy, xx = np.mgrid[0:16, 0:16]
    a[..., :3] = (210, 190, 110)
    a[..., 3] = np.where(((xx // 4 + yy // 4) % 2) == 0, 255, 20)
    tex.append(S.Texture(16, 16, abi.ARK_TEX_RGBA8_SRGB, a, abi.ARK_WRAP_CLAMP_TO_EDGE))
    ies = (0.55 + 0.45 * np.cos(np.linspace(0, 3, 16))[None, :] * np.ones((16, 1))).astype(np.float32)
    tex.append(S.Texture(16, 16, abi.ARK_TEX_R32F, ies, abi.ARK_WRAP_CLAMP_TO_EDGE))
    mr = np.zeros((4, 4, 4), np.uint8)
    mr[..., 1], mr[..., 2], mr[..., 3] = rng.integers(60, 255, (4, 4)), rng.integers(150, 255, (4, 4)), 255
    tex.append(S.Texture(4, 4, abi.ARK_TEX_RGBA8_UNORM, mr))
    env = rng.uniform(0.2, 2.0, size=(4, 8, 4)).astype(np.float32)
    env[1, 5, :3] = (18.0, 16.0, 12.0)
    tex.append(S.Texture(8, 4, abi.ARK_TEX_RGBA32F, env))
    nm = np.zeros((8, 8, 4), np.uint8)
    nm[..., 0], nm[..., 1], nm[..., 2], nm[..., 3] = rng.integers(70, 190, (8, 8)), rng.integers(70, 190, (8, 8)), 255, 255
    tex.append(S.Texture(8, 8, abi.ARK_TEX_RGBA8_UNORM, nm))
    g = np.zeros((4, 4, 4), np.uint8)
    g[..., :3] = rng.integers(200, 255, (4, 4, 3))
    g[..., 3] = rng.integers(60, 200, (4, 4))
    tex.append(S.Texture(4, 4, abi.ARK_TEX_RGBA8_SRGB, g, abi.ARK_WRAP_CLAMP_TO_EDGE))
    return tex


def _build(sun=True, spots=2, classes=(True, True)) -> S.SceneData:
    """classes: (masked, blend) geometry present."""
    rng = np.random.default_rng(11)
    b = _Builder()
    O, M, B = abi.ARK_RT_HIT_MASK_OPAQUE, abi.ARK_RT_HIT_MASK_MASKED, abi.ARK_RT_HIT_MASK_BLEND
    floor = _grid((0, 0, 0), (2, 0, 0), (0, 0, -2), (0, 1, 0), 4, 2.0)
    b.instance(b.mesh(*floor, 0), 32, O)
    shell = _merge([_grid(c, a, v, n, 3, 2.0) for c, a, v, n in (((0, 3, 0), (2, 0, 0), (0, 0, 2), (0, -1, 0)), ((-2, 1.5, 0), (0, 0, 2), (0, 1.5, 0), (1, 0, 0)),
                                                               ((2, 1.5, 0), (0, 0, -2), (0, 1.5, 0), (-1, 0, 0)), ((0, 1.5, -2), (2, 0, 0), (0, 1.5, 0), (0, 0, 1)))])
    b.instance(b.mesh(*shell, 1), 72, O)
    if classes[0]:
        masked = _merge([_grid(c, (0.45, 0, 0), (0, 0.4, 0), (0, 0, 1), 1, 1.0) for c in ((-1.1, 2.0, -0.7), (0.0, 2.1, -0.9), (1.1, 2.0, -0.7))])
        b.instance(b.mesh(*masked, 2), 6, M)
        b.instance(b.mesh(*_grid((-1.5, 0.9, -1.2), (0.35, 0, 0), (0, 0.35, 0), (0, 0, 1), 1, 1.0), 3), 2, M)
    if classes[1]:
        b.instance(b.mesh(*_grid((0.7, 0.9, 0.6), (0.65, 0, 0), (0, 0.6, 0), (0, 0, 1), 2, 1.0), 4), 8, B)
    box = b.mesh(*_box((0.35, 0.3), 0.9), 5)
    b.instance(box, 12, O, [[1, 0, 0, 0.8], [0, 1, 0, 0.0], [0, 0, 1, -0.8]])
    b.instance(b.alias(box, 6), 12, O, [[0.9, 0, 0.3, -0.8], [0, 1, 0, 0.0], [-0.3, 0, 0.9, -0.9]])
    b.instance(box, 12, O, [[-1, 0, 0, -0.05], [0, 1.3, 0, 0.0], [0, 0, 1, -1.5]])  # mirrored
    b.instance(b.mesh(*_grid((0, 2.99, -0.5), (0.5, 0, 0), (0, 0, 0.3), (0, -1, 0), 1, 1.0), 7), 2, O)
    if classes[1]:  # a second pane behind the first: paths cross glass twice (what insideGlass would be about)
        b.instance(b.mesh(*_grid((0.6, 0.9, 0.25), (0.65, 0, 0), (0, 0.6, 0), (0, 0, 1), 2, 1.0), 4), 8, B)
    sd = np.array([0.3, -0.6, -0.8])
    all_spots = [S.SpotLight((30.0, 26.0, 22.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.3, 2.8, -0.2), 0.8, 2),
                 S.SpotLight((12.0, 20.0, 28.0), (0.6, -0.8, 0.0), (0.0, 0.0, 1.0), (0.8, 0.6, 0.0), (-1.8, 2.5, 0.2), 0.6, 2)]
    return S.SceneData(positions=np.concatenate(b.pos), vertices=np.concatenate(b.vtx), indices=np.concatenate(b.idx), meshes=np.array(b.meshes, dtype=S.MESH_DTYPE),
                       materials=np.array(_materials(), dtype=S.MATERIAL_DTYPE), instances=np.array(b.insts, dtype=S.INSTANCE_DTYPE), textures=_textures(rng),
                       sun=((2.2, 2.0, 1.8), tuple(sd / np.linalg.norm(sd))) if sun else None, spots=all_spots[:spots], environment_texture=4)


@functools.lru_cache(maxsize=None)
def scene() -> S.SceneData:
    return _build()


@functools.lru_cache(maxsize=None)
def scene_opaque_only() -> S.SceneData:
    """No masked and no blend class: the traversal's roots 1 and 2 are -1."""
    return _build(classes=(False, False))


def moved_instances(sc: S.SceneData, instance: int = 5, by=(0.25, 0.0, 0.35)):
    """The scene's instances with the metal box (instance 5 of scene()) translated."""
    inst = sc.instances.copy()
    M = inst[instance]["object_to_world"].reshape(3, 4).copy()
    M[:, 3] += np.asarray(by, np.float32)
    inst[instance]["object_to_world"] = M.reshape(-1)
    return inst


def world_triangles(sc: S.SceneData):
    """(triangles (T, 3, 3) float64 in world space, instance per triangle) in instance order."""
    tris, owner = [], []
    for k, inst in enumerate(sc.instances):
        mesh = sc.meshes[inst["rt_mesh_index"]]
        idx = sc.indices[mesh["first_index"]: mesh["first_index"] + 3 * inst["triangle_count"]].astype(np.int64)
        p = sc.positions[mesh["first_vertex"] + idx].astype(np.float32)
        M = inst["object_to_world"].reshape(3, 4).astype(np.float32)
        w = (p @ M[:, :3].T + M[:, 3]).astype(np.float32)  # the library's fp32 transform is not restated: close enough for a 99 % check
        tris.append(w.reshape(-1, 3, 3).astype(np.float64))
        owner.append(np.full(int(inst["triangle_count"]), k, np.int64))
    return np.concatenate(tris), np.concatenate(owner)
