"""Python host for the MI355X DDGI path, mirroring the reference node's
interface (arkose/rendering/nodes/DDGINode.h/.cpp) over the C-ABI.

* ``ProbeGrid``   — arkcore/scene/ProbeGrid.h:6-15 (+ Scene::generateProbeGridFromBoundingBox,
                    arkose/scene/Scene.cpp:534-583).
* ``DDGIConfig``  — the node's private members and their defaults (DDGINode.h:25-38).
* ``DDGIContext`` — one ark_ddgi context (device resources of one node on one GPU).
* ``DDGINode``    — name() == "DDGI"; ``execute(app_state)`` is the execute lambda
                    (DDGINode.cpp:132-259): rolling window, first-frame hysteresis,
                    push-constant values. The native C++ node
                    (arkoserenderer_amd/host/rendering/nodes/DDGINode.cpp) is the
                    drop-in for the engine; this mirror drives tests and bench.py.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .scene import SceneData

# ArkDdgiDebugShadeHit as a numpy record (debug_shade)
SHADE_HIT_DTYPE = np.dtype([("instance", np.uint32), ("primitive", np.uint32), ("u", np.float32), ("v", np.float32), ("t", np.float32)])


@dataclass
class ProbeGrid:
    grid_dimensions: tuple  # (x=width, y=height, z=depth)
    probe_spacing: tuple
    offset_to_first: tuple

    def probe_count(self) -> int:
        x, y, z = self.grid_dimensions
        return int(x * y * z)

    @staticmethod
    def from_bounding_box(lo, hi):
        """Scene::generateProbeGridFromBoundingBox (Scene.cpp:534-583) on the scene's
        world AABB: grown by 1 m on every side, 16 probes per axis except the largest,
        which gets 32; spacing = bounds / counts, first probe at the grown minimum
        (fp32 vec3 arithmetic). The largest axis is the reference's rule (:563-570):
        x unless y or z is strictly larger than x, then y if y > z, else z - so a
        y == z tie above x picks z, and ties with x pick x."""
        lo = np.asarray(lo, np.float32) - np.float32(1.0)
        hi = np.asarray(hi, np.float32) + np.float32(1.0)
        bounds = (hi - lo).astype(np.float32)
        largest = 0
        if bounds[1] > bounds[0] or bounds[2] > bounds[0]:
            largest = 1 if bounds[1] > bounds[2] else 2
        counts = np.array([16.0, 16.0, 16.0], np.float32)
        counts[largest] = 32.0
        spacing = (bounds / counts).astype(np.float32)
        return ProbeGrid(tuple(int(v) for v in counts), tuple(float(v) for v in spacing), tuple(float(v) for v in lo))


@dataclass
class DDGIConfig:
    rays_per_probe: int = 256            # m_raysPerProbeInt
    hysteresis_irradiance: float = 0.93  # m_hysteresisIrradiance
    hysteresis_visibility: float = 0.93  # m_hysteresisVisibility
    visibility_sharpness: float = 50.0   # m_visibilitySharpness
    probe_updates_per_frame: int = 2048  # m_probeUpdatesPerFrame
    compute_probe_offsets: bool = True   # m_computeProbeOffsets
    apply_probe_offsets: bool = True     # m_applyProbeOffsets
    use_scene_ambient: bool = True       # m_useSceneAmbient
    injected_ambient_lx: float = 100.0   # m_injectedAmbientLx
    max_rays_per_probe: int = abi.ARK_DDGI_MAX_RAYS_PER_PROBE        # DDGINode.h:22
    max_probe_updates: int = abi.ARK_DDGI_REFERENCE_MAX_PROBE_UPDATES  # DDGINode.h:23
    clear_overflow_mode: int = abi.ARK_DDGI_CLEAR_OVERFLOW_INF
    # context options beyond the reference node's (ArkDdgiDesc): the sun's shadow-ray
    # structure, serial frames (no frames in flight), host threads of the BVH builds
    sun_bvh: int = abi.ARK_DDGI_SUN_BVH_AUTO
    serial_frames: bool = False
    background_rebuild: bool = True
    # ARK_DDGI_FLAG_GPU_REBUILD (experimental): the world BVHs' background rebuild on the
    # device (an LBVH), one host rebuild once the motion stops; background_rebuild=False wins
    gpu_rebuild: bool = False
    # ARK_DDGI_FLAG_GPU_REBUILD_SUN (experimental): the light-space sun BVH's background build
    # on the device too (after a sun-direction change and after refits), one host rebuild once
    # no refit has come since; independent of gpu_rebuild
    gpu_rebuild_sun: bool = False
    # ARK_DDGI_FLAG_GPU_REBUILD_SAH (experimental): the device builds that gpu_rebuild and
    # gpu_rebuild_sun enable rebuild every subtree of at most 256 triangles by a sweep SAH
    # before the 8-wide collapse; alone it does nothing
    gpu_rebuild_sah: bool = False
    # ARK_DDGI_FLAG_GPU_REBUILD_PLAN (experimental): the device builds that run that SAH pass
    # split down to single triangles and collapse by the SAH-optimal plan (the host build's)
    # where they otherwise open members greedily; without the pass it does nothing
    gpu_rebuild_plan: bool = False
    # the sun's cover map (on by default; False: ARK_DDGI_FLAG_NO_SUN_COVER_MAP, every sun
    # shadow ray is traced - same results)
    sun_cover_map: bool = True
    # the sun-only shading schedule (on by default; False: ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE,
    # the shadow-ray generator runs as for every other scene - same results)
    fused_sun_shade: bool = True
    # the probe rays' hit candidates (on by default; False: ARK_DDGI_FLAG_NO_RAY_SEEDS, no
    # per-probe direction -> last-hit cache, every ray enters the BVH with tmax = zFar - same
    # results)
    ray_seeds: bool = True
    build_threads: int = 0


@dataclass
class AppState:
    """arkose/rendering/AppState.h:5-29"""
    frame_index: int = 0
    delta_time: float = 1.0 / 60.0

    def is_first_frame(self) -> bool:
        return self.frame_index == 0


class VertexUpdate:
    """One range of the scene's vertex pools for DDGIContext.update_geometry, starting at
    the absolute vertex `first_vertex`. positions: n x 3 float32, vertices: n x 9 float32
    (or the scene's vertex dtype: tex_coord 2, normal 3, tangent 4), either None to keep the
    pool's. numpy arrays are host sources. torch device tensors are device sources
    (ARK_DDGI_VERTICES_DEVICE: both must then be device tensors) and positions then need
    `bounds` = (lo xyz, hi xyz); the object keeps the arrays alive."""

    def __init__(self, first_vertex: int, positions=None, vertices=None, bounds=None):
        self.first_vertex = int(first_vertex)
        self.flags = 0
        self._keep = []
        self._ptr = [None, None]
        count = None
        for k, (a, width) in enumerate(((positions, 3), (vertices, 9))):
            if a is None:
                continue
            if not hasattr(a, "is_cuda"):  # an ndarray, or a list / tuple of rows
                a = np.asarray(a, dtype=None if isinstance(a, np.ndarray) else np.float32)
            device = not isinstance(a, np.ndarray) and a.is_cuda
            if device:  # a torch device tensor
                a = a.contiguous()
                if str(a.dtype) != "torch.float32":
                    raise TypeError("VertexUpdate: float32 tensors")
                floats, ptr = a.numel(), a.data_ptr()
            else:
                a = np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.numpy())
                if a.dtype != np.float32:
                    a = a.view(np.float32) if a.dtype.itemsize == 4 * width else a.astype(np.float32)
                floats, ptr = a.size, a.ctypes.data
            n = floats // width
            if floats != n * width:
                raise ValueError("VertexUpdate: %d floats per vertex" % width)
            if count is not None and (n != count or device != bool(self.flags)):
                raise ValueError("VertexUpdate: positions and vertices differ in count or in host / device")
            count = n
            self.flags = abi.ARK_DDGI_VERTICES_DEVICE if device else 0
            self._keep.append(a)
            self._ptr[k] = ptr
        self.vertex_count = count or 0
        self.bounds = None if bounds is None else [float(v) for v in np.asarray(bounds, dtype=np.float32).reshape(6)]

    def to_abi(self) -> abi.ArkDdgiVertexUpdate:
        u = abi.ArkDdgiVertexUpdate()
        u.struct_size = C.sizeof(abi.ArkDdgiVertexUpdate)
        u.first_vertex = self.first_vertex
        u.vertex_count = self.vertex_count
        u.flags = self.flags
        u.positions = self._ptr[0]
        u.vertices = self._ptr[1]
        if self.bounds is not None:
            u.bounds[:] = self.bounds
        return u


class Skin:
    """A skin for DDGIContext.register_skin: a range of the scene's vertex pools starting at
    `first_vertex` with its bind pose. positions n x 3 and vertices n x 9 float32 (or the
    scene's vertex dtype); joint_indices n x 4 uint32 with joint_weights n x 4 float32, or
    both None: morph-only; morph_targets K x n x 9 float32 (position, normal, tangent
    deltas), or None. The object keeps the arrays alive."""

    def __init__(self, first_vertex: int, positions, vertices, joint_indices=None, joint_weights=None, joint_count: int = 0, morph_targets=None):
        f32 = lambda a, w: np.ascontiguousarray(np.asarray(a).view(np.float32) if np.asarray(a).dtype.itemsize == 4 * w and np.asarray(a).dtype != np.float32  # noqa: E731
                                                 else np.asarray(a, dtype=np.float32)).reshape(-1, w)
        self.first_vertex = int(first_vertex)
        self.positions = f32(positions, 3)
        self.vertices = f32(vertices, 9)
        n = self.positions.shape[0]
        if self.vertices.shape[0] != n:
            raise ValueError("Skin: positions and vertices differ in count")
        self.vertex_count = n
        self.skinning = None
        self.joint_count = 0
        if (joint_indices is None) != (joint_weights is None):
            raise ValueError("Skin: joint_indices and joint_weights go together")
        if joint_indices is not None:
            sk = np.zeros(n, dtype=np.dtype([("joint_indices", np.uint32, 4), ("joint_weights", np.float32, 4)]))
            sk["joint_indices"] = np.asarray(joint_indices, dtype=np.uint32).reshape(n, 4)
            sk["joint_weights"] = np.asarray(joint_weights, dtype=np.float32).reshape(n, 4)
            self.skinning = sk
            self.joint_count = int(joint_count)
        self.morph_targets = None
        self.morph_target_count = 0
        if morph_targets is not None and np.asarray(morph_targets).size:
            m = np.ascontiguousarray(np.asarray(morph_targets, dtype=np.float32)).reshape(-1, n, 9)
            self.morph_targets = m
            self.morph_target_count = m.shape[0]

    def to_abi(self) -> abi.ArkDdgiSkinDesc:
        d = abi.ArkDdgiSkinDesc()
        d.struct_size = C.sizeof(abi.ArkDdgiSkinDesc)
        d.first_vertex = self.first_vertex
        d.vertex_count = self.vertex_count
        d.joint_count = self.joint_count
        d.morph_target_count = self.morph_target_count
        d.positions = self.positions.ctypes.data
        d.vertices = self.vertices.ctypes.data
        d.skinning = self.skinning.ctypes.data if self.skinning is not None else None
        d.morph_targets = self.morph_targets.ctypes.data if self.morph_targets is not None else None
        return d


class SkinPose:
    """One skin's pose for DDGIContext.skin_geometry: `skin` the handle register_skin
    returned, joint_matrices joint_count x 4 x 4 float32 with each matrix column-major (the
    reference's appliedJointMatrices: element [j, c, r] is row r of column c; from row-major
    numpy matrices M pass M.transpose(0, 2, 1)), or None for a morph-only skin;
    morph_weights K float32, or None."""

    def __init__(self, skin: int, joint_matrices=None, morph_weights=None):
        self.skin = int(skin)
        self.joint_matrices = None if joint_matrices is None else np.ascontiguousarray(np.asarray(joint_matrices, dtype=np.float32)).reshape(-1, 16)
        self.morph_weights = None if morph_weights is None else np.ascontiguousarray(np.asarray(morph_weights, dtype=np.float32)).reshape(-1)

    def to_abi(self) -> abi.ArkDdgiSkinPose:
        p = abi.ArkDdgiSkinPose()
        p.struct_size = C.sizeof(abi.ArkDdgiSkinPose)
        p.skin = self.skin
        p.joint_matrices = self.joint_matrices.ctypes.data if self.joint_matrices is not None else None
        p.morph_weights = self.morph_weights.ctypes.data if self.morph_weights is not None and self.morph_weights.size else None
        return p


def skin_host(skin: Skin, pose: SkinPose, prev_positions=None, lib=None):
    """ark_ddgi_debug_skin_host: the skinning pass restated on the host (no GPU). Returns
    (positions n x 3, vertices n x 9, velocities n x 3, bounds 6); raises ArkDdgiError for a
    skin or a pose that registration or skin_geometry would refuse."""
    lib = lib or abi.load_library()
    n = skin.vertex_count
    d, p = skin.to_abi(), pose.to_abi()
    prev = None if prev_positions is None else np.ascontiguousarray(np.asarray(prev_positions, dtype=np.float32)).reshape(n, 3)
    pos, vert, vel, bounds = np.zeros((n, 3), np.float32), np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32), np.zeros(6, np.float32)
    rc = lib.ark_ddgi_debug_skin_host(C.byref(d), C.byref(p), prev.ctypes.data if prev is not None else None, pos.ctypes.data, vert.ctypes.data, vel.ctypes.data,
                                      bounds.ctypes.data)
    if rc != 0:
        raise abi.ArkDdgiError(rc, "ark_ddgi_debug_skin_host")
    return pos, vert, vel, bounds


def skin_device_parity(skin: Skin, pose: SkinPose, prev_positions=None, dst_first_vertex: int = 0, device: int = 0, lib=None) -> dict:
    """ark_ddgi_debug_skin_device_parity: k_skin_vertices against the host restatement by bits."""
    lib = lib or abi.load_library()
    d, p = skin.to_abi(), pose.to_abi()
    prev = None if prev_positions is None else np.ascontiguousarray(np.asarray(prev_positions, dtype=np.float32)).reshape(skin.vertex_count, 3)
    out = (C.c_uint64 * 5)()
    rc = lib.ark_ddgi_debug_skin_device_parity(int(device), C.byref(d), C.byref(p), prev.ctypes.data if prev is not None else None, int(dst_first_vertex), out)
    if rc != 0:
        raise abi.ArkDdgiError(rc, "ark_ddgi_debug_skin_device_parity")
    return dict(zip(("positions", "vertices", "velocities", "outside", "kernel_ns"), (int(v) for v in out)))


def _check(lib, ctx, rc, what):
    if rc != 0:
        msg = lib.ark_ddgi_last_error(ctx)
        raise abi.ArkDdgiError(rc, f"{what}: {msg.decode() if msg else ''}")


def desc_for(grid: ProbeGrid, z_far: float, config: DDGIConfig, device: int = 0, shard_rank: int = 0,
             shard_count: int = 1) -> abi.ArkDdgiDesc:
    """The ArkDdgiDesc of a context (host only; the oracle takes it too)."""
    d = abi.ArkDdgiDesc()
    d.struct_size = C.sizeof(abi.ArkDdgiDesc)
    for k in range(3):
        d.grid_dims[k] = int(grid.grid_dimensions[k])
        d.probe_spacing[k] = float(grid.probe_spacing[k])
        d.offset_to_first[k] = float(grid.offset_to_first[k])
    d.z_far = float(z_far)
    d.max_rays_per_probe = int(config.max_rays_per_probe)
    d.max_probe_updates = int(config.max_probe_updates)
    d.device = int(device)
    d.clear_overflow_mode = int(config.clear_overflow_mode)
    d.shard_rank = int(shard_rank)
    d.shard_count = int(shard_count)
    d.sun_bvh = int(config.sun_bvh)
    d.flags = (abi.ARK_DDGI_FLAG_SERIAL_FRAMES if config.serial_frames else 0) | (0 if config.background_rebuild else abi.ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD)
    d.flags |= abi.ARK_DDGI_FLAG_GPU_REBUILD if config.gpu_rebuild else 0
    d.flags |= abi.ARK_DDGI_FLAG_GPU_REBUILD_SUN if config.gpu_rebuild_sun else 0
    d.flags |= abi.ARK_DDGI_FLAG_GPU_REBUILD_SAH if config.gpu_rebuild_sah else 0
    d.flags |= abi.ARK_DDGI_FLAG_GPU_REBUILD_PLAN if config.gpu_rebuild_plan else 0
    d.flags |= 0 if config.sun_cover_map else abi.ARK_DDGI_FLAG_NO_SUN_COVER_MAP
    d.flags |= 0 if config.fused_sun_shade else abi.ARK_DDGI_FLAG_NO_FUSED_SUN_SHADE
    d.flags |= 0 if config.ray_seeds else abi.ARK_DDGI_FLAG_NO_RAY_SEEDS
    d.build_threads = int(config.build_threads)
    return d


class DDGIContext:
    """Owns one ark_ddgi context (device memory of one DDGI node on one GPU)."""

    def __init__(self, grid: ProbeGrid, z_far: float, config: DDGIConfig | None = None, device: int = 0,
                 shard_rank: int = 0, shard_count: int = 1):
        self.lib = abi.load_library()
        self.grid = grid
        self.config = config or DDGIConfig()
        d = desc_for(grid, z_far, self.config, device, shard_rank, shard_count)
        self.desc = d
        h = C.c_void_p()
        rc = self.lib.ark_ddgi_create(C.byref(d), C.byref(h))
        if rc != 0:
            raise abi.ArkDdgiError(rc, "ark_ddgi_create")
        self.h = h
        self._scene = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.ark_ddgi_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def check(self, rc, what):
        _check(self.lib, self.h, rc, what)

    def last_error(self) -> str:
        """ark_ddgi_last_error: the message of the last error (or of a failed background rebuild)."""
        m = self.lib.ark_ddgi_last_error(self.h)
        return m.decode() if m else ""

    def set_scene(self, scene: SceneData):
        s = scene.to_abi()
        self.check(self.lib.ark_ddgi_set_scene(self.h, C.byref(s)), "ark_ddgi_set_scene")
        self._scene = scene

    def set_lights(self, sun=None, spots=()):
        """ark_ddgi_set_lights: the per-frame light set (GpuScene.cpp:790-858). sun =
        (colour, direction) with the colour pre-exposed (colour x intensity x
        lightPreExposure, :811) or None; spots = SpotLights, colours pre-exposed (:844)."""
        from .scene import lights_abi

        L, keep = lights_abi(sun, spots)
        self.check(self.lib.ark_ddgi_set_lights(self.h, C.byref(L)), "ark_ddgi_set_lights")
        del keep

    def set_instances(self, instances: np.ndarray):
        """ark_ddgi_set_instances: the per-frame TLAS instance update (GpuScene.cpp:872-1009),
        a device refit. `instances` = the scene's INSTANCE_DTYPE array with new transforms."""
        a = np.ascontiguousarray(instances)
        self.check(self.lib.ark_ddgi_set_instances(self.h, C.c_void_p(a.ctypes.data), int(a.size)), "ark_ddgi_set_instances")

    def set_instances_async(self, instances: np.ndarray, stream: int | None):
        """ark_ddgi_set_instances_async: the same refit enqueued on `stream` (no host wait)."""
        a = np.ascontiguousarray(instances)
        self.check(self.lib.ark_ddgi_set_instances_async(self.h, C.c_void_p(a.ctypes.data), int(a.size), C.c_void_p(stream) if stream else None),
                   "ark_ddgi_set_instances_async")

    def _geometry_args(self, updates, instances):
        ups = list(updates)
        arr = (abi.ArkDdgiVertexUpdate * max(1, len(ups)))(*[u.to_abi() for u in ups])
        inst = None if instances is None else np.ascontiguousarray(instances)
        return ups, arr, inst

    def update_geometry(self, updates, instances: np.ndarray | None = None):
        """ark_ddgi_update_geometry: deforming meshes (GpuScene.cpp:629-711, :934-992). `updates`
        = VertexUpdates, ranges of the scene's vertex pools with new contents; `instances` =
        the scene's INSTANCE_DTYPE array with new transforms, or None to keep them. One refit."""
        ups, arr, inst = self._geometry_args(updates, instances)
        self.check(self.lib.ark_ddgi_update_geometry(self.h, arr, len(ups), C.c_void_p(inst.ctypes.data) if inst is not None else None,
                                                     int(inst.size) if inst is not None else 0), "ark_ddgi_update_geometry")

    def update_geometry_async(self, updates, instances: np.ndarray | None = None, stream: int | None = None):
        """ark_ddgi_update_geometry_async: the same enqueued on `stream` (no host wait). Device
        sources must stay untouched until the stream has passed the call's work."""
        ups, arr, inst = self._geometry_args(updates, instances)
        self.check(self.lib.ark_ddgi_update_geometry_async(self.h, arr, len(ups), C.c_void_p(inst.ctypes.data) if inst is not None else None,
                                                           int(inst.size) if inst is not None else 0, C.c_void_p(stream) if stream else None),
                   "ark_ddgi_update_geometry_async")

    def geometry_update_stats(self) -> tuple:
        """ark_ddgi_get_geometry_update_stats: (update_geometry calls, vertices written,
        device-source positions dropped as non-finite, device-source positions clamped)."""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.ark_ddgi_get_geometry_update_stats(self.h, out), "ark_ddgi_get_geometry_update_stats")
        return tuple(int(v) for v in out)

    def register_skin(self, skin: "Skin") -> int:
        """ark_ddgi_register_skin: the skin's arrays copied to the device; returns its handle.
        Valid after set_scene; a new set_scene drops every skin."""
        d = skin.to_abi()
        h = C.c_uint32()
        self.check(self.lib.ark_ddgi_register_skin(self.h, C.byref(d), C.byref(h)), "ark_ddgi_register_skin")
        return int(h.value)

    def unregister_skin(self, skin: int):
        self.check(self.lib.ark_ddgi_unregister_skin(self.h, int(skin)), "ark_ddgi_unregister_skin")

    def _skin_args(self, poses, instances):
        ps = list(poses)
        arr = (abi.ArkDdgiSkinPose * max(1, len(ps)))(*[p.to_abi() for p in ps])
        inst = None if instances is None else np.ascontiguousarray(instances)
        return ps, arr, inst

    def skin_geometry(self, poses, instances: np.ndarray | None = None):
        """ark_ddgi_skin_geometry: every pose's skin computed on the device (skinning.comp) and
        written over its range of the pools, with optional new transforms: one refit."""
        ps, arr, inst = self._skin_args(poses, instances)
        self.check(self.lib.ark_ddgi_skin_geometry(self.h, arr, len(ps), C.c_void_p(inst.ctypes.data) if inst is not None else None,
                                                   int(inst.size) if inst is not None else 0), "ark_ddgi_skin_geometry")

    def skin_geometry_async(self, poses, instances: np.ndarray | None = None, stream: int | None = None):
        """ark_ddgi_skin_geometry_async: the same enqueued on `stream` (no host wait)."""
        ps, arr, inst = self._skin_args(poses, instances)
        self.check(self.lib.ark_ddgi_skin_geometry_async(self.h, arr, len(ps), C.c_void_p(inst.ctypes.data) if inst is not None else None,
                                                         int(inst.size) if inst is not None else 0, C.c_void_p(stream) if stream else None),
                   "ark_ddgi_skin_geometry_async")

    def skin_views(self, skin: int) -> abi.ArkDdgiSkinViews:
        """ark_ddgi_get_skin_views: device pointers to the skin's latest positions, vertices and velocities."""
        v = abi.ArkDdgiSkinViews()
        self.check(self.lib.ark_ddgi_get_skin_views(self.h, int(skin), C.byref(v)), "ark_ddgi_get_skin_views")
        return v

    def skin_stats(self) -> dict:
        """ark_ddgi_get_skin_stats."""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.ark_ddgi_get_skin_stats(self.h, out), "ark_ddgi_get_skin_stats")
        return dict(zip(("calls", "vertices", "rejected", "skins"), (int(v) for v in out)))

    def geometry_update_info(self) -> dict:
        """ark_ddgi_debug_geometry_update_info: what update_geometry allocated for the scene
        (all 0 for a scene that never called it)."""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.ark_ddgi_debug_geometry_update_info(self.h, out), "ark_ddgi_debug_geometry_update_info")
        return dict(zip(("map_allocations", "map_fills", "device_bytes", "position_updates"), (int(v) for v in out)))

    def share_scene(self, src: "DDGIContext"):
        """ark_ddgi_share_scene: use src's device scene and BVH (same GPU), no copy."""
        self.check(self.lib.ark_ddgi_share_scene(self.h, src.h), "ark_ddgi_share_scene")
        self._scene = src._scene

    def mark_external_write(self):
        """ark_ddgi_mark_external_write: offsets / atlases were written through the
        device views on the next update's stream; that update then runs after it."""
        self.check(self.lib.ark_ddgi_mark_external_write(self.h), "ark_ddgi_mark_external_write")

    def update(self, params: abi.ArkDdgiFrameParams, stream: int | None = None):
        self.check(self.lib.ark_ddgi_update(self.h, C.byref(params), C.c_void_p(stream) if stream else None), "ark_ddgi_update")

    def debug_probe_update(self, params: abi.ArkDdgiFrameParams, hits=None, stream: int | None = None):
        """ark_ddgi_debug_probe_update: the probe update's launches alone (slot table, offsets,
        blend and borders) over the surfels the context holds (write(ARK_DDGI_SURFELS) plants
        them). `hits`: [window probes, rays_per_probe] records with fields t (float32) and tri
        (uint32, 0xffffffff a miss) in slot order, required when params.update_offsets."""
        a = None
        if hits is not None:
            a = np.zeros(np.asarray(hits).shape, np.dtype([("t", np.float32), ("tri", np.uint32)]))
            a["t"], a["tri"] = hits["t"], hits["tri"]
            a = np.ascontiguousarray(a)
        self.check(self.lib.ark_ddgi_debug_probe_update(self.h, C.byref(params), C.c_void_p(a.ctypes.data) if a is not None else None,
                                                        C.c_void_p(stream) if stream else None), "ark_ddgi_debug_probe_update")

    def debug_shade(self, params: abi.ArkDdgiFrameParams, hits, stream: int | None = None) -> int:
        """ark_ddgi_debug_shade: hit shading alone (slot table, shadow rays, k_shade in the
        update's schedule) over planted hits: [window probes * rays_per_probe] records with
        fields instance (0xffffffff a miss), primitive, u, v, t in slot order. Returns the
        return code: 0, or ARK_DDGI_E_INVALID_ARGUMENT for a refused record (nothing launched)."""
        a = np.zeros(np.asarray(hits).size, SHADE_HIT_DTYPE)
        for k in SHADE_HIT_DTYPE.names:
            a[k] = np.asarray(hits)[k].reshape(-1)
        rc = self.lib.ark_ddgi_debug_shade(self.h, C.byref(params), C.c_void_p(a.ctypes.data), C.c_void_p(stream) if stream else None)
        if rc != abi.ARK_DDGI_E_INVALID_ARGUMENT:
            self.check(rc, "ark_ddgi_debug_shade")
        return rc

    def world_records(self) -> np.ndarray:
        """ark_ddgi_debug_world_records: the front copy's triangle records in leaf order,
        uint32 [records, 12] (word 9 the instance, word 10 the primitive; 0xffffffff: a hole)."""
        n = C.c_uint64()
        self.check(self.lib.ark_ddgi_debug_world_records(self.h, None, 0, C.byref(n)), "ark_ddgi_debug_world_records")
        out = np.zeros((int(n.value), 12), np.uint32)
        self.check(self.lib.ark_ddgi_debug_world_records(self.h, C.c_void_p(out.ctypes.data), int(n.value), C.byref(n)), "ark_ddgi_debug_world_records")
        return out

    def update_overlapped(self, params: abi.ArkDdgiFrameParams, stream: int | None, shade_wait_event: int | None,
                          done_event: int | None):
        """ark_ddgi_update_overlapped: raw hipStream_t / hipEvent_t handles (ints)."""
        v = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        self.check(self.lib.ark_ddgi_update_overlapped(self.h, C.byref(params), v(stream), v(shade_wait_event), v(done_event)),
                   "ark_ddgi_update_overlapped")

    def update_exchanged(self, params: abi.ArkDdgiFrameParams, stream: int | None):
        """ark_ddgi_update_exchanged: shading waits (device-side) for the last exchange_end."""
        self.check(self.lib.ark_ddgi_update_exchanged(self.h, C.byref(params), C.c_void_p(stream) if stream else None),
                   "ark_ddgi_update_exchanged")

    def exchange_begin(self, comm_stream: int | None):
        """ark_ddgi_exchange_begin: comm_stream waits (device-side) for the last update."""
        self.check(self.lib.ark_ddgi_exchange_begin(self.h, C.c_void_p(comm_stream) if comm_stream else None), "ark_ddgi_exchange_begin")

    def exchange_end(self, comm_stream: int | None):
        """ark_ddgi_exchange_end: the exchange enqueued on comm_stream so far completes the frame."""
        self.check(self.lib.ark_ddgi_exchange_end(self.h, C.c_void_p(comm_stream) if comm_stream else None), "ark_ddgi_exchange_end")

    def window_exchange_info(self) -> abi.ArkDdgiWindowExchange:
        """ark_ddgi_window_exchange_info: the packet layout of the last update's window."""
        w = abi.ArkDdgiWindowExchange()
        self.check(self.lib.ark_ddgi_window_exchange_info(self.h, C.byref(w)), "ark_ddgi_window_exchange_info")
        return w

    def pack_window(self, dst_ptr: int, nbytes: int, comm_stream: int | None):
        """ark_ddgi_pack_window: this rank's updated tiles -> dst (bytes_per_rank) on comm_stream."""
        self.check(self.lib.ark_ddgi_pack_window(self.h, C.c_void_p(dst_ptr), nbytes, C.c_void_p(comm_stream) if comm_stream else None),
                   "ark_ddgi_pack_window")

    def unpack_window(self, src_ptr: int, nbytes: int, comm_stream: int | None):
        """ark_ddgi_unpack_window: every rank's packets (world x bytes_per_rank) -> the other slabs' tiles."""
        self.check(self.lib.ark_ddgi_unpack_window(self.h, C.c_void_p(src_ptr), nbytes, C.c_void_p(comm_stream) if comm_stream else None),
                   "ark_ddgi_unpack_window")

    def synchronize(self):
        self.check(self.lib.ark_ddgi_synchronize(self.h), "ark_ddgi_synchronize")

    def set_sequencing(self, device_sequence_words: bool, timeout_ms: int = 0):
        """ark_ddgi_set_sequencing: device sequence words (True) or events between the
        context's streams, and the bound of each wait (0 = keep)."""
        self.check(self.lib.ark_ddgi_set_sequencing(self.h, int(device_sequence_words), int(timeout_ms)), "ark_ddgi_set_sequencing")

    def sequencing(self) -> dict:
        """ark_ddgi_get_sequencing: {device_sequence_words, timeout_ms, timeouts}."""
        w, t, n = C.c_int(), C.c_uint32(), C.c_uint32()
        self.check(self.lib.ark_ddgi_get_sequencing(self.h, C.byref(w), C.byref(t), C.byref(n)), "ark_ddgi_get_sequencing")
        return {"device_sequence_words": bool(w.value), "timeout_ms": int(t.value), "timeouts": int(n.value)}

    def size(self, which: int) -> int:
        n = C.c_uint64()
        self.check(self.lib.ark_ddgi_resource_size(self.h, which, C.byref(n)), "ark_ddgi_resource_size")
        return int(n.value)

    def read(self, which: int) -> np.ndarray:
        n = self.size(which)
        dt = {abi.ARK_DDGI_PROBE_OFFSETS: np.float32, abi.ARK_DDGI_DEBUG_HITS: np.float32, abi.ARK_DDGI_DEBUG_SHADOW_BITS: np.uint32}.get(which, np.uint16)
        out = np.empty(n // np.dtype(dt).itemsize, dtype=dt)
        self.check(self.lib.ark_ddgi_read(self.h, which, out.ctypes.data, n), "ark_ddgi_read")
        return out

    def write(self, which: int, data: np.ndarray):
        data = np.ascontiguousarray(data)
        self.check(self.lib.ark_ddgi_write(self.h, which, data.ctypes.data, data.nbytes), "ark_ddgi_write")

    def save_state(self) -> bytes:
        """ark_ddgi_save_state: the DDGI history (atlases + offsets) as one blob."""
        n = C.c_uint64()
        self.check(self.lib.ark_ddgi_state_size(self.h, C.byref(n)), "ark_ddgi_state_size")
        buf = (C.c_uint8 * n.value)()
        self.check(self.lib.ark_ddgi_save_state(self.h, buf, n.value), "ark_ddgi_save_state")
        return bytes(buf)

    def load_state(self, blob: bytes):
        """ark_ddgi_load_state: restores a blob of a context with the same grid / zFar / shard."""
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        self.check(self.lib.ark_ddgi_load_state(self.h, buf, len(blob)), "ark_ddgi_load_state")

    def next_probe_index(self) -> int:
        """ark_ddgi_get_next_probe_index: the rolling window's next first probe."""
        v = C.c_uint32()
        self.check(self.lib.ark_ddgi_get_next_probe_index(self.h, C.byref(v)), "ark_ddgi_get_next_probe_index")
        return int(v.value)

    def device_views(self) -> abi.ArkDdgiDeviceViews:
        v = abi.ArkDdgiDeviceViews()
        self.check(self.lib.ark_ddgi_get_device_views(self.h, C.byref(v)), "ark_ddgi_get_device_views")
        return v

    def reset_history(self):
        self.check(self.lib.ark_ddgi_reset_history(self.h), "ark_ddgi_reset_history")

    def set_counting(self, on: bool):
        self.check(self.lib.ark_ddgi_set_counting(self.h, int(on)), "ark_ddgi_set_counting")

    def counters(self) -> abi.ArkDdgiCounters:
        c = abi.ArkDdgiCounters()
        self.check(self.lib.ark_ddgi_get_counters(self.h, C.byref(c)), "ark_ddgi_get_counters")
        return c

    def set_timing(self, on: bool):
        self.check(self.lib.ark_ddgi_set_timing(self.h, int(on)), "ark_ddgi_set_timing")

    def last_timings(self):
        out = (C.c_float * 5)()
        self.check(self.lib.ark_ddgi_get_last_timings(self.h, out, 5), "ark_ddgi_get_last_timings")
        return list(out)

    def bake_ao(self, instance_index: int, width: int, height: int, sample_count: int, bent_normals: bool,
                stream: int | None = None):
        """ark_ddgi_bake_ao: AO / bent-normal bake of one instance's mesh segment."""
        d = abi.ArkBakeAoDesc()
        d.struct_size = C.sizeof(abi.ArkBakeAoDesc)
        d.instance_index, d.width, d.height, d.sample_count = int(instance_index), int(width), int(height), int(sample_count)
        d.bent_normals = int(bool(bent_normals))
        self.check(self.lib.ark_ddgi_bake_ao(self.h, C.byref(d), C.c_void_p(stream) if stream else None), "ark_ddgi_bake_ao")
        self._bake = (int(width), int(height), bool(bent_normals))

    def bake_read(self, which: int) -> np.ndarray:
        w, h, bent = self._bake
        shape, dt = {abi.ARK_BAKE_TRIANGLE_INDEX: ((h, w), np.uint32), abi.ARK_BAKE_BARYCENTRICS: ((h, w, 4), np.uint16),
                     abi.ARK_BAKE_OUTPUT: ((h, w, 4 if bent else 1), np.uint8)}[which]
        out = np.empty(shape, dt)
        self.check(self.lib.ark_ddgi_bake_read(self.h, which, out.ctypes.data, out.nbytes), "ark_ddgi_bake_read")
        return out

    def lighting_compose(self, width: int, height: int, flags: int, camera: dict, planes: dict, out_ptr: int,
                         stream: int | None = None):
        """ark_ddgi_lighting_compose. `planes` maps ArkComposeDesc plane names to DEVICE
        pointers (ints; absent = NULL); `camera` holds the three column-major 4x4
        matrices (CameraState, shared/CameraState.h); `out_ptr` is the RGBA16F output."""
        d = abi.ArkComposeDesc()
        d.struct_size = C.sizeof(abi.ArkComposeDesc)
        d.width, d.height, d.flags = int(width), int(height), int(flags)
        for k in ("view_from_pixel", "view_from_world", "world_from_view"):
            m = np.ascontiguousarray(camera[k], np.float32).reshape(16)
            getattr(d, k)[:] = [float(v) for v in m]
        for name, _, _ in abi.COMPOSE_PLANES:
            ptr = planes.get(name)
            setattr(d, name, int(ptr) if ptr else None)
        d.out = int(out_ptr)
        self.check(self.lib.ark_ddgi_lighting_compose(self.h, C.byref(d), C.c_void_p(stream) if stream else None),
                   "ark_ddgi_lighting_compose")

    def rt_local_shadows(self, desc: abi.ArkRtShadowsDesc, stream: int | None = None):
        """ark_ddgi_rt_local_shadows: `desc` holds device pointers (include/ark_ddgi.h; rt_shadows_desc)."""
        desc.struct_size = C.sizeof(abi.ArkRtShadowsDesc)
        self.check(self.lib.ark_ddgi_rt_local_shadows(self.h, C.byref(desc), C.c_void_p(stream) if stream else None), "ark_ddgi_rt_local_shadows")

    def path_trace(self, desc: abi.ArkPathTracerDesc, stream: int | None = None):
        """ark_ddgi_path_trace: `desc` holds device pointers (include/ark_ddgi.h; path_tracer_desc)."""
        desc.struct_size = C.sizeof(abi.ArkPathTracerDesc)
        self.check(self.lib.ark_ddgi_path_trace(self.h, C.byref(desc), C.c_void_p(stream) if stream else None), "ark_ddgi_path_trace")

    def rt_reflections_denoise(self, desc: abi.ArkReflDenoiseDesc, stream: int | None = None):
        """ark_ddgi_rt_reflections_denoise: `desc` holds device pointers (include/ark_ddgi.h; refl_denoise_desc)."""
        desc.struct_size = C.sizeof(abi.ArkReflDenoiseDesc)
        self.check(self.lib.ark_ddgi_rt_reflections_denoise(self.h, C.byref(desc), C.c_void_p(stream) if stream else None), "ark_ddgi_rt_reflections_denoise")

    def rt_reflections(self, desc: abi.ArkReflectionsDesc, stream: int | None = None):
        """ark_ddgi_rt_reflections: `desc` holds device pointers (include/ark_ddgi.h)."""
        desc.struct_size = C.sizeof(abi.ArkReflectionsDesc)
        self.check(self.lib.ark_ddgi_rt_reflections(self.h, C.byref(desc), C.c_void_p(stream) if stream else None), "ark_ddgi_rt_reflections")

    def probe_debug(self, visualisation: int, distance_scale: float, count: int, probes_ptr: int, dirs_ptr: int, out_ptr: int,
                    stream: int | None = None):
        """ark_ddgi_probe_debug on device arrays (uint32 probe indices, float3 directions,
        RGBA16F out)."""
        d = abi.ArkProbeDebugDesc()
        d.struct_size = C.sizeof(abi.ArkProbeDebugDesc)
        d.visualisation, d.distance_scale, d.count = int(visualisation), float(distance_scale), int(count)
        d.probe_indices, d.directions, d.out = int(probes_ptr), int(dirs_ptr), int(out_ptr)
        self.check(self.lib.ark_ddgi_probe_debug(self.h, C.byref(d), C.c_void_p(stream) if stream else None), "ark_ddgi_probe_debug")

    def bvh_stats(self) -> abi.ArkDdgiBvhStats:
        s = abi.ArkDdgiBvhStats()
        self.check(self.lib.ark_ddgi_get_bvh_stats(self.h, C.byref(s)), "ark_ddgi_get_bvh_stats")
        return s

    def scene_digest(self) -> tuple:
        """ark_ddgi_debug_scene_digest: digests of the world BVH nodes, world records, sun
        BVH nodes, sun records the kernels read now (tests of the refit)."""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.ark_ddgi_debug_scene_digest(self.h, out), "ark_ddgi_debug_scene_digest")
        return tuple(int(v) for v in out)

    def world_bvh_check(self) -> dict:
        """ark_ddgi_debug_world_bvh_check: the world BVH8s the kernels read now, downloaded
        and checked on the host (violations 0 = valid)."""
        out = (C.c_uint64 * 8)()
        rc = self.lib.ark_ddgi_debug_world_bvh_check(self.h, out)
        if rc < 0:
            self.check(rc, "ark_ddgi_debug_world_bvh_check")
        return dict(zip(_BVH_CHECK_KEYS, (int(v) for v in out)))

    def sun_cover_counts(self, host_restatement: bool = True) -> dict:
        """ark_ddgi_debug_sun_cover_counts after a counting update: the sun's rays resolved
        by the cover map and listed, on the device and (host_restatement) by the host."""
        out = (C.c_uint64 * 12)()
        fn = self.lib.ark_ddgi_debug_sun_cover_counts if host_restatement else self.lib.ark_ddgi_debug_sun_cover_counts_device
        self.check(fn(self.h, out), "ark_ddgi_debug_sun_cover_counts")
        keys = ("occluded", "lit", "listed", "in_use", "nx", "ny", "bytes", "build_us", "host_occluded", "host_lit", "host_listed", "map_diff")
        return dict(zip(keys, (int(v) for v in out)))

    def shade_schedule(self) -> dict:
        """ark_ddgi_debug_shade_schedule: whether the last update ran the sun-only shading
        schedule, and the rays it deferred to its second shading pass."""
        out = (C.c_uint64 * 2)()
        self.check(self.lib.ark_ddgi_debug_shade_schedule(self.h, out), "ark_ddgi_debug_shade_schedule")
        return {"sun_only": bool(out[0]), "deferred": int(out[1])}

    def seed_info(self) -> dict:
        """ark_ddgi_debug_seed_info: the probe rays' hit-candidate cache - whether the context
        keeps one, its texels per side, the scene's opaque record range, and the probe rays of
        the last counting update whose candidate was hit."""
        out = (C.c_uint64 * 5)()
        self.check(self.lib.ark_ddgi_debug_seed_info(self.h, out), "ark_ddgi_debug_seed_info")
        return {"enabled": bool(out[0]), "texels": int(out[1]), "first": int(out[2]), "end": int(out[3]), "candidate_hits": int(out[4])}

    def seed_fill(self, mode: int, value: int = 0):
        """ark_ddgi_debug_seed_fill: overwrites the cache - mode 0 the sentinel, 1 random opaque
        records from the seed `value`, 2 the record `value` everywhere (refused when it is not
        a record of the opaque class)."""
        self.check(self.lib.ark_ddgi_debug_seed_fill(self.h, int(mode), int(value)), "ark_ddgi_debug_seed_fill")

    def set_sun_only_small_windows(self, on: bool):
        """ark_ddgi_debug_set_sun_only_small_windows: pipelined half-occupancy windows, which keep
        the generator schedule by default, run the sun-only schedule too (tests)."""
        self.check(self.lib.ark_ddgi_debug_set_sun_only_small_windows(self.h, int(on)), "ark_ddgi_debug_set_sun_only_small_windows")

    def sun_bvh_installed_check(self) -> dict:
        """ark_ddgi_debug_sun_bvh_installed_check: the light-space sun BVH8 the kernels read
        now, downloaded and checked on the host (violations 0 = valid); "installed": False
        (and every count 0) when there is none."""
        out = (C.c_uint64 * 8)()
        rc = self.lib.ark_ddgi_debug_sun_bvh_installed_check(self.h, out)
        if rc < 0:
            self.check(rc, "ark_ddgi_debug_sun_bvh_installed_check")
        r = dict(zip(_BVH_CHECK_KEYS, (int(v) for v in out)))
        r["installed"] = r["nodes"] > 0
        return r

    def refit_reach(self) -> dict:
        """ark_ddgi_debug_refit_reach: the nodes of the world BVHs and of the light-space
        sun BVH, and how many of each the last refit reached (all 0 before the first)."""
        out = (C.c_uint64 * 4)()
        self.check(self.lib.ark_ddgi_debug_refit_reach(self.h, out), "ark_ddgi_debug_refit_reach")
        return dict(zip(("world_nodes", "world_reached", "sun_nodes", "sun_reached"), (int(v) for v in out)))


    def refit_inflation(self) -> tuple:
        """ark_ddgi_debug_refit_inflation: the last refit's box inflation steps (world, light space)."""
        out = (C.c_float * 2)()
        self.check(self.lib.ark_ddgi_debug_refit_inflation(self.h, out), "ark_ddgi_debug_refit_inflation")
        return float(out[0]), float(out[1])


_BVH_CHECK_KEYS = ("nodes", "leaf_children", "max_depth", "violations", "records", "records_with_holes", "record_digest", "installed_builder")


def sun_lbvh_check(triangles, sun_dir, origins, tmax: float = 1e30, w_bits: int | None = None, sah: bool | None = None, plan: bool | None = None) -> tuple:
    """ark_ddgi_debug_sun_lbvh_check: the device build of the sun's light-space BVH8 run
    serially on the host over world triangles (n x 9 floats), then a sun shadow ray from
    each origin (m x 3 floats) through it against brute force. Returns (rc, dict): rays,
    occluded_brute, occluded_bvh, mismatches, node_visits, triangle_tests, nodes,
    max_stack_depth, violations, inflation_differs, cost_lbvh, cost_host (any-hit steps per
    ray) and the tree's leaf_children, depth, records_with_holes, w_bits. w_bits: the
    key's Morton bits given to w (None: the default). sah not None:
    ark_ddgi_debug_sun_lbvh_check_sah, with (True) or without the SAH pass of
    gpu_rebuild_sah, and `treelets`. plan not None: ark_ddgi_debug_sun_lbvh_check_plan, with
    (True) or without the collapse plan of gpu_rebuild_plan on top of sah (None: True), and
    `plan_root_cost` (an fp32 word), `small_internal`. No GPU."""
    lib = abi.load_library()
    tris = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    sd = np.ascontiguousarray(sun_dir, dtype=np.float32).reshape(3)
    org = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    keys = ("rays", "occluded_brute", "occluded_bvh", "mismatches", "node_visits", "triangle_tests", "nodes", "max_stack_depth", "violations",
            "inflation_differs", "cost_lbvh", "cost_host", "leaf_children", "depth", "records_with_holes", "w_bits")
    if plan is not None:
        out = (C.c_uint64 * 19)()
        rc = lib.ark_ddgi_debug_sun_lbvh_check_plan(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], float(tmax),
                                                    -1 if w_bits is None else int(w_bits), 0 if sah is False else 1, 1 if plan else 0, out)
        keys = keys + ("treelets", "plan_root_cost", "small_internal")
    elif sah is None:
        out = (C.c_uint64 * 16)()
        rc = lib.ark_ddgi_debug_sun_lbvh_check_opts(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], float(tmax),
                                                    -1 if w_bits is None else int(w_bits), out)
    else:
        out = (C.c_uint64 * 17)()
        rc = lib.ark_ddgi_debug_sun_lbvh_check_sah(tris.ctypes.data, tris.shape[0], sd.ctypes.data, org.ctypes.data, org.shape[0], float(tmax),
                                                   -1 if w_bits is None else int(w_bits), 1 if sah else 0, out)
        keys = keys + ("treelets",)
    r = dict(zip(keys, (int(v) for v in out)))
    r["cost_lbvh"] /= 1e6
    r["cost_host"] /= 1e6
    return rc, r


def lbvh_check(triangles, criterion: int | None = None, sah: bool | None = None, plan: bool | None = None) -> tuple:
    """ark_ddgi_debug_lbvh_check: the device LBVH build's logic run serially on the host
    over world triangles (n x 9 floats). Returns (rc, out[8]) with out as
    ark_ddgi_debug_bvh8_check: nodes, leaf children, max depth, violations, triangles,
    radix-tree nodes, internal children, BVH8 SAH cost x 1e6. sah not None:
    ark_ddgi_debug_lbvh_check_sah, with (True) or without the SAH pass of gpu_rebuild_sah,
    out[9] with the treelets last. plan not None: ark_ddgi_debug_lbvh_check_plan, with (True)
    or without the collapse plan of gpu_rebuild_plan on top of sah (None: True), out[11] with
    the plan's root cost word and the internal members of at most 3 triangles last. No GPU."""
    lib = abi.load_library()
    tris = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    out = (C.c_uint64 * (11 if plan is not None else 8 if sah is None else 9))()
    if plan is not None:
        rc = lib.ark_ddgi_debug_lbvh_check_plan(tris.ctypes.data, tris.shape[0], 1 if criterion is None else int(criterion), 0 if sah is False else 1,
                                                1 if plan else 0, out)
    elif sah is not None:
        rc = lib.ark_ddgi_debug_lbvh_check_sah(tris.ctypes.data, tris.shape[0], 1 if criterion is None else int(criterion), 1 if sah else 0, out)
    elif criterion is None:
        rc = lib.ark_ddgi_debug_lbvh_check(tris.ctypes.data, tris.shape[0], out)
    else:
        rc = lib.ark_ddgi_debug_lbvh_check_opts(tris.ctypes.data, tris.shape[0], int(criterion), out)
    return rc, [int(v) for v in out]


def triangle_records(triangles, instances, holes=None) -> np.ndarray:
    """The 48-byte triangle records of world triangles (n x 9 floats) as a snapshot of the
    world BVHs holds them (make_gpu_triangle: v0, e1 = v1 - v0, e2 = v2 - v0 in fp32,
    instance, primitive = the triangle's index, flip 0): n x 12 uint32 words. holes: a
    boolean mask of records replaced by hole records (all zero, instance 0xffffffff)."""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    rec = np.zeros((t.shape[0], 12), np.uint32)
    f = rec.view(np.float32)
    f[:, 0:3] = t[:, 0:3]
    f[:, 3:6] = t[:, 3:6] - t[:, 0:3]
    f[:, 6:9] = t[:, 6:9] - t[:, 0:3]
    rec[:, 9] = np.asarray(instances, np.uint32)
    rec[:, 10] = np.arange(t.shape[0], dtype=np.uint32)
    if holes is not None:
        h = np.asarray(holes, bool)
        rec[h] = 0
        rec[h, 9] = 0xFFFFFFFF
    return rec


_LBVH_PARITY_KEYS = ("prims", "nodes", "records_with_holes", "depth", "why", "compaction", "wave_order", "header_counts", "header_box", "max_abs",
                     "inflation", "keys", "sorted_indices", "splits", "shape", "node_header", "grid", "planes", "children", "records", "perm", "holes",
                     "level_order", "padding", "first_device_node", "first_host_node", "hip_error", "pairs", "host_nodes")
LBVH_PARITY_MISMATCHES = _LBVH_PARITY_KEYS[5:24]
# ark_ddgi_debug_lbvh_device_parity_sah's further words
_LBVH_PARITY_SAH_KEYS = _LBVH_PARITY_KEYS + ("treelets", "treelet_list", "sorted_after_sah", "node_boxes", "prim_boxes")
LBVH_PARITY_SAH_MISMATCHES = LBVH_PARITY_MISMATCHES + _LBVH_PARITY_SAH_KEYS[30:34]
# ark_ddgi_debug_lbvh_device_parity_plan's further words
_LBVH_PARITY_PLAN_KEYS = _LBVH_PARITY_SAH_KEYS + ("upper_nodes", "plan_picks", "plan_costs", "upper_boxes", "upper_list", "upper_rounds")
LBVH_PARITY_PLAN_MISMATCHES = LBVH_PARITY_SAH_MISMATCHES + _LBVH_PARITY_PLAN_KEYS[35:39]
LBVH_WHY = ("", "no records", "no triangles", "record of an unknown instance", "too deep", "node scratch", "4 GiB", "other")


def lbvh_device_parity(records, class_of, sun_dir=None, w_bits: int | None = None, device: int = 0, sah: bool | None = None, plan: bool | None = None) -> tuple:
    """ark_ddgi_debug_lbvh_device_parity: the device LBVH build (the world's, or with sun_dir
    the sun's light-space one) run once over triangle records (triangle_records) and compared
    bit for bit, stage by stage, with its host restatement. class_of: instance -> hit-mask
    class. Returns (rc, dict): prims, nodes, records_with_holes, depth, why (LBVH_WHY's text)
    and one mismatch count per stage (LBVH_PARITY_MISMATCHES). sah not None:
    ark_ddgi_debug_lbvh_device_parity_sah, both builds with (True) or without the SAH pass
    of gpu_rebuild_sah; also treelets and LBVH_PARITY_SAH_MISMATCHES' counts. plan not None:
    ark_ddgi_debug_lbvh_device_parity_plan, both builds with (True) or without the collapse plan
    of gpu_rebuild_plan on top of sah (None: True); also upper_nodes and
    LBVH_PARITY_PLAN_MISMATCHES' counts. Needs a GPU."""
    lib = abi.load_library()
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 12)
    cls = np.ascontiguousarray(class_of, dtype=np.int32).reshape(-1)
    sd = None if sun_dir is None else np.ascontiguousarray(sun_dir, dtype=np.float32).reshape(3)
    if plan is not None:
        out = (C.c_uint64 * 48)()
        rc = lib.ark_ddgi_debug_lbvh_device_parity_plan(int(device), rec.ctypes.data, rec.shape[0], cls.ctypes.data, cls.shape[0],
                                                        None if sd is None else sd.ctypes.data, -1 if w_bits is None else int(w_bits),
                                                        0 if sah is False else 1, 1 if plan else 0, out)
        r = dict(zip(_LBVH_PARITY_PLAN_KEYS, (int(v) for v in out)))
    elif sah is None:
        out = (C.c_uint64 * 32)()
        rc = lib.ark_ddgi_debug_lbvh_device_parity(int(device), rec.ctypes.data, rec.shape[0], cls.ctypes.data, cls.shape[0],
                                                   None if sd is None else sd.ctypes.data, -1 if w_bits is None else int(w_bits), out)
        r = dict(zip(_LBVH_PARITY_KEYS, (int(v) for v in out)))
    else:
        out = (C.c_uint64 * 40)()
        rc = lib.ark_ddgi_debug_lbvh_device_parity_sah(int(device), rec.ctypes.data, rec.shape[0], cls.ctypes.data, cls.shape[0],
                                                       None if sd is None else sd.ctypes.data, -1 if w_bits is None else int(w_bits), 1 if sah else 0, out)
        r = dict(zip(_LBVH_PARITY_SAH_KEYS, (int(v) for v in out)))
    r["why"] = LBVH_WHY[r["why"]] if rc >= 0 else "error"
    return rc, r


def bvh8_compare_selftest(triangles, sun_dir=None, seed: int = 1) -> tuple:
    """ark_ddgi_debug_bvh8_compare_selftest: the canonical tree comparison of
    lbvh_device_parity tried on a renumbered twin of the host LBVH tree of the triangles and on
    six mutations of it. Returns (rc, dict). No GPU."""
    lib = abi.load_library()
    tris = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    sd = None if sun_dir is None else np.ascontiguousarray(sun_dir, dtype=np.float32).reshape(3)
    out = (C.c_uint64 * 16)()
    rc = lib.ark_ddgi_debug_bvh8_compare_selftest(tris.ctypes.data, tris.shape[0], None if sd is None else sd.ctypes.data, int(seed), out)
    keys = ("nodes", "renumbered", "twin_differences", "pairs", "twin_violations", "plane_looser", "grid_coarser", "children_exchanged",
            "leaf_members_exchanged", "records_exchanged", "perm_altered", "full_check_plane_looser", "full_check_grid_coarser")
    return rc, dict(zip(keys, (int(v) for v in out)))


def frame_params(config: DDGIConfig, grid: ProbeGrid, app: AppState, first_probe_index: int,
                 light_pre_exposure: float = 1.0, ambient_illuminance: float = 0.0,
                 environment_brightness: float = 1.0) -> abi.ArkDdgiFrameParams:
    """Push-constant values of the execute lambda (DDGINode.cpp:132-259)."""
    p = abi.ArkDdgiFrameParams()
    p.struct_size = C.sizeof(abi.ArkDdgiFrameParams)
    p.frame_index = int(app.frame_index) & 0xFFFFFFFF
    p.first_probe_index = int(first_probe_index)
    p.probe_updates = min(int(config.probe_updates_per_frame), grid.probe_count())
    p.rays_per_probe = int(config.rays_per_probe)
    p.hysteresis_irradiance = 0.0 if app.is_first_frame() else config.hysteresis_irradiance
    p.hysteresis_visibility = 0.0 if app.is_first_frame() else config.hysteresis_visibility
    p.visibility_sharpness = config.visibility_sharpness
    ambient_lx = ambient_illuminance if config.use_scene_ambient else config.injected_ambient_lx
    p.ambient_amount = float(np.float32(ambient_lx) * np.float32(light_pre_exposure))
    p.environment_multiplier = float(np.float32(environment_brightness) * np.float32(light_pre_exposure))
    p.delta_time = float(app.delta_time)
    p.update_offsets = int(config.compute_probe_offsets and config.apply_probe_offsets)
    return p


class DDGINode:
    """Python mirror of DDGINode (name "DDGI") driving a DDGIContext."""

    def __init__(self, config: DDGIConfig | None = None):
        self.config = config or DDGIConfig()
        self.probe_update_idx = 0  # m_probeUpdateIdx (DDGINode.h:32)
        self.ctx: DDGIContext | None = None
        self.grid: ProbeGrid | None = None
        self.exposure = dict(light_pre_exposure=1.0, ambient_illuminance=0.0, environment_brightness=1.0)

    def name(self) -> str:
        return "DDGI"

    def construct(self, scene: SceneData, grid: ProbeGrid | None, z_far: float, device: int = 0,
                  shard_rank: int = 0, shard_count: int = 1, **exposure) -> bool:
        """DDGINode::construct (DDGINode.cpp:37-130). Returns False (no-op node)
        when there is no probe grid, like NullExecuteCallback (:39-42)."""
        if grid is None or grid.probe_count() == 0:
            return False
        self.grid = grid
        self.ctx = DDGIContext(grid, z_far, self.config, device, shard_rank, shard_count)
        self.ctx.set_scene(scene)
        self.exposure.update(exposure)
        return True

    def next_params(self, app: AppState) -> abi.ArkDdgiFrameParams:
        return frame_params(self.config, self.grid, app, self.probe_update_idx, **self.exposure)

    def execute_overlapped(self, app: AppState, stream: int | None, shade_wait_event: int | None,
                           done_event: int | None) -> abi.ArkDdgiFrameParams:
        """execute() through ark_ddgi_update_overlapped (Z-slab ranks, see collective.py)."""
        if self.ctx is None:
            return None
        p = self.next_params(app)
        self.ctx.update_overlapped(p, stream, shade_wait_event, done_event)
        self.probe_update_idx = (self.probe_update_idx + p.probe_updates) % self.grid.probe_count()
        return p

    def execute_exchanged(self, app: AppState, stream: int | None) -> abi.ArkDdgiFrameParams:
        """execute() through ark_ddgi_update_exchanged (Z-slab ranks, see collective.py)."""
        if self.ctx is None:
            return None
        p = self.next_params(app)
        self.ctx.update_exchanged(p, stream)
        self.probe_update_idx = (self.probe_update_idx + p.probe_updates) % self.grid.probe_count()
        return p

    def execute(self, app: AppState, stream: int | None = None) -> abi.ArkDdgiFrameParams:
        if self.ctx is None:
            return None
        p = self.next_params(app)
        self.ctx.update(p, stream)
        self.probe_update_idx = (self.probe_update_idx + p.probe_updates) % self.grid.probe_count()
        return p

    def save_state(self) -> bytes:
        """The node's DDGI history: atlases, offsets and the window position."""
        return self.ctx.save_state()

    def load_state(self, blob: bytes):
        """Restores save_state()'s blob and resumes the rolling window where it was."""
        self.ctx.load_state(blob)
        self.probe_update_idx = self.ctx.next_probe_index()


class BakeAmbientOcclusionNode:
    """Python mirror of BakeAmbientOcclusionNode (name "Bake ambient occlusion",
    arkose/rendering/baking/BakeAmbientOcclusionNode.{h,cpp}): bakes the mesh segment
    of one instance; the output format selects AO (R8Uint) or bent normals (RGBA8)
    (BakeAmbientOcclusionNode.cpp:20-31). The scene/BVH come from a DDGIContext."""

    R8UINT = "R8Uint"
    RGBA8 = "RGBA8"

    def __init__(self, instance_index: int, sample_count: int = 500):
        assert sample_count > 0  # BakeAmbientOcclusionNode.cpp:12
        self.instance_index = instance_index
        self.sample_count = sample_count

    def name(self) -> str:
        return "Bake ambient occlusion"

    def execute(self, ctx: DDGIContext, width: int, height: int, output_format: str, stream: int | None = None) -> np.ndarray:
        if output_format not in (self.R8UINT, self.RGBA8):
            raise ValueError("BakeAmbientOcclusionNode: unknown AO texture format - only R8Uint & RGBA8 (bent normals)")
        bent = output_format == self.RGBA8
        ctx.bake_ao(self.instance_index, width, height, self.sample_count, bent, stream)
        return ctx.bake_read(abi.ARK_BAKE_OUTPUT)



def _tensor_stream(tensor, stream: int | None) -> int:
    """Stream for a consumer node whose planes are torch tensors: the caller's, else
    torch's current stream on the tensor's device (handle 0 = the null stream), so the
    launch is ordered after torch's producers of the planes and before its readers,
    as the reference records the node into the frame's one command list. The C-ABI
    orders it after the context's earlier operations on any stream."""
    if stream:
        return stream
    import torch

    return torch.cuda.current_stream(tensor.device).cuda_stream


def _check_plane(node: str, name: str, t, h: int, w: int, channels: int | None, dtypes):
    """A device plane the kernel indexes as [h][w](channels): contiguous, that shape,
    one of `dtypes` (torch dtypes)."""
    shape = (h, w) if channels is None else (h, w, channels)
    if not t.is_cuda or not t.is_contiguous() or tuple(int(v) for v in t.shape) != shape or t.dtype not in dtypes:
        raise ValueError(f"{node}: plane {name} must be a contiguous {list(shape)} device tensor of {'/'.join(str(d) for d in dtypes)}, "
                         f"got {list(t.shape)} {t.dtype}")


class LightingComposeNode:
    """Python mirror of LightingComposeNode (name "Lighting compose",
    arkose/rendering/lighting/LightingComposeNode.{h,cpp}) for the WITH_DDGI
    configuration: the node's toggles (LightingComposeNode.h:16-25 defaults, GUI at
    LightingComposeNode.cpp:9-44) become ArkComposeDesc flags; the G-buffer planes are
    device tensors (torch) in the formats GpuScene.cpp:326-360 creates."""

    def __init__(self):
        self.include_direct_light = True
        self.include_skin_diffuse_light = True
        self.include_glossy_gi = True
        self.include_diffuse_gi = True
        self.with_baked_occlusion = True
        self.use_bent_normal_direction = True
        self.with_bent_normal_occlusion = True
        self.with_screen_space_occlusion = True
        self.include_material_color = True  # GpuScene::shouldIncludeMaterialColor

    def name(self) -> str:
        return "Lighting compose"

    def flags(self, has_screen_space_occlusion: bool) -> int:
        f = 0
        f |= abi.ARK_COMPOSE_DIRECT_LIGHT if self.include_direct_light else 0
        f |= abi.ARK_COMPOSE_SKIN_DIFFUSE_LIGHT if self.include_skin_diffuse_light else 0
        f |= abi.ARK_COMPOSE_DIFFUSE_GI if self.include_diffuse_gi else 0
        f |= abi.ARK_COMPOSE_BAKED_OCCLUSION if self.with_baked_occlusion else 0
        f |= abi.ARK_COMPOSE_USE_BENT_NORMAL if self.use_bent_normal_direction else 0
        f |= abi.ARK_COMPOSE_BENT_NORMAL_OCCLUSION if self.with_bent_normal_occlusion else 0
        # no AmbientOcclusion texture: the option is forced off (LightingComposeNode.cpp:56-60)
        f |= abi.ARK_COMPOSE_SCREEN_SPACE_OCCLUSION if (self.with_screen_space_occlusion and has_screen_space_occlusion) else 0
        f |= abi.ARK_COMPOSE_GLOSSY_GI if self.include_glossy_gi else 0
        f |= abi.ARK_COMPOSE_MATERIAL_COLOR if self.include_material_color else 0
        return f

    def execute(self, ctx: DDGIContext, camera: dict, gbuffer: dict, out, stream: int | None = None):
        """gbuffer: plane name -> contiguous device tensor [H, W(, C)] (missing = NULL,
        read as 0 like the node's black stand-ins); out: uint16/float16 device tensor
        [H, W, 4] (SceneColorWithGI, RGBA16F)."""
        h, w = int(out.shape[0]), int(out.shape[1])
        planes = {}
        for name, _, _ in abi.COMPOSE_PLANES:
            t = gbuffer.get(name)
            if t is not None:
                if not t.is_contiguous() or int(t.shape[0]) != h or int(t.shape[1]) != w:
                    raise ValueError(f"LightingComposeNode: plane {name} must be a contiguous [{h}, {w}, ...] tensor")
                planes[name] = t.data_ptr()
        s = _tensor_stream(out, stream)
        ctx.lighting_compose(w, h, self.flags("screen_space_occlusion" in gbuffer), camera, planes, out.data_ptr(), s)


class DDGIProbeDebug:
    """Python mirror of DDGIProbeDebug (name "DDGI probe debug",
    arkose/rendering/nodes/DDGIProbeDebug.{h,cpp}): the fragment stage of its probe
    spheres (probeDebug.frag) on (probe, normal) samples - `sphere_samples` gives the
    reference's 48x48 sphere vertices; rasterising them is the caller's."""

    def __init__(self):
        self.debug_visualisation = abi.ARK_PROBE_DEBUG_DISABLED  # m_debugVisualisation
        self.probe_scale = 0.1
        self.distance_scale = 0.01
        self.use_probe_offset = True

    def name(self) -> str:
        return "DDGI probe debug"

    @staticmethod
    def sphere_samples(rings: int = 48, sectors: int = 48) -> np.ndarray:
        """Unit-sphere vertex positions of createSphereRenderData (DDGIProbeDebug.cpp:75-98)."""
        r = np.arange(rings, dtype=np.float32)[:, None]
        s = np.arange(sectors, dtype=np.float32)[None, :]
        R, S = np.float32(1.0 / (rings - 1)), np.float32(1.0 / (sectors - 1))
        pi = np.float32(np.pi)
        y = np.sin(-(pi / 2) + pi * r * R) * np.ones_like(s)
        x = np.cos(2 * pi * s * S) * np.sin(pi * r * R)
        z = np.sin(2 * pi * s * S) * np.sin(pi * r * R)
        return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)

    def execute(self, ctx: DDGIContext, probes, dirs, out, stream: int | None = None):
        """probes: uint32/int32 device tensor [n]; dirs: float32 device tensor [n, 3];
        out: 16-bit device tensor [n, 4]. A no-op when the visualisation is disabled
        (DDGIProbeDebug.cpp:53-54)."""
        if self.debug_visualisation == abi.ARK_PROBE_DEBUG_DISABLED:
            return
        s = _tensor_stream(out, stream)
        ctx.probe_debug(self.debug_visualisation, self.distance_scale, int(probes.shape[0]), probes.data_ptr(), dirs.data_ptr(),
                        out.data_ptr(), s)


def reflections_desc(width: int, height: int, camera: dict, planes: dict, no_tracing_roughness: float = 0.6,
                     environment_multiplier: float = 1.0, ambient_amount: float = 0.0) -> abi.ArkReflectionsDesc:
    """ArkReflectionsDesc from a camera dict (world_from_view, view_from_projection:
    column-major 16 floats) and a plane dict of pointers (depth, material,
    normal_velocity, blue_noise, out_radiance, out_direction; missing = NULL) plus
    noise_width / noise_height. The default threshold is RTReflectionsNode's
    (RTReflectionsNode.h:20, m_noTracingRoughnessThreshold 0.6)."""
    d = abi.ArkReflectionsDesc()
    d.struct_size = C.sizeof(abi.ArkReflectionsDesc)
    d.width, d.height = int(width), int(height)
    d.no_tracing_roughness, d.environment_multiplier, d.ambient_amount = float(no_tracing_roughness), float(environment_multiplier), float(ambient_amount)
    for k in ("world_from_view", "view_from_projection"):
        getattr(d, k)[:] = [float(v) for v in np.asarray(camera[k], np.float32).reshape(16)]
    for k in ("depth", "material", "normal_velocity", "blue_noise", "out_radiance", "out_direction"):
        v = planes.get(k)
        setattr(d, k, int(v) if v else None)
    d.noise_width, d.noise_height = int(planes.get("noise_width", 0)), int(planes.get("noise_height", 0))
    return d


REFL_DENOISE_CAMERA_KEYS = ("world_from_view", "view_from_projection", "previous_frame_view_from_world", "previous_frame_projection_from_view")


def refl_denoise_desc(width: int, height: int, camera: dict, planes: dict, flags: int = 0, no_tracing_roughness: float = 0.6,
                      temporal_stability: float = 0.7) -> abi.ArkReflDenoiseDesc:
    """ArkReflDenoiseDesc from a camera dict (REFL_DENOISE_CAMERA_KEYS: column-major 16 floats;
    z_near, z_far) and a dict of plane addresses (abi.REFL_DENOISE_PLANES; missing = NULL):
    device addresses for DDGIContext.rt_reflections_denoise, host addresses for
    refl_denoise_host. The defaults are RTReflectionsNode's members (RTReflectionsNode.h:20, :25)."""
    d = abi.ArkReflDenoiseDesc()
    d.struct_size = C.sizeof(abi.ArkReflDenoiseDesc)
    d.width, d.height, d.flags = int(width), int(height), int(flags)
    d.no_tracing_roughness, d.temporal_stability = float(no_tracing_roughness), float(temporal_stability)
    for k in REFL_DENOISE_CAMERA_KEYS:
        getattr(d, k)[:] = [float(v) for v in np.asarray(camera[k], np.float32).reshape(16)]
    d.z_near, d.z_far = float(camera["z_near"]), float(camera["z_far"])
    for k, _, _, _ in abi.REFL_DENOISE_PLANES:
        v = planes.get(k)
        setattr(d, k, int(v) if v else None)
    return d


def refl_denoise_plane_shape(name: str, width: int, height: int):
    """(shape, numpy dtype) of one of abi.REFL_DENOISE_PLANES; 16-bit planes as uint16 words."""
    _, dtype, ch, per_tile = next(p for p in abi.REFL_DENOISE_PLANES if p[0] == name)
    h, w = ((height + 7) // 8, (width + 7) // 8) if per_tile else (height, width)
    return ((h, w) if ch == 1 else (h, w, ch)), {"float16": np.uint16, "float32": np.float32, "uint8": np.uint8}[dtype]


def refl_denoise_host(width: int, height: int, camera: dict, planes: dict, flags: int = 0, no_tracing_roughness: float = 0.6,
                      temporal_stability: float = 0.7):
    """ark_ddgi_debug_refl_denoise_host: the denoiser passes restated on the host, no GPU.
    planes: every one of abi.REFL_DENOISE_PLANES as a C-contiguous numpy array of
    refl_denoise_plane_shape (16-bit planes as uint16 or float16); the written ones are
    written in place, as the device entry writes the caller's planes."""
    lib = abi.load_library()
    addr = {}
    for k, _, _, _ in abi.REFL_DENOISE_PLANES:
        a = planes[k]
        shape, dtype = refl_denoise_plane_shape(k, width, height)
        if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"] or a.shape != shape or a.dtype.itemsize != np.dtype(dtype).itemsize:
            raise ValueError(f"refl_denoise_host: plane {k} must be a contiguous {list(shape)} array of {np.dtype(dtype)}")
        addr[k] = a.ctypes.data
    d = refl_denoise_desc(width, height, camera, addr, flags, no_tracing_roughness, temporal_stability)
    rc = lib.ark_ddgi_debug_refl_denoise_host(C.byref(d))
    if rc != 0:
        raise abi.ArkDdgiError(rc, "ark_ddgi_debug_refl_denoise_host: a descriptor ark_ddgi_rt_reflections_denoise refuses")
    return planes


class RTReflectionsNode:
    """Mirror of RTReflectionsNode (RTReflectionsNode.cpp:60-139): the raygen with WITH_DDGI on
    torch G-buffer planes, then the denoiser passes (historyCopy, reproject, prefilter,
    resolveTemporal, historyCopy) over planes the node owns, as the reference node owns its
    textures. Defaults are the node's members (RTReflectionsNode.h:19-25)."""

    def __init__(self):
        self.no_tracing_roughness_threshold = 0.6  # m_noTracingRoughnessThreshold (parameter2)
        self.mirror_roughness_threshold = 0.001    # m_mirrorRoughnessThreshold (parameter1): read by no code path of the raygen
        self.denoise_enabled = True                # m_denoiseEnabled
        self.temporal_stability = 0.7              # m_temporalStability
        self.denoise_planes = None                 # allocate_denoise_planes
        self.relative_first_frame = True           # appState.isRelativeFirstFrame(): set again by a resize

    def name(self) -> str:
        return "RT reflections"

    def allocate_denoise_planes(self, width: int, height: int, device) -> dict:
        """The denoiser's nine written planes for a resolution, zeroed (reproject leaves the
        non-glossy pixels of reprojected / variance / num_samples untouched and the later
        passes read them), and the relative-first-frame flag set: the next execute runs the
        initial historyCopy. 16-bit planes are float16 tensors."""
        import torch

        planes = {}
        for k, dtype, _, _ in abi.REFL_DENOISE_PLANES:
            if k in abi.REFL_DENOISE_INPUTS or k == "radiance":
                continue
            shape, _ = refl_denoise_plane_shape(k, width, height)
            planes[k] = torch.zeros(shape, dtype=getattr(torch, dtype), device=device)
        self.denoise_planes = planes
        self._denoise_extent = (int(width), int(height), torch.device(device))
        self.relative_first_frame = True
        return planes

    def execute(self, ctx: DDGIContext, camera: dict, gbuffer: dict, blue_noise, out_radiance, out_direction,
                environment_multiplier: float = 1.0, ambient_amount: float = 0.0, stream: int | None = None):
        """gbuffer: depth float32 [h, w], material uint8 [h, w, 4], normal_velocity
        16-bit [h, w, 4] (missing = NULL, read as 0); blue_noise float32 [hn, wn, 2]
        (one RG layer); out_radiance / out_direction 16-bit [h, w, 4].

        A camera that also carries the denoiser's CameraState fields
        (previous_frame_view_from_world, previous_frame_projection_from_view, z_near, z_far)
        runs the denoiser after the raygen and returns the DenoisedReflections plane
        (denoise_planes["resolved"]); its planes are allocated for out_radiance's resolution
        on first use and again after a resize, which is a relative first frame. With
        denoise_enabled off the raygen's radiance is copied to that plane
        (RTReflectionsNode.cpp:134-138). Without those fields only the raygen runs, as before
        the denoiser existed, and None is returned."""
        import torch

        h, w = int(out_radiance.shape[0]), int(out_radiance.shape[1])
        half = (torch.float16, torch.int16, torch.uint16) if hasattr(torch, "uint16") else (torch.float16, torch.int16)
        node = "RTReflectionsNode"
        _check_plane(node, "out_radiance", out_radiance, h, w, 4, half)
        _check_plane(node, "out_direction", out_direction, h, w, 4, half)
        spec = {"depth": (None, (torch.float32,)), "material": (4, (torch.uint8,)), "normal_velocity": (4, half)}
        for k, t in gbuffer.items():
            if k not in spec:
                raise ValueError(f"{node}: unknown plane {k}")
            if t is not None:
                _check_plane(node, k, t, h, w, spec[k][0], spec[k][1])
        planes = {k: (t.data_ptr() if t is not None else None) for k, t in gbuffer.items()}
        planes.update(out_radiance=out_radiance.data_ptr(), out_direction=out_direction.data_ptr())
        if blue_noise is not None:
            if (not blue_noise.is_cuda or not blue_noise.is_contiguous() or blue_noise.dim() != 3 or int(blue_noise.shape[2]) != 2
                    or blue_noise.dtype != torch.float32 or blue_noise.shape[0] == 0 or blue_noise.shape[1] == 0):
                raise ValueError(f"{node}: blue_noise must be a contiguous float32 [hn, wn, 2] device tensor, "
                                 f"got {list(blue_noise.shape)} {blue_noise.dtype}")
            planes.update(blue_noise=blue_noise.data_ptr(), noise_width=int(blue_noise.shape[1]), noise_height=int(blue_noise.shape[0]))
        d = reflections_desc(w, h, camera, planes, self.no_tracing_roughness_threshold, environment_multiplier, ambient_amount)
        s = _tensor_stream(out_radiance, stream)
        ctx.rt_reflections(d, s)
        if "previous_frame_view_from_world" not in camera:
            return None
        for k in ("depth", "material", "normal_velocity"):
            if gbuffer.get(k) is None:
                raise ValueError(f"{node}: the denoiser needs plane {k}")
        if self.denoise_planes is None or self._denoise_extent != (w, h, out_radiance.device):
            self.allocate_denoise_planes(w, h, out_radiance.device)
        addr = {k: t.data_ptr() for k, t in self.denoise_planes.items()}
        addr.update(radiance=out_radiance.data_ptr(), depth=gbuffer["depth"].data_ptr(), material=gbuffer["material"].data_ptr(),
                    normal_velocity=gbuffer["normal_velocity"].data_ptr())
        flags = (0 if self.denoise_enabled else abi.ARK_REFL_DENOISE_DISABLED) | (abi.ARK_REFL_DENOISE_FIRST_FRAME if self.relative_first_frame else 0)
        ctx.rt_reflections_denoise(refl_denoise_desc(w, h, camera, addr, flags, self.no_tracing_roughness_threshold, self.temporal_stability), s)
        if self.denoise_enabled:
            self.relative_first_frame = False  # (a disabled frame copies no history: the next enabled one is still a first frame)
        return self.denoise_planes["resolved"]



class RTShadowLight:
    """A ray-traced spot light as RTLocalShadowNode passes it (RTLocalShadowNode.cpp:60-75):
    the transform's position and forward(), the outer cone angle (the full angle SpotLight
    stores; the raygen gets cos(angle / 2), RTLocalShadowNode.cpp:77) and lightSourceRadius (SpotLight.h:45)."""

    def __init__(self, position, direction, outer_cone_angle: float, source_radius: float = 0.025):
        self.position = tuple(float(v) for v in position)
        self.direction = tuple(float(v) for v in direction)
        self.outer_cone_angle = float(outer_cone_angle)
        self.source_radius = float(source_radius)

    @property
    def outer_cone_angle_cos(self) -> float:
        return float(np.cos(np.float32(self.outer_cone_angle / 2.0), dtype=np.float32))


def rt_shadows_desc(width: int, height: int, camera: dict, depth, lights, masks, frame_index: int = 0) -> abi.ArkRtShadowsDesc:
    """ArkRtShadowsDesc from a camera dict (world_from_view, view_from_projection:
    column-major 16 floats), the depth plane's address, RTShadowLight objects and one mask
    address per light (device addresses for DDGIContext.rt_local_shadows, host addresses for
    rt_shadows_host). frame_index is what the raygen's frameIndex() returns. The lights array
    lives as long as the descriptor."""
    d = abi.ArkRtShadowsDesc()
    d.struct_size = C.sizeof(abi.ArkRtShadowsDesc)
    d.width, d.height, d.frame_index = int(width), int(height), int(frame_index) & 0xFFFFFFFF
    for k in ("world_from_view", "view_from_projection"):
        getattr(d, k)[:] = [float(v) for v in np.asarray(camera[k], np.float32).reshape(16)]
    d.depth = int(depth) if depth else None
    lights = list(lights)
    masks = list(masks)
    if len(masks) != len(lights):
        raise ValueError(f"rt_shadows_desc: {len(lights)} lights, {len(masks)} masks")
    arr = (abi.ArkRtShadowLight * max(1, len(lights)))()
    for a, l, m in zip(arr, lights, masks):
        a.position[:] = l.position
        a.direction[:] = l.direction
        a.outer_cone_angle_cos = l.outer_cone_angle_cos
        a.source_radius = l.source_radius
        a.out_mask = int(m) if m else None
    d._lights_keepalive = arr
    d.lights = C.cast(arr, C.POINTER(abi.ArkRtShadowLight)) if lights else None
    d.light_count = len(lights)
    return d


RT_SHADOW_COUNTS = ("sky", "culled", "lit", "occluded")


def _rt_shadows_host_desc(width, height, camera, depth, lights, frame_index):
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if depth.shape != (height, width):
        raise ValueError(f"rt_shadows_host: depth must be [{height}, {width}], got {list(depth.shape)}")
    lights = list(lights)
    masks = [np.full((height, width), 0xAA, np.uint8) for _ in lights]
    d = rt_shadows_desc(width, height, camera, depth.ctypes.data if depth.size else 1, lights, [m.ctypes.data if m.size else 1 + k for k, m in enumerate(masks)],
                        frame_index)
    return d, depth, masks


def _rt_shadow_counts(out, n):
    return [dict(zip(RT_SHADOW_COUNTS, (int(out[4 * l + k]) for k in range(4)))) for l in range(n)]


def rt_shadows_host(records, class_of, class_mask: int, width: int, height: int, camera: dict, depth, lights, frame_index: int = 0):
    """ark_ddgi_debug_rt_shadows_host: the shadow masks of ark_ddgi_rt_local_shadows restated on
    the host over triangle records (triangle_records) by brute force, no GPU. class_of:
    instance -> hit-mask class; bit c of class_mask: class c occludes (1: opaque only, the
    feature; 7: every class). depth: float32 [h, w] host array. Returns (masks, counts): one
    uint8 [h, w] array and one {sky, culled, lit, occluded} dict per light."""
    lib = abi.load_library()
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 12)
    cls = np.ascontiguousarray(class_of, dtype=np.int32).reshape(-1)
    d, depth, masks = _rt_shadows_host_desc(width, height, camera, depth, lights, frame_index)
    out = (C.c_uint64 * (4 * max(1, len(masks))))()
    rc = lib.ark_ddgi_debug_rt_shadows_host(rec.ctypes.data, rec.shape[0], cls.ctypes.data, cls.shape[0], int(class_mask), C.byref(d), out)
    if rc != 0:
        raise abi.ArkDdgiError(rc, "ark_ddgi_debug_rt_shadows_host: a descriptor ark_ddgi_rt_local_shadows refuses")
    return masks, _rt_shadow_counts(out, len(masks))


def rt_shadows_host_ctx(ctx: DDGIContext, class_mask: int, width: int, height: int, camera: dict, depth, lights, frame_index: int = 0):
    """ark_ddgi_debug_rt_shadows_host_ctx: rt_shadows_host over the records of the context's
    front copy (it follows refits and vertex updates). Synchronous; needs the context's GPU."""
    d, depth, masks = _rt_shadows_host_desc(width, height, camera, depth, lights, frame_index)
    out = (C.c_uint64 * (4 * max(1, len(masks))))()
    ctx.check(ctx.lib.ark_ddgi_debug_rt_shadows_host_ctx(ctx.h, int(class_mask), C.byref(d), out), "ark_ddgi_debug_rt_shadows_host_ctx")
    return masks, _rt_shadow_counts(out, len(masks))


class RTLocalShadowNode:
    """Mirror of RTLocalShadowNode (name "RT local shadows", RTLocalShadowNode.cpp:47-90):
    every ray-traced spot light's screen-size R8 shadow mask, all lights in one call. The
    raygen's frame parameter is frameIndex % 8 (RTLocalShadowNode.cpp:69)."""

    FRAME_PERIOD = 8

    def name(self) -> str:
        return "RT local shadows"

    def frame_parameter(self, frame_index: int) -> int:
        return int(frame_index) % self.FRAME_PERIOD

    def execute(self, ctx: DDGIContext, camera: dict, depth, lights, masks, frame_index: int, stream: int | None = None):
        """depth: float32 [h, w] device tensor; lights: RTShadowLight objects; masks: one uint8
        [h, w] device tensor per light, each written whole."""
        import torch

        node = "RTLocalShadowNode"
        h, w = int(depth.shape[0]), int(depth.shape[1])
        _check_plane(node, "depth", depth, h, w, None, (torch.float32,))
        lights, masks = list(lights), list(masks)
        if len(lights) != len(masks):
            raise ValueError(f"{node}: {len(lights)} lights, {len(masks)} masks")
        for k, m in enumerate(masks):
            _check_plane(node, f"mask {k}", m, h, w, None, (torch.uint8,))
        d = rt_shadows_desc(w, h, camera, depth.data_ptr(), lights, [m.data_ptr() for m in masks], self.frame_parameter(frame_index))
        ctx.rt_local_shadows(d, _tensor_stream(depth, stream))

    def execute_host(self, records, class_of, class_mask: int, camera: dict, depth, lights, frame_index: int):
        """The same frame through rt_shadows_host (no GPU): (masks, counts)."""
        depth = np.asarray(depth)
        return rt_shadows_host(records, class_of, class_mask, int(depth.shape[1]), int(depth.shape[0]), camera, depth, lights, self.frame_parameter(frame_index))


def path_tracer_desc(width: int, height: int, camera: dict, image, accumulation=None, flags: int = 0, frame_index: int = 0, accumulated_frames: int = 0,
                     environment_multiplier: float = 1.0, max_paths_per_batch: int = 0) -> abi.ArkPathTracerDesc:
    """ArkPathTracerDesc from a camera dict (world_from_view, view_from_projection: column-major
    16 floats; z_near, z_far) and the planes' addresses (device addresses for
    DDGIContext.path_trace, host addresses for path_tracer_host)."""
    d = abi.ArkPathTracerDesc()
    d.struct_size = C.sizeof(abi.ArkPathTracerDesc)
    d.width, d.height, d.flags = int(width), int(height), int(flags)
    d.frame_index, d.accumulated_frames, d.max_paths_per_batch = int(frame_index) & 0xFFFFFFFF, int(accumulated_frames), int(max_paths_per_batch)
    d.environment_multiplier, d.z_near, d.z_far = float(environment_multiplier), float(camera["z_near"]), float(camera["z_far"])
    for k in ("world_from_view", "view_from_projection"):
        getattr(d, k)[:] = [float(v) for v in np.asarray(camera[k], np.float32).reshape(16)]
    d.image = int(image) if image else None
    d.accumulation = int(accumulation) if accumulation else None
    return d


def _path_tracer_host(call, width, height, camera, flags, frame_index, accumulated_frames, environment_multiplier, accumulation, vertices):
    image = np.full((height, width, 4), 0x5555, np.uint16)
    acc = None
    if flags:
        acc = np.ascontiguousarray(accumulation, dtype=np.float32).copy() if accumulation is not None else np.zeros((height, width, 4), np.float32)
        if acc.shape != (height, width, 4):
            raise ValueError(f"path_tracer_host: accumulation must be [{height}, {width}, 4], got {list(acc.shape)}")
    d = path_tracer_desc(width, height, camera, image.ctypes.data if image.size else 8, acc.ctypes.data if acc is not None and acc.size else (16 if flags else None), flags,
                         frame_index, accumulated_frames, environment_multiplier)
    vtx = np.zeros((height, width, abi.PATH_TRACER_MAX_SEGMENTS), np.dtype(abi.PATH_TRACER_VERTEX)) if vertices else None
    out = (C.c_uint64 * len(abi.PATH_TRACER_COUNTS))()
    call(d, vtx.ctypes.data if vtx is not None and vtx.size else None, out)
    return image, acc, vtx, dict(zip(abi.PATH_TRACER_COUNTS, (int(v) for v in out)))


def path_tracer_host(scene: SceneData, width: int, height: int, camera: dict, flags: int = 0, frame_index: int = 0, accumulated_frames: int = 0,
                     environment_multiplier: float = 1.0, accumulation=None, vertices: bool = False):
    """ark_ddgi_debug_path_tracer_host: the frame of ark_ddgi_path_trace restated on the host
    over `scene`, no GPU. Returns (image uint16 [h, w, 4], accumulation float32 [h, w, 4] or
    None, vertices (a structured array [h, w, 16] of abi.PATH_TRACER_VERTEX) or None, counts)."""
    lib = abi.load_library()
    abi_scene = scene.to_abi()

    def call(d, vtx, out):
        rc = lib.ark_ddgi_debug_path_tracer_host(C.byref(abi_scene), C.byref(d), vtx, out)
        if rc != 0:
            raise abi.ArkDdgiError(rc, "ark_ddgi_debug_path_tracer_host: a scene or a descriptor the library refuses")

    return _path_tracer_host(call, width, height, camera, flags, frame_index, accumulated_frames, environment_multiplier, accumulation, vertices)


def path_tracer_host_ctx(ctx: DDGIContext, width: int, height: int, camera: dict, flags: int = 0, frame_index: int = 0, accumulated_frames: int = 0,
                         environment_multiplier: float = 1.0, accumulation=None, vertices: bool = False):
    """ark_ddgi_debug_path_tracer_host_ctx: path_tracer_host over the context's own scene,
    downloaded (it follows refits and set_lights). Synchronous; needs the context's GPU."""

    def call(d, vtx, out):
        ctx.check(ctx.lib.ark_ddgi_debug_path_tracer_host_ctx(ctx.h, C.byref(d), vtx, out), "ark_ddgi_debug_path_tracer_host_ctx")

    return _path_tracer_host(call, width, height, camera, flags, frame_index, accumulated_frames, environment_multiplier, accumulation, vertices)


def path_tracer_last_counts(ctx: DDGIContext) -> tuple:
    """ark_ddgi_debug_path_tracer_last_counts: (live paths per segment [16], shadow rays listed
    per segment [16]) of the last batch of the context's last path_trace call. Synchronous."""
    out = (C.c_uint32 * (2 * abi.PATH_TRACER_MAX_SEGMENTS))()
    ctx.check(ctx.lib.ark_ddgi_debug_path_tracer_last_counts(ctx.h, out), "ark_ddgi_debug_path_tracer_last_counts")
    v = [int(x) for x in out]
    return v[:abi.PATH_TRACER_MAX_SEGMENTS], v[abi.PATH_TRACER_MAX_SEGMENTS:]


class PathTracerNode:
    """Mirror of PathTracerNode (name "Path tracer", PathTracerNode.cpp:81-103): one path per
    pixel and frame into the RGBA16F image, accumulated into the caller's RGBA32F plane. The
    node holds the reference's state; the library holds none."""

    def __init__(self):
        self.should_accumulate = True           # m_shouldAccumulate
        self.current_accumulated_frames = 0     # m_currentAccumulatedFrames
        self.max_accumulated_frames = 1000      # m_maxAccumulatedFrames

    def name(self) -> str:
        return "Path tracer"

    def plan(self, is_relative_first_frame: bool, camera_changed: bool, pending_uploads: bool) -> int:
        """The frame's flags by PathTracerNode.cpp:83-84: ARK_PATH_TRACER_RESET,
        ARK_PATH_TRACER_ACCUMULATE, or -1 when nothing is traced (the maximum is reached)."""
        should_reset = (not self.should_accumulate) or is_relative_first_frame or camera_changed or pending_uploads
        should_accum = (not should_reset) and self.should_accumulate and self.current_accumulated_frames < self.max_accumulated_frames
        if should_accum:
            return abi.ARK_PATH_TRACER_ACCUMULATE
        return abi.ARK_PATH_TRACER_RESET if should_reset else -1

    def advance(self, flags: int):
        """The frame count after a frame planned as `flags` (PathTracerNode.cpp:98, :101)."""
        if flags == abi.ARK_PATH_TRACER_ACCUMULATE:
            self.current_accumulated_frames += 1
        elif flags == abi.ARK_PATH_TRACER_RESET:
            self.current_accumulated_frames = 1

    def execute(self, ctx: DDGIContext, app: AppState, camera: dict, image, accumulation, environment_multiplier: float = 1.0, camera_changed: bool = False,
                pending_uploads: bool = False, stream: int | None = None, max_paths_per_batch: int = 0):
        """image: float16 [h, w, 4] device tensor (pathTraceImage); accumulation: float32
        [h, w, 4] device tensor (PathTracerAccumulation). camera_changed and pending_uploads
        are the caller's (scene.camera().hasChangedSinceLastFrame(), scene.hasPendingUploads()).
        Returns the accumulation plane."""
        import torch

        node = "PathTracerNode"
        h, w = int(image.shape[0]), int(image.shape[1])
        _check_plane(node, "image", image, h, w, 4, (torch.float16,))
        _check_plane(node, "accumulation", accumulation, h, w, 4, (torch.float32,))
        flags = self.plan(app.is_first_frame(), camera_changed, pending_uploads)
        if flags >= 0:
            d = path_tracer_desc(w, h, camera, image.data_ptr(), accumulation.data_ptr(), flags, app.frame_index, self.current_accumulated_frames, environment_multiplier,
                                 max_paths_per_batch)
            ctx.path_trace(d, _tensor_stream(image, stream))
            self.advance(flags)
        return accumulation
