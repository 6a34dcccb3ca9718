"""The world BVH8s rebuilt on the device while instances move (ARK_DDGI_FLAG_GPU_REBUILD,
DDGIConfig.gpu_rebuild; csrc/ddgi_bvh_build.hip): an LBVH per hit-mask class over a device
snapshot of the refitted records, installed by the background-rebuild machinery. Hits do
not depend on the tree, so every frame stays bit-exact against the oracle across the
installs; ark_ddgi_debug_world_bvh_check downloads the installed BVHs and checks them on
the host. Once the motion stops one host rebuild replaces the LBVH (the settle rebuild).
"""
import time

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S
import oracle_lib as O
import scenes
from parity import RESOURCES, diff_report

pytestmark = pytest.mark.gpu

GRID = D.ProbeGrid((4, 4, 4), (1.0, 0.8, 1.0), (-1.5, 0.3, -1.5))
EXPOSURE = dict(light_pre_exposure=1.0, environment_brightness=1.0)
WAIT_S = 60  # wall-clock bound of every polling loop


def _cfg(R=32, K=64, **kw):
    return D.DDGIConfig(rays_per_probe=R, probe_updates_per_frame=K, max_rays_per_probe=R, max_probe_updates=K, **kw)


def _compare(ctx, orc, frame, what):
    for k, w in RESOURCES.items():
        r = diff_report(k, ctx.read(w), orc.read(w))
        assert r["mismatch"] == 0, f"frame {frame} ({what}): {r}"


def _moved(inst0, f):
    """One instance a frame, each further each time."""
    inst = inst0.copy()
    M = inst["object_to_world"].reshape(-1, 3, 4).copy()
    M[f % len(inst), :, 3] += np.float32(0.02 * (f + 1))
    inst["object_to_world"] = M.reshape(len(inst), 12)
    return inst


def _rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)


def _frame(ctx, cfg, grid, f, first, orc=None, what=""):
    p = D.frame_params(cfg, grid, D.AppState(f), first, **EXPOSURE)
    ctx.update(p)
    ctx.synchronize()
    if orc is not None:
        orc.update(p)
        _compare(ctx, orc, f, what)
    return (first + p.probe_updates) % grid.probe_count()


def test_structure_and_records():
    """All three hit-mask classes: the installed device build is a valid set of BVH8s over
    the same records, bit for bit those a refit alone leaves."""
    sc = scenes.features_scene()
    cfg = _cfg(gpu_rebuild=True)
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ref = D.DDGIContext(GRID, 100.0, _cfg(background_rebuild=False))
    try:
        ctx.set_scene(sc)
        before = ctx.world_bvh_check()
        assert before["violations"] == 0 and before["installed_builder"] == 0, before
        first, f, t0 = 0, 0, time.time()
        inst = sc.instances
        while ctx.bvh_stats().bvh_gpu_rebuilds < 1:
            inst = _moved(sc.instances, f)
            ctx.set_instances(inst)
            first = _frame(ctx, cfg, GRID, f, first)
            f += 1
            assert time.time() - t0 < WAIT_S, f"no device build installed within {WAIT_S} s: {ctx.last_error()}"
        st = ctx.bvh_stats()
        after = ctx.world_bvh_check()
        print(f"features scene: device build installed after {f} frames in {st.bvh_rebuild_ms:.1f} ms: {after}")
        assert after["violations"] == 0, (after, ctx.last_error())
        assert st.bvh_installed_builder == 1 and after["installed_builder"] == 1
        assert st.bvh_gpu_fallbacks == 0 and st.bvh_rebuild_failures == 0
        assert after["records"] == before["records"]
        # the records whichever builder placed them: a refit of set_scene's BVHs to the same transforms
        ref.set_scene(sc)
        ref.set_instances(inst)
        want = ref.world_bvh_check()
        assert want["violations"] == 0 and want["installed_builder"] == 0
        assert (after["records"], after["record_digest"]) == (want["records"], want["record_digest"])
    finally:
        ctx.close()
        ref.close()


def test_parity_across_installs():
    """test_continuous_motion_installs_rebuilds' motion with the device build: every frame
    bit-exact against the oracle before, across and after three installs."""
    import torch

    sc = S.soup(20_000, extent=7.0)
    grid = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
    cfg = _cfg(compute_probe_offsets=True, sun_bvh=abi.ARK_DDGI_SUN_BVH_LIGHT_SPACE, gpu_rebuild=True)
    ctx = D.DDGIContext(grid, 10000.0, cfg)
    ctx.set_scene(sc)
    assert ctx.bvh_stats().sun_node_count > 0
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    stream = torch.cuda.Stream()
    inst0 = sc.instances.copy()
    first, f, t0 = 0, 0, time.time()
    try:
        while True:
            inst = inst0.copy()
            M = inst["object_to_world"].reshape(-1, 3, 4).copy()
            M[f % len(inst), :, 3] += np.float32(0.02 * (f + 1))
            M[1, :, :3] = _rot_y(0.05 * f) @ M[1, :, :3]
            inst["object_to_world"] = M.reshape(len(inst), 12)
            ctx.set_instances_async(inst, stream.cuda_stream)
            orc.set_instances(inst)
            p = D.frame_params(cfg, grid, D.AppState(f), first, **EXPOSURE)
            ctx.update(p, stream.cuda_stream)
            orc.update(p)
            ctx.synchronize()
            _compare(ctx, orc, f, "continuous motion, device rebuilds")
            st = ctx.bvh_stats()
            first = (first + p.probe_updates) % grid.probe_count()
            f += 1
            if st.bvh_gpu_rebuilds >= 3:
                break
            assert time.time() - t0 < WAIT_S, f"{st.bvh_gpu_rebuilds} device builds installed within {WAIT_S} s: {ctx.last_error()}"
        print(f"continuous motion: {f} frames, {st.bvh_gpu_rebuilds} device builds installed (last {st.bvh_rebuild_ms:.1f} ms), sun rebuilds {st.sun_rebuilds}")
        assert st.bvh_gpu_fallbacks == 0 and st.bvh_rebuild_failures == 0
        assert ctx.world_bvh_check()["violations"] == 0, ctx.last_error()
    finally:
        ctx.close()
        orc.close()


def small_classes_scene():
    """5 opaque triangles (one of zero area), 1 masked, 2 blend: a class of one triangle (a
    root that is one leaf slot), of two, and one whose root is opened."""
    pos, idx, meshes, insts = [], [], [], []

    def add(P, tris, mat, mask):
        meshes.append((sum(len(p) for p in pos), sum(len(i) for i in idx), mat))
        pos.append(np.asarray(P, np.float32))
        idx.append(np.asarray(tris, np.uint32).reshape(-1))
        inst = np.zeros((), dtype=S.INSTANCE_DTYPE)
        inst["object_to_world"] = np.eye(3, 4, dtype=np.float32).reshape(-1)
        inst["rt_mesh_index"] = len(meshes) - 1
        inst["triangle_count"] = len(tris)
        inst["hit_mask"] = mask
        insts.append(inst)

    # a floor of two triangles, a back wall of two, and a zero-area triangle (three equal indices' worth of points)
    add([(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2), (-2, 0, -2), (2, 0, -2), (2, 3, -2), (-2, 3, -2), (0.5, 1.0, 0.5)],
        [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (8, 8, 8)], 0, abi.ARK_RT_HIT_MASK_OPAQUE)
    add([(-0.5, 0.5, 0.0), (0.5, 0.5, 0.0), (0.0, 1.5, 0.0)], [(0, 1, 2)], 1, abi.ARK_RT_HIT_MASK_MASKED)
    add([(-1, 2.0, -1), (1, 2.0, -1), (1, 2.0, 1), (-1, 2.0, 1)], [(0, 1, 2), (0, 2, 3)], 2, abi.ARK_RT_HIT_MASK_BLEND)
    m0 = S.default_material()
    m0["metallic_factor"] = 0.0
    m0["color_tint"] = (0.8, 0.7, 0.6, 1.0)
    m1 = S.default_material()
    m1["base_color"] = 0
    m1["blend_mode"] = abi.ARK_BLEND_MODE_MASKED
    m1["mask_cutoff"] = 0.5
    m2 = S.default_material()
    m2["blend_mode"] = abi.ARK_BLEND_MODE_TRANSLUCENT
    m2["color_tint"] = (0.2, 0.4, 0.9, 0.5)
    a = np.zeros((4, 4, 4), np.uint8)
    a[..., :3] = 200
    a[..., 3] = np.where((np.arange(4)[:, None] + np.arange(4)[None, :]) % 2 == 0, 255, 20)
    P = np.concatenate(pos)
    vx = np.zeros(len(P), dtype=S.VERTEX_DTYPE)
    vx["normal"] = (0, 1, 0)
    vx["tex_coord"] = P[:, [0, 2]]
    vx["tangent"] = (1, 0, 0, 1)
    return S.SceneData(positions=P, vertices=vx, indices=np.concatenate(idx), meshes=np.array(meshes, dtype=S.MESH_DTYPE),
                       materials=np.array([m0, m1, m2], dtype=S.MATERIAL_DTYPE), instances=np.array(insts, dtype=S.INSTANCE_DTYPE),
                       textures=[S.Texture(4, 4, abi.ARK_TEX_RGBA8_SRGB, a, abi.ARK_WRAP_REPEAT)],
                       sun=((2.0, 1.9, 1.7), tuple(np.array([0.3, -1.0, -0.4]) / np.linalg.norm([0.3, -1.0, -0.4]))))


def test_small_classes():
    sc = small_classes_scene()
    cfg = _cfg(gpu_rebuild=True)
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    orc = O.Oracle(ctx.desc)
    try:
        ctx.set_scene(sc)
        orc.set_scene(sc)
        first, f, t0 = 0, 0, time.time()
        while ctx.bvh_stats().bvh_gpu_rebuilds < 1:
            inst = _moved(sc.instances, f)
            ctx.set_instances(inst)
            orc.set_instances(inst)
            first = _frame(ctx, cfg, GRID, f, first, orc, "small classes, moving")
            f += 1
            assert time.time() - t0 < WAIT_S, f"no device build installed within {WAIT_S} s: {ctx.last_error()}"
        chk = ctx.world_bvh_check()
        st = ctx.bvh_stats()
        assert chk["violations"] == 0, (chk, ctx.last_error())
        assert st.bvh_gpu_fallbacks == 0 and chk["installed_builder"] == 1
        # a root node each: opaque (5 triangles: opened), masked (1) and blend (2): one leaf slot
        assert chk["nodes"] == 3 and chk["records"] == 8 and chk["max_depth"] == 1, chk
        # one frame traced through the device-built BVHs
        _frame(ctx, cfg, GRID, f, first, orc, "small classes, device build")
    finally:
        ctx.close()
        orc.close()


def test_settle_rebuild():
    """A static scene does not stay on an LBVH: after the motion stops, one host rebuild
    replaces the installed device build. Bit-exact throughout."""
    sc = S.soup(20_000, extent=7.0)
    grid = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
    cfg = _cfg(gpu_rebuild=True)
    ctx = D.DDGIContext(grid, 10000.0, cfg)
    orc = O.Oracle(ctx.desc)
    try:
        ctx.set_scene(sc)
        orc.set_scene(sc)
        first, f, t0 = 0, 0, time.time()
        while ctx.bvh_stats().bvh_gpu_rebuilds < 1:
            inst = _moved(sc.instances, f)
            ctx.set_instances(inst)
            orc.set_instances(inst)
            first = _frame(ctx, cfg, grid, f, first, orc, "moving")
            f += 1
            assert time.time() - t0 < WAIT_S, f"no device build installed within {WAIT_S} s: {ctx.last_error()}"
        moving = ctx.bvh_stats()
        # the motion stops: device builds until one is of the last transforms, then the host's
        t0 = time.time()
        while True:
            first = _frame(ctx, cfg, grid, f, first, orc, "settling")
            f += 1
            st = ctx.bvh_stats()
            if st.bvh_installed_builder == 0 and st.bvh_rebuilds > moving.bvh_rebuilds:
                break
            assert time.time() - t0 < WAIT_S, f"no settle rebuild within {WAIT_S} s (rebuilds {st.bvh_rebuilds}, device {st.bvh_gpu_rebuilds}): {ctx.last_error()}"
        assert st.bvh_built_refit_version == st.refit_version and st.bvh_rebuild_failures == 0
        chk = ctx.world_bvh_check()
        assert chk["violations"] == 0 and chk["installed_builder"] == 0, chk
        # and it stays: nothing more is started
        rebuilds = st.bvh_rebuilds
        for _ in range(3):
            first = _frame(ctx, cfg, grid, f, first, orc, "settled")
            f += 1
        assert ctx.bvh_stats().bvh_rebuilds == rebuilds
    finally:
        ctx.close()
        orc.close()


def test_rebuilt_tree_is_tighter_than_refitted():
    """The 512 boxes of a city block swap their whole transforms among themselves: every
    low node of the refitted tree then spans boxes from all over the block, while the
    rebuilt one groups neighbours again. Same hits, fewer node visits."""
    sc0 = S.city_block(box_count=512, extent=40.0)
    sc = S.SceneData(**{**{k: v for k, v in sc0.__dict__.items() if not k.startswith("_")}, "spots": []})
    grid = D.ProbeGrid((4, 4, 4), (10.0, 3.0, 10.0), (5.0, 1.0, 5.0))
    inst = sc.instances.copy()
    perm = np.random.default_rng(1234).permutation(512)
    inst["object_to_world"][:512] = sc.instances["object_to_world"][:512][perm]  # the ground (the last instance) stays
    p = None
    out = {}
    for name, kw in (("refitted", dict(background_rebuild=False)), ("rebuilt", dict(gpu_rebuild=True))):
        cfg = _cfg(R=64, K=64, **kw)
        ctx = D.DDGIContext(grid, 1000.0, cfg)
        try:
            ctx.set_scene(sc)
            ctx.set_counting(True)
            ctx.set_instances(inst)
            if name == "rebuilt":
                t0 = time.time()
                while ctx.bvh_stats().bvh_gpu_rebuilds < 1:
                    ctx.set_instances(inst)  # (an update or a set_instances installs a finished build)
                    assert time.time() - t0 < WAIT_S, f"no device build installed within {WAIT_S} s: {ctx.last_error()}"
                assert ctx.bvh_stats().bvh_installed_builder == 1
                assert ctx.world_bvh_check()["violations"] == 0, ctx.last_error()
            p = D.frame_params(cfg, grid, D.AppState(0), 0, **EXPOSURE)
            ctx.update(p)
            ctx.synchronize()
            out[name] = (int(ctx.counters().primary_node_visits), {k: ctx.read(w) for k, w in RESOURCES.items()})
        finally:
            ctx.close()
    print(f"primary node visits, 512 permuted boxes: refitted {out['refitted'][0]}, device-rebuilt {out['rebuilt'][0]}")
    for k in RESOURCES:
        assert diff_report(k, out["rebuilt"][1][k], out["refitted"][1][k])["mismatch"] == 0, k
    assert out["rebuilt"][0] < out["refitted"][0]


def test_flag_off():
    """The default: rebuilds stay the host's."""
    sc = S.soup(20_000, extent=7.0)
    grid = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
    cfg = _cfg()
    assert not cfg.gpu_rebuild
    ctx = D.DDGIContext(grid, 10000.0, cfg)
    try:
        ctx.set_scene(sc)
        first, f, t0 = 0, 0, time.time()
        while ctx.bvh_stats().bvh_rebuilds < 1:
            if f < 4:
                ctx.set_instances(_moved(sc.instances, f))
            first = _frame(ctx, cfg, grid, f, first)
            f += 1
            assert time.time() - t0 < WAIT_S, f"no host rebuild installed within {WAIT_S} s: {ctx.last_error()}"
        st = ctx.bvh_stats()
        assert st.bvh_gpu_rebuilds == 0 and st.bvh_installed_builder == 0 and st.bvh_gpu_fallbacks == 0
        assert ctx.world_bvh_check()["installed_builder"] == 0
    finally:
        ctx.close()
