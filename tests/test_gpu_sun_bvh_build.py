"""The sun's light-space BVH8 rebuilt on the device (ARK_DDGI_FLAG_GPU_REBUILD_SUN,
DDGIConfig.gpu_rebuild_sun; csrc/ddgi_bvh_build.hip k_lbvh_prims_light / k_lbvh_keys_light):
one LBVH over every class's records, keyed and boxed in the sun's frame, installed by the
background-rebuild machinery after refits and after a sun-direction change. Hits do not
depend on the tree, so every frame stays bit-exact against the oracle across the installs;
ark_ddgi_debug_sun_bvh_installed_check downloads the installed tree and checks it on the
host. Once no refit has come since its snapshot one host rebuild replaces it."""
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
SOUP_GRID = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
EXPOSURE = dict(light_pre_exposure=1.0, environment_brightness=1.0)
WAIT_S = 60  # wall-clock bound of every polling loop


def _cfg(R=32, K=64, **kw):
    kw.setdefault("sun_bvh", abi.ARK_DDGI_SUN_BVH_LIGHT_SPACE)
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
    """The features scene, whose three hit-mask classes share the one tree: the installed
    device build is a valid BVH8 over the same records as the world BVHs hold, bit for bit
    those a refit alone leaves."""
    sc = scenes.features_scene()
    cfg = _cfg(gpu_rebuild_sun=True)
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ref = D.DDGIContext(GRID, 100.0, _cfg(background_rebuild=False))
    try:
        ctx.set_scene(sc)
        before = ctx.sun_bvh_installed_check()
        assert before["installed"] and before["violations"] == 0 and before["installed_builder"] == 0, (before, ctx.last_error())
        assert (before["records"], before["record_digest"]) == tuple(ctx.world_bvh_check()[k] for k in ("records", "record_digest"))
        first, f, t0 = 0, 0, time.time()
        inst = sc.instances
        while ctx.bvh_stats().sun_gpu_rebuilds < 1:
            inst = _moved(sc.instances, f)
            ctx.set_instances(inst)
            first = _frame(ctx, cfg, GRID, f, first)
            f += 1
            assert time.time() - t0 < WAIT_S, f"no device build of the sun BVH installed within {WAIT_S} s: {ctx.last_error()}"
        st = ctx.bvh_stats()
        after = ctx.sun_bvh_installed_check()
        world = ctx.world_bvh_check()
        print(f"features scene: device build of the sun BVH installed after {f} frames in {st.sun_build_ms:.1f} ms: {after}")
        assert after["violations"] == 0, (after, ctx.last_error())
        assert st.sun_installed_builder == 1 and after["installed_builder"] == 1
        assert st.sun_gpu_fallbacks == 0 and st.sun_rebuild_failures == 0
        assert st.bvh_gpu_rebuilds == 0  # the world flag is off
        assert world["violations"] == 0
        assert (after["records"], after["record_digest"]) == (world["records"], world["record_digest"])
        # the records whichever builder placed them: a refit of set_scene's BVHs to the same transforms
        ref.set_scene(sc)
        ref.set_instances(inst)
        want = ref.sun_bvh_installed_check()
        assert want["violations"] == 0 and want["installed_builder"] == 0
        assert (after["records"], after["record_digest"]) == (want["records"], want["record_digest"])
        wantw = ref.world_bvh_check()
        assert (after["records"], after["record_digest"]) == (wantw["records"], wantw["record_digest"])
    finally:
        ctx.close()
        ref.close()


def small_classes_scene():
    """test_gpu_bvh_build.py's: 5 opaque triangles (one of zero area), 1 masked, 2 blend."""
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


def test_small_scene():
    """8 records, one of zero area: the tree is one root node."""
    sc = small_classes_scene()
    cfg = _cfg(gpu_rebuild_sun=True)
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    orc = O.Oracle(ctx.desc)
    try:
        ctx.set_scene(sc)
        orc.set_scene(sc)
        assert ctx.bvh_stats().sun_node_count > 0
        first, f, t0 = 0, 0, time.time()
        while ctx.bvh_stats().sun_gpu_rebuilds < 1:
            inst = _moved(sc.instances, f)
            ctx.set_instances(inst)
            orc.set_instances(inst)
            first = _frame(ctx, cfg, GRID, f, first, orc, "small scene, moving")
            f += 1
            assert time.time() - t0 < WAIT_S, f"no device build of the sun BVH installed within {WAIT_S} s: {ctx.last_error()}"
        chk = ctx.sun_bvh_installed_check()
        st = ctx.bvh_stats()
        assert chk["violations"] == 0, (chk, ctx.last_error())
        assert st.sun_gpu_fallbacks == 0 and chk["installed_builder"] == 1 and st.sun_installed_builder == 1
        assert chk["nodes"] == 1 and chk["records"] == 8 and chk["max_depth"] == 1, chk
        # one frame traced through the device-built tree
        _frame(ctx, cfg, GRID, f, first, orc, "small scene, device build")
    finally:
        ctx.close()
        orc.close()


def test_parity_across_installs():
    """Both flags under continuous motion on a side stream: every frame bit-exact against
    the oracle until the world BVHs and the sun's have each been device-built twice."""
    import torch

    sc = S.soup(20_000, extent=7.0)
    cfg = _cfg(compute_probe_offsets=True, gpu_rebuild=True, gpu_rebuild_sun=True)
    ctx = D.DDGIContext(SOUP_GRID, 10000.0, cfg)
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
            p = D.frame_params(cfg, SOUP_GRID, D.AppState(f), first, **EXPOSURE)
            ctx.update(p, stream.cuda_stream)
            orc.update(p)
            ctx.synchronize()
            _compare(ctx, orc, f, "continuous motion, device rebuilds of both")
            st = ctx.bvh_stats()
            first = (first + p.probe_updates) % SOUP_GRID.probe_count()
            f += 1
            if st.sun_gpu_rebuilds >= 2 and st.bvh_gpu_rebuilds >= 2:
                break
            assert time.time() - t0 < WAIT_S, f"{st.bvh_gpu_rebuilds} world and {st.sun_gpu_rebuilds} sun device builds within {WAIT_S} s: {ctx.last_error()}"
        print(f"continuous motion: {f} frames, device builds installed: world {st.bvh_gpu_rebuilds} (last {st.bvh_rebuild_ms:.1f} ms), "
              f"sun {st.sun_gpu_rebuilds} (last {st.sun_build_ms:.1f} ms)")
        assert st.bvh_gpu_fallbacks == 0 and st.sun_gpu_fallbacks == 0
        assert st.bvh_rebuild_failures == 0 and st.sun_rebuild_failures == 0
        assert ctx.world_bvh_check()["violations"] == 0, ctx.last_error()
        assert ctx.sun_bvh_installed_check()["violations"] == 0, ctx.last_error()
    finally:
        ctx.close()
        orc.close()


def test_sun_direction_change():
    """A static scene whose sun turns: the device build for the new direction is installed,
    then the settle rebuild replaces it with the host's tree, and nothing more starts."""
    sc = S.soup(20_000, extent=7.0)
    cfg = _cfg(gpu_rebuild_sun=True)
    ctx = D.DDGIContext(SOUP_GRID, 10000.0, cfg)
    orc = O.Oracle(ctx.desc)
    try:
        ctx.set_scene(sc)
        orc.set_scene(sc)
        first, f = 0, 0
        first = _frame(ctx, cfg, SOUP_GRID, f, first, orc, "before")
        f += 1
        for d in ((0.3, -1.0, -0.4), (-0.5, -1.0, 0.2)):
            d = np.asarray(d, np.float32)
            sun = (sc.sun[0], tuple(float(x) for x in d / np.linalg.norm(d)))
            ctx.set_lights(sun, ())
            orc.set_lights(sun, ())
            start = ctx.bvh_stats()
            # the device build for this direction
            t0 = time.time()
            while ctx.bvh_stats().sun_gpu_rebuilds == start.sun_gpu_rebuilds:
                first = _frame(ctx, cfg, SOUP_GRID, f, first, orc, "direction changed")
                f += 1
                assert time.time() - t0 < WAIT_S, f"no device build for the new direction within {WAIT_S} s: {ctx.last_error()}"
            st = ctx.bvh_stats()
            assert st.sun_installed_builder == 1 and st.sun_rebuilds == start.sun_rebuilds + 1
            chk = ctx.sun_bvh_installed_check()
            assert chk["violations"] == 0 and chk["installed_builder"] == 1, (chk, ctx.last_error())
            first = _frame(ctx, cfg, SOUP_GRID, f, first, orc, "device build installed")
            f += 1
            # the settle rebuild
            t0 = time.time()
            while ctx.bvh_stats().sun_installed_builder != 0:
                first = _frame(ctx, cfg, SOUP_GRID, f, first, orc, "settling")
                f += 1
                assert time.time() - t0 < WAIT_S, f"no settle rebuild within {WAIT_S} s: {ctx.last_error()}"
            st = ctx.bvh_stats()
            assert st.sun_rebuilds == start.sun_rebuilds + 2 and st.sun_gpu_rebuilds == start.sun_gpu_rebuilds + 1
            chk = ctx.sun_bvh_installed_check()
            assert chk["violations"] == 0 and chk["installed_builder"] == 0, (chk, ctx.last_error())
            # and it stays: nothing more is started
            for _ in range(3):
                first = _frame(ctx, cfg, SOUP_GRID, f, first, orc, "settled")
                f += 1
            st = ctx.bvh_stats()
            assert st.sun_rebuilds == start.sun_rebuilds + 2 and st.sun_gpu_fallbacks == 0 and st.sun_rebuild_failures == 0
            assert st.bvh_rebuilds == 0
    finally:
        ctx.close()
        orc.close()


def test_flag_off():
    """gpu_rebuild alone: the sun's rebuilds stay the host's."""
    sc = S.soup(20_000, extent=7.0)
    cfg = _cfg(gpu_rebuild=True)
    assert not cfg.gpu_rebuild_sun
    ctx = D.DDGIContext(SOUP_GRID, 10000.0, cfg)
    try:
        ctx.set_scene(sc)
        first, f, t0 = 0, 0, time.time()
        while ctx.bvh_stats().sun_rebuilds < 1:
            if f < 4:
                ctx.set_instances(_moved(sc.instances, f))
            first = _frame(ctx, cfg, SOUP_GRID, f, first)
            f += 1
            assert time.time() - t0 < WAIT_S, f"no sun rebuild installed within {WAIT_S} s: {ctx.last_error()}"
        st = ctx.bvh_stats()
        assert st.sun_gpu_rebuilds == 0 and st.sun_installed_builder == 0 and st.sun_gpu_fallbacks == 0
        chk = ctx.sun_bvh_installed_check()
        assert chk["violations"] == 0 and chk["installed_builder"] == 0, (chk, ctx.last_error())
    finally:
        ctx.close()
