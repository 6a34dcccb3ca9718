"""Deforming meshes through the C-ABI (ark_ddgi_update_geometry): ranges of the vertex pools
replaced between updates, with or without new transforms, as one device refit.

The reference skins its skeletal-mesh instances into the vertex pools every frame and
updates their BLASes (GpuScene.cpp:629-711, :934-992). Here the oracle is handed the
deformed pools as a new scene each time (oracle_set_scene keeps the atlas history). Bar:
bit-exact atlases and offsets after every call, whatever the refit skipped, whichever of
the three geometry copies it wrote and whoever built the BVHs in between.
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

GRID = D.ProbeGrid((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))
EXPOSURE = dict(light_pre_exposure=1.0, ambient_illuminance=0.05, environment_brightness=0.5)
BOX, MIRRORED, MASKED = 3, 4, 1  # instances of scenes.features_scene(); 3 and 4 share one RT mesh


def _cfg(R=128, K=144, **kw):
    return D.DDGIConfig(rays_per_probe=R, probe_updates_per_frame=K, compute_probe_offsets=True, max_rays_per_probe=R, max_probe_updates=144, **kw)


def _compare(ctx, orc, what):
    for k, w in RESOURCES.items():
        r = diff_report(k, ctx.read(w), orc.read(w))
        assert r["mismatch"] == 0, f"{what}: {r}"


def _with(sc, **kw):
    return S.SceneData(**{**sc.__dict__, **kw})


def _mesh_range(sc, instance):
    """(first vertex, vertex count) of the pool range the instance's mesh reaches."""
    m = sc.meshes[int(sc.instances["rt_mesh_index"][instance])]
    n = 3 * int(sc.instances["triangle_count"][instance])
    idx = sc.indices[int(m["first_index"]):int(m["first_index"]) + n]
    return int(m["first_vertex"]), int(idx.max()) + 1


def _wobble(sc, instance, phase, amp=0.05):
    """The mesh range of `instance` displaced by a sine of its own rest positions, its normals
    recomputed (away from the range's centre): (first, positions, vertices) of the range."""
    first, n = _mesh_range(sc, instance)
    P0 = sc.positions[first:first + n].astype(np.float32)
    P = (P0 + np.float32(amp) * np.sin(np.float32(phase) + np.float32(3.0) * P0[:, [1, 2, 0]])).astype(np.float32)
    V = sc.vertices[first:first + n].copy()
    nrm = P - P.mean(0)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-6)
    V["normal"] = nrm.astype(np.float32)
    return first, P, V


def _apply(sc, P, V, first, p, v):
    P[first:first + len(p)] = p
    if v is not None:
        V[first:first + len(v)] = v


def _frame(ctx, orc, cfg, grid, f, idx, what, exposure=EXPOSURE):
    p = D.frame_params(cfg, grid, D.AppState(f), idx, **exposure)
    ctx.update(p)
    orc.update(p)
    ctx.synchronize()
    _compare(ctx, orc, f"frame {f} ({what})")
    return (idx + p.probe_updates) % grid.probe_count()


def _sun(mode):
    return abi.ARK_DDGI_SUN_BVH_LIGHT_SPACE if mode == "light" else abi.ARK_DDGI_SUN_BVH_WORLD


@pytest.mark.parametrize("sun_bvh", ["light", "world"])
def test_five_frames_deform_and_move(sun_bvh):
    """Every frame the box mesh (instances 3 and its mirrored twin 4) is displaced by a sine
    and its normals recomputed; from frame 2 the mirrored box also moves rigidly in the same
    call. Atlases and offsets equal the oracle's, which is handed the deformed pools."""
    sc = scenes.features_scene()
    cfg = _cfg(sun_bvh=_sun(sun_bvh))
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    P, V = sc.positions.copy(), sc.vertices.copy()
    inst = sc.instances.copy()
    idx = 0
    try:
        idx = _frame(ctx, orc, cfg, GRID, 0, idx, "rest")
        for f in range(1, 6):
            first, p, v = _wobble(sc, BOX, 0.9 * f)
            _apply(sc, P, V, first, p, v)
            moved = None
            if f >= 2:
                M = inst["object_to_world"].reshape(-1, 3, 4).copy()
                M[MIRRORED, :, 3] += np.array([0.07, 0.0, 0.05], np.float32)
                inst["object_to_world"] = M.reshape(len(inst), 12)
                moved = inst
            ctx.update_geometry([D.VertexUpdate(first, p, v)], moved)
            orc.set_scene(_with(sc, positions=P.copy(), vertices=V.copy(), instances=inst.copy()))
            assert (ctx.bvh_stats().sun_node_count > 0) == (sun_bvh == "light")
            idx = _frame(ctx, orc, cfg, GRID, f, idx, "deformed" + (" and moved" if moved is not None else ""))
        assert ctx.geometry_update_stats() == (5, 5 * len(p), 0, 0)
        info = ctx.geometry_update_info()
        assert info["map_allocations"] == 1 and info["map_fills"] >= 1 and info["position_updates"] == 5  # (a fill more per installed world rebuild)
    finally:
        ctx.close()
        orc.close()


def test_records_equal_fresh_set_scene():
    """After three deformations the BVHs are valid and hold, bit for bit, the records a fresh
    set_scene of the deformed pools holds (the order-independent record digest), world and
    light-space."""
    sc = scenes.features_scene()
    cfg = _cfg(R=32, sun_bvh=_sun("light"), background_rebuild=False)
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    P, V = sc.positions.copy(), sc.vertices.copy()
    for f in range(1, 4):
        first, p, v = _wobble(sc, BOX, 1.3 * f)
        _apply(sc, P, V, first, p, v)
        ctx.update_geometry([D.VertexUpdate(first, p, v)])
    ref = D.DDGIContext(GRID, 100.0, cfg)
    ref.set_scene(_with(sc, positions=P, vertices=V))
    try:
        for check in ("world_bvh_check", "sun_bvh_installed_check"):
            got, want = getattr(ctx, check)(), getattr(ref, check)()
            assert got["violations"] == 0 and want["violations"] == 0, (check, got, want)
            assert got["records"] == want["records"] and got["record_digest"] == want["record_digest"], (check, got, want)
        assert ctx.sun_bvh_installed_check()["installed"]
    finally:
        ctx.close()
        ref.close()


SOUP_GRID = D.ProbeGrid((4, 4, 4), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))


def test_three_copies_catch_up():
    """A soup of 20,480 triangles in 80 instances (instance bits alias mod 64), instances 3
    and 67 deformed. One deformation, then three refits that move only another instance: each
    brings another of the three copies, which last saw the old vertices, up to date. Then the
    deformation A -> B -> A and a loop of period 3, where a copy's records are as old as the
    pose coming back. The oracle agrees after every call, and the records end equal to a
    fresh set_scene's."""
    sc = S.soup(20_480, extent=7.0, material_count=80)
    assert len(sc.instances) == 80 and sc.triangle_count == 20_480
    cfg = D.DDGIConfig(rays_per_probe=32, probe_updates_per_frame=64, compute_probe_offsets=True, max_rays_per_probe=32, max_probe_updates=64,
                       sun_bvh=_sun("light"), background_rebuild=False)
    ctx = D.DDGIContext(SOUP_GRID, 10000.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    exposure = dict(light_pre_exposure=1.0, environment_brightness=1.0)
    P, V = sc.positions.copy(), sc.vertices.copy()
    inst = sc.instances.copy()
    state = {"idx": 0, "f": 0}

    def pose(k):
        """Pose k of the two deformed instances (0: rest)."""
        ups = []
        for i in (3, 67):
            first, p, v = _wobble(sc, i, 1.1 * k + i, amp=0.0 if k == 0 else 0.08)
            _apply(sc, P, V, first, p, v)
            ups.append(D.VertexUpdate(first, p, v))
        return ups

    def step(ups, moved, what):
        ctx.update_geometry(ups, moved)
        orc.set_scene(_with(sc, positions=P.copy(), vertices=V.copy(), instances=inst.copy()))
        state["idx"] = _frame(ctx, orc, cfg, SOUP_GRID, state["f"], state["idx"], what, exposure)
        state["f"] += 1

    try:
        step(pose(1), None, "deformed once")
        for k in range(3):
            M = inst["object_to_world"].reshape(-1, 3, 4).copy()
            M[5, :, 3] += np.float32(0.05)
            inst["object_to_world"] = M.reshape(len(inst), 12)
            step([], inst, f"other instance moved, refit {k + 1}")
        for k in (2, 1, 2, 1):
            step(pose(k), None, f"A -> B -> A: pose {k}")
        for k in (0, 1, 2, 0, 1, 2, 0):
            step(pose(k), None, f"period 3: pose {k}")
        ref = D.DDGIContext(SOUP_GRID, 10000.0, cfg)
        try:
            ref.set_scene(_with(sc, positions=P, vertices=V, instances=inst))
            for check in ("world_bvh_check", "sun_bvh_installed_check"):
                got, want = getattr(ctx, check)(), getattr(ref, check)()
                assert got["violations"] == 0, (check, got)
                assert got["record_digest"] == want["record_digest"], (check, got, want)
        finally:
            ref.close()
    finally:
        ctx.close()
        orc.close()


def test_shared_mesh_moves_both_instances():
    """The box and the mirrored box draw one RT mesh: one range update re-derives the records
    of both (the refit reaches nodes of both), and the frame equals the oracle's."""
    sc = scenes.features_scene()
    cfg = _cfg(sun_bvh=_sun("world"), background_rebuild=False)
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    P, V = sc.positions.copy(), sc.vertices.copy()
    first, p, v = _wobble(sc, MIRRORED, 0.4, amp=0.1)
    _apply(sc, P, V, first, p, v)
    deformed = _with(sc, positions=P, vertices=V)
    orc.set_scene(deformed)
    ref = D.DDGIContext(GRID, 100.0, cfg)
    try:
        ctx.update_geometry([D.VertexUpdate(first, p, v)])
        _frame(ctx, orc, cfg, GRID, 0, 0, "shared mesh deformed")
        ref.set_scene(deformed)
        assert ctx.world_bvh_check()["record_digest"] == ref.world_bvh_check()["record_digest"]
        ref.set_scene(sc)
        ref.set_instances(sc.instances)  # (its records of the old vertices, for the control below)
        assert ctx.world_bvh_check()["record_digest"] != ref.world_bvh_check()["record_digest"]
    finally:
        ctx.close()
        ref.close()
        orc.close()


def test_masked_quads_positions_and_uvs():
    """The alpha-tested quads get new positions and new UVs: the any-hit alpha test of the
    probe rays and the shadow rays reads the vertex pool, the shading its records."""
    sc = scenes.features_scene()
    cfg = _cfg(sun_bvh=_sun("light"))
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    P, V = sc.positions.copy(), sc.vertices.copy()
    idx = 0
    try:
        idx = _frame(ctx, orc, cfg, GRID, 0, idx, "rest")
        for f in (1, 2):
            first, p, v = _wobble(sc, MASKED, 0.8 * f, amp=0.12)
            v["tex_coord"] = (sc.vertices["tex_coord"][first:first + len(v)] * np.float32(1.0 + 0.5 * f) + np.float32(0.13 * f)).astype(np.float32)
            v["normal"] = sc.vertices["normal"][first:first + len(v)]
            _apply(sc, P, V, first, p, v)
            ctx.update_geometry([D.VertexUpdate(first, p, v)])
            orc.set_scene(_with(sc, positions=P.copy(), vertices=V.copy()))
            idx = _frame(ctx, orc, cfg, GRID, f, idx, "masked quads deformed, new UVs")
    finally:
        ctx.close()
        orc.close()


@pytest.mark.parametrize("gpu", [False, True])
def test_deform_every_frame_across_installs(gpu):
    """An instance deforms every frame for at least 40 frames, enqueued without host waits,
    while background rebuilds (host, or both device builds) snapshot, build and install -
    refitted forward over the deformations that came in meanwhile, the triangle -> record
    map filled again. After a world and a sun install, one more deformed frame equals the
    oracle's, which is given the context's history."""
    import torch

    sc = S.soup(64_000, extent=7.0)
    grid = D.ProbeGrid((8, 8, 8), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    cfg = D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=200, compute_probe_offsets=True, max_rays_per_probe=64, max_probe_updates=200,
                       sun_bvh=_sun("light"), gpu_rebuild=gpu, gpu_rebuild_sun=gpu)
    ctx = D.DDGIContext(grid, 10000.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    stream = torch.cuda.Stream()
    exposure = dict(light_pre_exposure=1.0, environment_brightness=1.0)
    P, V = sc.positions.copy(), sc.vertices.copy()
    first_probe, f, t0 = 0, 0, time.time()
    try:
        while True:
            first, p, v = _wobble(sc, 2, 0.3 * f, amp=0.1)
            ctx.update_geometry_async([D.VertexUpdate(first, p, v)], None, stream.cuda_stream)
            prm = D.frame_params(cfg, grid, D.AppState(f), first_probe, **exposure)
            ctx.update(prm, stream.cuda_stream)
            first_probe = (first_probe + prm.probe_updates) % grid.probe_count()
            f += 1
            st = ctx.bvh_stats()
            if f >= 40 and st.bvh_rebuilds >= 1 and st.sun_rebuilds >= 1:
                break
            if f >= 40:
                ctx.synchronize()
            assert time.time() - t0 < 120, f"rebuilds not installed within 120 s (world {st.bvh_rebuilds}, sun {st.sun_rebuilds})"
        ctx.synchronize()
        assert ctx.geometry_update_info()["map_fills"] >= 2  # the first use, and after a world install
        first, p, v = _wobble(sc, 2, 0.3 * f, amp=0.1)
        _apply(sc, P, V, first, p, v)
        orc.set_scene(_with(sc, positions=P, vertices=V))
        for w in RESOURCES.values():
            orc.write(w, ctx.read(w))
        ctx.update_geometry_async([D.VertexUpdate(first, p, v)], None, stream.cuda_stream)
        prm = D.frame_params(cfg, grid, D.AppState(f), first_probe, **exposure)
        ctx.update(prm, stream.cuda_stream)
        orc.update(prm)
        ctx.synchronize()
        _compare(ctx, orc, f"frame {f} after installs (world {st.bvh_rebuilds}, sun {st.sun_rebuilds})")
        assert ctx.world_bvh_check()["violations"] == 0
    finally:
        ctx.close()
        orc.close()


@pytest.mark.parametrize("with_vertices", [False, True])
def test_frames_in_flight(with_vertices):
    """Eight deformations, each followed by an update, queued on one stream without a host
    wait (positions alone, which leave the frames pipelined, or with the other vertex
    data): every frame traces and shades its own geometry, so the end equals the oracle's,
    which ran them one by one."""
    import torch

    sc = scenes.features_scene()
    cfg = _cfg(R=64, sun_bvh=_sun("light"))
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    stream = torch.cuda.Stream()
    P, V = sc.positions.copy(), sc.vertices.copy()
    idx = 0
    try:
        for f in range(9):
            if f > 0:
                first, p, v = _wobble(sc, BOX, 0.9 * f, amp=0.1)
                if not with_vertices:
                    v = None
                _apply(sc, P, V, first, p, v)
                ctx.update_geometry_async([D.VertexUpdate(first, p, v)], None, stream.cuda_stream)
                orc.set_scene(_with(sc, positions=P.copy(), vertices=V.copy()))
            prm = D.frame_params(cfg, GRID, D.AppState(f), idx, **EXPOSURE)
            ctx.update(prm, stream.cuda_stream)
            orc.update(prm)
            idx = (idx + prm.probe_updates) % GRID.probe_count()
        ctx.synchronize()
        _compare(ctx, orc, "nine frames in flight")
    finally:
        ctx.close()
        orc.close()


def test_shared_scene_sees_the_deformation():
    """B shares A's scene: a deformation through A is what B's next update traces and shades."""
    sc = scenes.features_scene()
    cfg = _cfg(sun_bvh=_sun("light"))
    a = D.DDGIContext(GRID, 100.0, cfg)
    b = D.DDGIContext(GRID, 100.0, cfg)
    a.set_scene(sc)
    b.share_scene(a)
    orc = O.Oracle(b.desc)
    orc.set_scene(sc)
    P, V = sc.positions.copy(), sc.vertices.copy()
    try:
        idx = _frame(b, orc, cfg, GRID, 0, 0, "B, rest")
        a.update(D.frame_params(cfg, GRID, D.AppState(0), 0, **EXPOSURE))  # (A has a frame in flight)
        first, p, v = _wobble(sc, BOX, 2.0, amp=0.1)
        _apply(sc, P, V, first, p, v)
        a.update_geometry([D.VertexUpdate(first, p, v)])
        orc.set_scene(_with(sc, positions=P, vertices=V))
        _frame(b, orc, cfg, GRID, 1, idx, "B after A deformed the box")
    finally:
        a.close()
        b.close()
        orc.close()


def test_device_source():
    """A torch device tensor as the source gives byte for byte what the host source gives. A
    buffer with one position outside `bounds` and one NaN gives what the host source of the
    clamped / kept data gives; the stats count one of each, and nothing hangs."""
    import torch

    sc = scenes.features_scene()
    cfg = _cfg(R=32, sun_bvh=_sun("light"), background_rebuild=False)
    host = D.DDGIContext(GRID, 100.0, cfg)
    dev = D.DDGIContext(GRID, 100.0, cfg)
    host.set_scene(sc)
    dev.set_scene(sc)
    stream = torch.cuda.current_stream().cuda_stream
    prm = D.frame_params(cfg, GRID, D.AppState(0), 0, **EXPOSURE)

    def both(p_host, p_dev, v, first, bounds, what):
        host.update_geometry([D.VertexUpdate(first, p_host, v)])
        tp = torch.from_numpy(p_dev).cuda()
        tv = torch.from_numpy(v.view(np.float32).reshape(-1, 9).copy()).cuda()
        torch.cuda.synchronize()
        dev.update_geometry_async([D.VertexUpdate(first, tp, tv, bounds=bounds)], None, stream)
        dev.synchronize()
        assert host.scene_digest() == dev.scene_digest(), what
        for c in (host, dev):
            c.update(prm)
            c.synchronize()
        for k, w in RESOURCES.items():
            assert np.array_equal(host.read(w), dev.read(w)), (what, k)

    try:
        first, p, v = _wobble(sc, BOX, 1.0, amp=0.1)
        _, p2, v2 = _wobble(sc, BOX, 2.0, amp=0.1)
        lo = np.minimum(p.min(0), p2.min(0)) - np.float32(0.01)
        hi = np.maximum(p.max(0), p2.max(0)) + np.float32(0.01)
        bounds = np.concatenate([lo, hi])
        both(p, p, v, first, bounds, "clean device source")
        assert dev.geometry_update_stats() == (1, len(p), 0, 0)
        bad = p2.copy()
        bad[2, 1] = np.float32(hi[1] + 5.0)  # outside: clamped to hi
        bad[5, 0] = np.float32("nan")        # dropped: the vertex keeps its old position, p[5]
        want = p2.copy()
        want[2, 1] = hi[1]
        want[5] = p[5]
        both(want, bad, v2, first, bounds, "one position outside bounds, one NaN")
        assert dev.geometry_update_stats() == (2, 2 * len(p), 1, 1)
    finally:
        host.close()
        dev.close()


def test_reflections_and_bake_of_the_deformed_instance():
    """A 64 x 36 rt_reflections and a 32 x 32 AO bake of the deformed box (which gets UVs with
    the deformation, so that the bake has texels) equal the oracle's on the deformed scene."""
    import torch

    import reflection_inputs as RI

    sc = scenes.features_scene()
    cfg = _cfg(R=64, sun_bvh=_sun("light"))
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    P, V = sc.positions.copy(), sc.vertices.copy()
    try:
        idx = _frame(ctx, orc, cfg, GRID, 0, 0, "rest")
        ctx.bake_ao(BOX, 32, 32, 8, False)  # (a reader of the positions pool ahead of the update)
        first, p, v = _wobble(sc, BOX, 1.7, amp=0.1)
        v["tex_coord"] = np.array([[0.05, 0.05], [0.95, 0.1], [0.1, 0.9], [0.9, 0.95], [0.5, 0.05], [0.95, 0.5], [0.05, 0.5], [0.5, 0.95]], np.float32)
        _apply(sc, P, V, first, p, v)
        ctx.update_geometry([D.VertexUpdate(first, p, v)])
        orc.set_scene(_with(sc, positions=P, vertices=V))
        _frame(ctx, orc, cfg, GRID, 1, idx, "deformed")
        W, H = 64, 36
        cam = RI.camera(W, H)
        g, _ = RI.gbuffer(W, H, cam, seed=3)
        kw = dict(environment_multiplier=0.5, ambient_amount=0.05)
        want_rad, want_dir = orc.rt_reflections(W, H, cam, g, **kw)
        t = {k: torch.from_numpy(np.ascontiguousarray(x)).cuda() for k, x in g.items()}
        rad = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
        dirs = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
        D.RTReflectionsNode().execute(ctx, cam, {k: t[k] for k in ("depth", "material", "normal_velocity")}, t["blue_noise"], rad, dirs, **kw)
        assert np.array_equal(rad.cpu().numpy().view(np.uint16), want_rad)
        assert np.array_equal(dirs.cpu().numpy().view(np.uint16), want_dir)
        ctx.bake_ao(BOX, 32, 32, 8, True)
        got = [ctx.bake_read(w) for w in (abi.ARK_BAKE_TRIANGLE_INDEX, abi.ARK_BAKE_BARYCENTRICS, abi.ARK_BAKE_OUTPUT)]
        want = orc.bake_ao(BOX, 32, 32, 8, True)
        assert (got[0] > 0).mean() > 0.2
        for name, x, y in zip(("triangle index", "barycentrics", "output"), got, want):
            assert np.array_equal(x, y), name
    finally:
        ctx.close()
        orc.close()


def test_bake_between_two_updates():
    """Update, bake, update, with no host wait between the bake and the second update: the
    bake reads the positions pool on the caller's stream while the second update stages its
    positions on the refit stream, which must wait for the bake (the event recorded after
    it). The bake equals the oracle's of the first pose, the next frame the oracle's of the
    second."""
    import torch

    sc = scenes.features_scene()
    cfg = _cfg(R=64, sun_bvh=_sun("light"))
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    stream = torch.cuda.Stream().cuda_stream
    uv = np.array([[0.05, 0.05], [0.95, 0.1], [0.1, 0.9], [0.9, 0.95], [0.5, 0.05], [0.95, 0.5], [0.05, 0.5], [0.5, 0.95]], np.float32)
    P, V = sc.positions.copy(), sc.vertices.copy()
    try:
        first, p1, v1 = _wobble(sc, BOX, 0.6, amp=0.1)
        v1["tex_coord"] = uv
        _apply(sc, P, V, first, p1, v1)
        ctx.update_geometry_async([D.VertexUpdate(first, p1, v1)], None, stream)
        orc.set_scene(_with(sc, positions=P.copy(), vertices=V.copy()))
        want = orc.bake_ao(BOX, 64, 64, 16, True)
        ctx.bake_ao(BOX, 64, 64, 16, True, stream)
        first, p2, v2 = _wobble(sc, BOX, 2.4, amp=0.15)
        v2["tex_coord"] = uv
        _apply(sc, P, V, first, p2, v2)
        ctx.update_geometry_async([D.VertexUpdate(first, p2, v2)], None, stream)
        orc.set_scene(_with(sc, positions=P.copy(), vertices=V.copy()))
        prm = D.frame_params(cfg, GRID, D.AppState(0), 0, **EXPOSURE)
        ctx.update(prm, stream)
        orc.update(prm)
        ctx.synchronize()
        got = [ctx.bake_read(w) for w in (abi.ARK_BAKE_TRIANGLE_INDEX, abi.ARK_BAKE_BARYCENTRICS, abi.ARK_BAKE_OUTPUT)]
        assert (got[0] > 0).mean() > 0.2
        for name, x, y in zip(("triangle index", "barycentrics", "output"), got, want):
            assert np.array_equal(x, y), name
        _compare(ctx, orc, "the frame after the second update")
    finally:
        ctx.close()
        orc.close()


def test_refusals_change_nothing():
    """A wrong struct_size, a range outside the pools, a NULL pointer pair, a non-finite host
    position, and missing or non-finite bounds with a device source are each refused with
    ARK_DDGI_E_INVALID_ARGUMENT, and the next frame equals the oracle's undeformed one."""
    import ctypes as C

    import torch

    sc = scenes.features_scene()
    cfg = _cfg(R=32, sun_bvh=_sun("light"))
    ctx = D.DDGIContext(GRID, 100.0, cfg)
    ctx.set_scene(sc)
    orc = O.Oracle(ctx.desc)
    orc.set_scene(sc)
    first, p, v = _wobble(sc, BOX, 1.0, amp=0.2)
    V = len(sc.positions)
    tp = torch.from_numpy(p).cuda()
    nan = p.copy()
    nan[3, 2] = np.float32("inf")

    class Raw(D.VertexUpdate):
        def __init__(self, *a, size=None, **kw):
            super().__init__(*a, **kw)
            self.size = size

        def to_abi(self):
            u = super().to_abi()
            if self.size is not None:
                u.struct_size = self.size
            return u

    empty = D.VertexUpdate(first)
    empty.vertex_count = len(p)
    cases = {
        "struct_size": Raw(first, p, v, size=C.sizeof(abi.ArkDdgiVertexUpdate) - 4),
        "range past the pools": D.VertexUpdate(V - len(p) + 1, p, v),
        "first vertex past the pools": D.VertexUpdate(V + 7, p, v),
        "no pointers": empty,
        "non-finite host position": D.VertexUpdate(first, nan, v),
        "device positions without bounds": D.VertexUpdate(first, tp),
        "device positions with non-finite bounds": D.VertexUpdate(first, tp, bounds=[0, 0, 0, 1, np.inf, 1]),
        "device positions with lo > hi": D.VertexUpdate(first, tp, bounds=[0, 2, 0, 1, 1, 1]),
    }
    try:
        idx = _frame(ctx, orc, cfg, GRID, 0, 0, "rest")
        digest = ctx.scene_digest()
        for f, (what, u) in enumerate(cases.items(), 1):
            with pytest.raises(abi.ArkDdgiError) as e:
                ctx.update_geometry([D.VertexUpdate(first, p, v), u])  # (the valid range ahead of it is not applied either)
            assert e.value.status == abi.ARK_DDGI_E_INVALID_ARGUMENT, what
            assert ctx.geometry_update_stats() == (0, 0, 0, 0), what
        bad = sc.instances.copy()
        bad["triangle_count"][0] -= 1
        with pytest.raises(abi.ArkDdgiError):
            ctx.update_geometry([D.VertexUpdate(first, p, v)], bad)
        assert ctx.scene_digest() == digest
        _frame(ctx, orc, cfg, GRID, 1, idx, "after the refusals")
    finally:
        ctx.close()
        orc.close()


def test_unused_feature_costs_nothing():
    """A context that never calls update_geometry holds none of its buffers and reports zero
    stats, also across set_instances; and a call without ranges is set_instances."""
    sc = scenes.features_scene()
    cfg = _cfg(R=32, sun_bvh=_sun("light"), background_rebuild=False)
    a = D.DDGIContext(GRID, 100.0, cfg)
    b = D.DDGIContext(GRID, 100.0, cfg)
    try:
        a.set_scene(sc)
        b.set_scene(sc)
        assert a.scene_digest() == b.scene_digest()
        inst = sc.instances.copy()
        M = inst["object_to_world"].reshape(-1, 3, 4).copy()
        M[BOX, :, 3] += np.float32(0.2)
        inst["object_to_world"] = M.reshape(len(inst), 12)
        a.set_instances(inst)
        a.update(D.frame_params(cfg, GRID, D.AppState(0), 0, **EXPOSURE))
        a.bake_ao(BOX, 8, 8, 2, False)
        a.synchronize()
        assert a.geometry_update_stats() == (0, 0, 0, 0)
        assert a.geometry_update_info() == dict(map_allocations=0, map_fills=0, device_bytes=0, position_updates=0)
        b.update_geometry([], inst)
        assert b.scene_digest() == a.scene_digest()
        assert b.geometry_update_stats() == (1, 0, 0, 0)
        assert b.geometry_update_info() == dict(map_allocations=0, map_fills=0, device_bytes=0, position_updates=0)
    finally:
        a.close()
        b.close()
