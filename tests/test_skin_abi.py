"""The skinning entries' ABI surface: struct layouts in the ctypes mirror against the library,
the new symbols, the Skin / SkinPose helpers and the calls' answers on a null context, all
without a GPU. The checks that need a context - calls before a set_scene, argument errors of
register_skin and skin_geometry, a skin's lifetime across set_scene and unregister_skin - are
marked gpu: a context cannot be created without a device."""
import ctypes as C

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S

SYMBOLS = ("ark_ddgi_register_skin", "ark_ddgi_unregister_skin", "ark_ddgi_skin_geometry", "ark_ddgi_skin_geometry_async", "ark_ddgi_get_skin_views",
           "ark_ddgi_get_skin_stats", "ark_ddgi_debug_skin_host", "ark_ddgi_debug_skin_device_parity")
STRUCTS = {"ArkSkinningVertex": 32, "ArkMorphTargetVertex": 36, "ArkDdgiSkinDesc": 72, "ArkDdgiSkinPose": 32, "ArkDdgiSkinViews": 32}


def test_layouts_and_symbols():
    lib = abi.load_library()
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, f"libark_ddgi.so lacks {missing}"
    for name in SYMBOLS:
        assert name in abi.EXPORTS, name
    sizes = (C.c_uint32 * len(abi.ABI_STRUCTS))()
    assert lib.ark_ddgi_debug_struct_sizes(sizes, len(sizes)) == len(sizes)
    for name, size in STRUCTS.items():
        s = getattr(abi, name)
        assert C.sizeof(s) == size and sizes[abi.ABI_STRUCTS.index(s)] == size, name
    assert abi.ArkDdgiSkinDesc.positions.offset == 24 and abi.ArkDdgiSkinDesc.morph_targets.offset == 48
    assert abi.ArkDdgiSkinPose.joint_matrices.offset == 8 and abi.ArkDdgiSkinPose.morph_weights.offset == 16
    assert lib.ark_ddgi_abi_version() == 1


def test_calls_without_a_context():
    lib = abi.load_library()
    out = (C.c_uint64 * 4)()
    h = C.c_uint32()
    d, p, v = abi.ArkDdgiSkinDesc(), abi.ArkDdgiSkinPose(), abi.ArkDdgiSkinViews()
    assert lib.ark_ddgi_register_skin(None, C.byref(d), C.byref(h)) == abi.ARK_DDGI_E_INVALID_ARGUMENT
    assert lib.ark_ddgi_unregister_skin(None, 0) == abi.ARK_DDGI_E_INVALID_ARGUMENT
    assert lib.ark_ddgi_skin_geometry(None, C.byref(p), 1, None, 0) == abi.ARK_DDGI_E_INVALID_ARGUMENT
    assert lib.ark_ddgi_skin_geometry_async(None, C.byref(p), 1, None, 0, None) == abi.ARK_DDGI_E_INVALID_ARGUMENT
    assert lib.ark_ddgi_get_skin_views(None, 0, C.byref(v)) == abi.ARK_DDGI_E_INVALID_ARGUMENT
    assert lib.ark_ddgi_get_skin_stats(None, out) == abi.ARK_DDGI_E_INVALID_ARGUMENT
    # the host restatement refuses a desc of the wrong size and null outputs
    assert lib.ark_ddgi_debug_skin_host(C.byref(d), C.byref(p), None, None, None, None, None) == abi.ARK_DDGI_E_INVALID_ARGUMENT


def test_helpers():
    sc, sk = S.skinned_tube(rings=5, segments=6, joints=3, morph_targets=2)
    n = 30
    assert sc.positions.shape == (n, 3) and sk["joint_indices"].shape == (n, 4) and sk["morph_targets"].shape == (2, n, 9)
    assert np.allclose(sk["joint_weights"].sum(1), 1.0) and sk["joint_indices"].max() == 2 and (sk["joint_weights"] >= 0).all()
    assert int(sc.indices.max()) == n - 1 and sc.instances["triangle_count"][0] == 2 * 6 * 4
    skin = D.Skin(11, sc.positions, sc.vertices, sk["joint_indices"], sk["joint_weights"], 3, sk["morph_targets"])
    d = skin.to_abi()
    assert (d.struct_size, d.first_vertex, d.vertex_count, d.joint_count, d.morph_target_count) == (72, 11, n, 3, 2)
    assert d.positions and d.vertices and d.skinning and d.morph_targets
    row = np.ctypeslib.as_array(C.cast(d.skinning, C.POINTER(C.c_uint32)), (n * 8,)).reshape(n, 8)
    assert np.array_equal(row[:, :4], sk["joint_indices"]) and np.array_equal(row[:, 4:].view(np.float32), sk["joint_weights"])
    m = D.Skin(0, sc.positions, sc.vertices, morph_targets=sk["morph_targets"]).to_abi()
    assert not m.skinning and m.joint_count == 0 and m.morph_target_count == 2
    with pytest.raises(ValueError):
        D.Skin(0, sc.positions, sc.vertices[:5])
    with pytest.raises(ValueError):
        D.Skin(0, sc.positions, sc.vertices, sk["joint_indices"], None)
    M = S.bend_pose(sk["joint_origins"], 0.3, translate=(1.0, 2.0, 3.0))
    assert M.shape == (3, 4, 4) and np.allclose(M[0, 3, :3], [1.0, 2.0, 3.0] + (np.eye(3) - M[0, :3, :3].T) @ sk["joint_origins"][0])  # column-major
    p = D.SkinPose(4, M, [0.5, 0.25]).to_abi()
    assert (p.struct_size, p.skin) == (32, 4) and p.joint_matrices and p.morph_weights
    assert not D.SkinPose(0).to_abi().joint_matrices


GRID = D.ProbeGrid((2, 2, 2), (1.0, 1.0, 1.0), (-0.5, 0.2, -0.5))


def _ctx():
    return D.DDGIContext(GRID, 100.0, D.DDGIConfig(rays_per_probe=32, probe_updates_per_frame=8, max_rays_per_probe=32, max_probe_updates=8))


@pytest.mark.gpu
def test_argument_errors_and_lifetime():
    sc, sk = S.skinned_tube(rings=6, segments=6, joints=3, morph_targets=1)
    n = len(sc.positions)
    skin = D.Skin(0, sc.positions, sc.vertices, sk["joint_indices"], sk["joint_weights"], 3, sk["morph_targets"])
    pose = D.SkinPose(0, S.bend_pose(sk["joint_origins"], 0.2), [0.3])
    ctx = _ctx()
    try:
        for call in (lambda: ctx.register_skin(skin), lambda: ctx.skin_geometry([pose]), lambda: ctx.unregister_skin(0), lambda: ctx.skin_views(0)):
            with pytest.raises(abi.ArkDdgiError) as e:
                call()
            assert e.value.status == abi.ARK_DDGI_E_NO_SCENE
        assert ctx.skin_stats() == dict(calls=0, vertices=0, rejected=0, skins=0)
        ctx.set_scene(sc)
        # a scene without a skin holds nothing for them
        with pytest.raises(abi.ArkDdgiError):
            ctx.skin_geometry([pose])
        assert ctx.skin_stats() == dict(calls=0, vertices=0, rejected=0, skins=0) and ctx.geometry_update_info()["device_bytes"] == 0
        # registration's refusals leave the registry as it was
        ji = sk["joint_indices"].copy()
        ji[3, 1] = 3
        jw = sk["joint_weights"].copy()
        jw[2, 0] = np.nan
        for bad in (D.Skin(1, sc.positions, sc.vertices, sk["joint_indices"], sk["joint_weights"], 3),  # past the pools' end
                    D.Skin(0, sc.positions, sc.vertices, ji, sk["joint_weights"], 3), D.Skin(0, sc.positions, sc.vertices, sk["joint_indices"], jw, 3),
                    D.Skin(0, sc.positions, sc.vertices)):
            with pytest.raises(abi.ArkDdgiError) as e:
                ctx.register_skin(bad)
            assert e.value.status == abi.ARK_DDGI_E_INVALID_ARGUMENT
        d = skin.to_abi()
        d.struct_size = 8
        assert ctx.lib.ark_ddgi_register_skin(ctx.h, C.byref(d), C.byref(C.c_uint32())) == abi.ARK_DDGI_E_INVALID_ARGUMENT
        assert ctx.skin_stats()["skins"] == 0
        h = ctx.register_skin(skin)
        assert h == 0 and ctx.skin_stats()["skins"] == 1 and ctx.skin_views(h).runs == 0 and not ctx.skin_views(h).positions
        # skin_geometry's refusals enqueue nothing and are counted
        bad_m = S.bend_pose(sk["joint_origins"], 0.2)
        bad_m[1, 2, 2] = np.inf
        for poses in ([D.SkinPose(h, bad_m, [0.3])], [D.SkinPose(h, pose.joint_matrices, [np.nan])], [D.SkinPose(5, pose.joint_matrices, [0.3])], [pose, pose],
                      [D.SkinPose(h, None, [0.3])]):
            with pytest.raises(abi.ArkDdgiError) as e:
                ctx.skin_geometry(poses)
            assert e.value.status == abi.ARK_DDGI_E_INVALID_ARGUMENT
        assert ctx.skin_stats() == dict(calls=0, vertices=0, rejected=5, skins=1) and ctx.geometry_update_stats() == (0, 0, 0, 0)
        ctx.skin_geometry([pose])
        v = ctx.skin_views(h)
        assert v.runs == 1 and v.vertex_count == n and v.positions and v.vertices and v.velocities
        assert ctx.skin_stats() == dict(calls=1, vertices=n, rejected=5, skins=1) and ctx.geometry_update_stats() == (1, n, 0, 0)
        ctx.unregister_skin(h)
        with pytest.raises(abi.ArkDdgiError):
            ctx.skin_geometry([pose])
        with pytest.raises(abi.ArkDdgiError):
            ctx.unregister_skin(h)
        h2 = ctx.register_skin(skin)
        assert h2 != h and ctx.skin_stats()["skins"] == 1
        # a new set_scene drops every skin
        ctx.set_scene(sc)
        assert ctx.skin_stats() == dict(calls=0, vertices=0, rejected=0, skins=0)
        with pytest.raises(abi.ArkDdgiError):
            ctx.skin_geometry([D.SkinPose(h2, pose.joint_matrices, [0.3])])
    finally:
        ctx.close()
