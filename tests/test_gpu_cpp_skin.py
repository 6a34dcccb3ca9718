"""The C++ path of a skeletal mesh instance: ddgi_headless --skin adds a tube to the scene
through GpuScene::addSkeletalMeshInstance (its bind pose an asset in the pools, the instance
with a target range of its own), poses it every frame through setJointMatrices /
setMorphTargetWeights, and the DDGINode registers the skin after its set_scene and sends the
newer poses in one ark_ddgi_skin_geometry_async. Its atlases and offsets equal, bit for bit,
those of the Python node given the same pools and poses through DDGIContext.skin_geometry."""
import os
import subprocess

import numpy as np
import pytest

from arkoserenderer_amd import abi
from arkoserenderer_amd import ddgi as D
from arkoserenderer_amd import scene as S
import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "arkoserenderer_amd", "bin", "ddgi_headless")


def _mirror(features, tube):
    """The pools as the C++ scene holds them: the features scene, the tube's bind pose as an
    asset nobody draws, then the skeletal instance's own copy of it, drawn by the last instance."""
    n, ni = len(tube.positions), tube.indices.size
    v0, i0 = len(features.positions), features.indices.size
    mesh = np.zeros(1, dtype=S.MESH_DTYPE)
    mesh["first_vertex"], mesh["first_index"], mesh["material_index"] = v0 + n, i0 + ni, len(features.materials)
    inst = tube.instances.copy()
    inst["rt_mesh_index"] = len(features.meshes)
    sc = S.SceneData(**{**features.__dict__,
                        "positions": np.concatenate([features.positions, tube.positions, tube.positions]),
                        "vertices": np.concatenate([features.vertices, tube.vertices, tube.vertices]),
                        "indices": np.concatenate([features.indices, tube.indices, tube.indices]),
                        "meshes": np.concatenate([features.meshes, mesh]), "materials": np.concatenate([features.materials, tube.materials]),
                        "instances": np.concatenate([features.instances, inst])})
    return sc, v0 + n


def test_headless_skin_matches_python(tmp_path):
    features = scenes.features_scene()
    tube, sk = S.skinned_tube(rings=14, segments=9, joints=4, morph_targets=2, base=(-0.5, 0.2, 0.9))
    grid = D.ProbeGrid((6, 4, 6), (0.7, 0.7, 0.7), (-1.75, 0.25, -1.75))
    cfg = D.DDGIConfig(rays_per_probe=64, probe_updates_per_frame=100, max_rays_per_probe=512, max_probe_updates=100)
    exposure = dict(light_pre_exposure=0.5, ambient_illuminance=0.1, environment_brightness=0.8)
    frames = 5
    poses = [(S.bend_pose(sk["joint_origins"], 0.07 * (f + 1), translate=(0.03 * f, 0.0, 0.0)), np.array([0.6 * np.sin(0.9 * f), 0.5 * np.cos(0.4 * f)], np.float32))
             for f in range(frames)]
    scene_path, skin_path, bind_path = (str(tmp_path / name) for name in ("features.arkscn", "tube.arkskin", "bind.arkskin"))
    features.save_binary(scene_path)
    S.save_skin_binary(skin_path, tube, sk, poses)
    S.save_skin_binary(bind_path, tube, sk, [])

    def headless(tag, skin):
        out = str(tmp_path / tag)
        cmd = [EXE, "--scene", scene_path, "--skin", skin, "--grid", "6", "4", "6", "--spacing", "0.7", "0.7", "0.7", "--origin", "-1.75", "0.25", "-1.75",
               "--rays", "64", "--updates", "100", "--frames", str(frames), "--zfar", "100", "--exposure", "0.5", "--env", "0.8",
               "--ambient", "0.1", "--offsets", "1", "--out", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return {k: np.fromfile(out + "." + k, dtype=dt) for k, dt in (("irr", np.uint16), ("vis", np.uint16), ("off", np.float32))}

    got = headless("posed", skin_path)
    bind = headless("bind", bind_path)
    sc, first = _mirror(features, tube)
    node = D.DDGINode(cfg)
    assert node.construct(sc, grid, 100.0, **exposure)
    try:
        h = node.ctx.register_skin(D.Skin(first, tube.positions, tube.vertices, sk["joint_indices"], sk["joint_weights"], sk["joint_count"], sk["morph_targets"]))
        for f in range(frames):
            node.ctx.skin_geometry([D.SkinPose(h, poses[f][0], poses[f][1])])
            node.execute(D.AppState(f))
        node.ctx.synchronize()
        want = {"irr": node.ctx.read(abi.ARK_DDGI_ATLAS_IRRADIANCE), "vis": node.ctx.read(abi.ARK_DDGI_ATLAS_VISIBILITY),
                "off": node.ctx.read(abi.ARK_DDGI_PROBE_OFFSETS)}
        assert node.ctx.skin_stats() == dict(calls=frames, vertices=frames * len(tube.positions), rejected=0, skins=1)
        assert node.ctx.geometry_update_stats()[2:] == (0, 0)
    finally:
        node.ctx.close()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(got["vis"], bind["vis"])  # (the poses are seen at all)
