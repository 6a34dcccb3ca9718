"""Cost of the path tracer (ark_ddgi_path_trace) at 1920 x 1080 on C4 (10 M-triangle soup) and
the C3 substitute.

    python tools/path_tracer_cost.py [--config c3 c4] [--calls 10]

Per config, with the scene's sun and at most one spot light (so that a 1080p frame's lists fit
one batch of the 512 MiB budget and the device's list counts are the whole frame's):
HIP events around `calls` frames ending in a synchronise, after a warm-up - ms per frame; the
live paths and the listed shadow rays of each of the 16 segments from the counts the last frame
left on the device; M ray segments/s and M shadow rays/s over the whole frame time (every stage
included). The same camera turned away from the scene (every pixel sky: the list is empty after
segment 0) costs what 16 segments of launches on empty lists cost: the fixed price of not
waiting on the host. The frame index changes from frame to frame, as a node's would. Last, as
context: the first segment alone (setup, one traversal, hit stage, shadow traversal, shading)
next to ark_ddgi_rt_reflections on the same scene and camera over a random-depth G-buffer.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080


def build(name):
    from arkoserenderer_amd import ddgi as D
    from arkoserenderer_amd import scene as S
    if name == "c4":
        return S.soup(10_000_000), D.ProbeGrid((32, 32, 32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), 256, 10000.0
    return S.sponza_substitute(), D.ProbeGrid(*S.sponza_substitute_grid()), 256, 10000.0


def camera(eye, target, far, fov_y=1.0, near=0.1):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, (0.0, 1.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    wv = np.eye(4)
    wv[:3, 0], wv[:3, 1], wv[:3, 2], wv[:3, 3] = s, u, -f, eye
    t = 1.0 / np.tan(fov_y / 2)
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1] = t / (W / H), t
    proj[2, 2], proj[2, 3] = far / (near - far), far * near / (near - far)
    proj[3, 2] = -1.0
    col = lambda m: np.asarray(m, np.float32).T.reshape(16)  # noqa: E731
    return {"world_from_view": col(wv), "view_from_projection": col(np.linalg.inv(proj)), "z_near": near, "z_far": far}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["c3", "c4"])
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    from arkoserenderer_amd import ddgi as D

    torch.cuda.set_device(0)
    for name in args.config:
        sc, grid, R, zf = build(name)
        cfg = D.DDGIConfig(rays_per_probe=R, probe_updates_per_frame=4096, max_rays_per_probe=R, max_probe_updates=4096)
        ctx = D.DDGIContext(grid, zf, cfg)
        ctx.set_scene(sc)
        ctx.set_lights(sc.sun, sc.spots[:1])
        lights = (1 if sc.sun is not None else 0) + len(sc.spots[:1])
        lo, hi = (np.asarray(v, np.float64) for v in sc.bounds())
        centre, ext = (lo + hi) / 2, hi - lo
        far = 4.0 * float(ext.max())
        eye = (centre[0], hi[1] + 0.25 * ext[1], hi[2] + 0.6 * ext[2])
        cams = {"scene": camera(eye, (centre[0], lo[1] + 0.3 * ext[1], centre[2]), far), "all_sky": camera(eye, (eye[0], eye[1] + ext[1], eye[2] + 2.0 * ext[2]), far)}
        image = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run(cam, calls):
            for f in range(2):
                ctx.path_trace(D.path_tracer_desc(W, H, cam, image.data_ptr(), None, 0, f, 0, 1.0))
            ctx.synchronize()
            ev[0].record()
            for f in range(calls):
                ctx.path_trace(D.path_tracer_desc(W, H, cam, image.data_ptr(), None, 0, 2 + f, 0, 1.0))
            ev[1].record()
            ctx.synchronize()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) / calls

        for cname, cam in cams.items():
            ms = run(cam, args.calls)
            paths, shadows = D.path_tracer_last_counts(ctx)
            img = image.float()
            print(json.dumps({"config": name, "camera": cname, "lights": lights, "triangles": sc.triangle_count, "ms_per_frame": round(ms, 4), "live_paths_per_segment": paths,
                              "shadow_rays_per_segment": shadows, "ray_segments": sum(paths), "shadow_rays": sum(shadows),
                              "msegments_per_s": round(sum(paths) / ms / 1e3, 1), "mshadow_rays_per_s": round(sum(shadows) / ms / 1e3, 1),
                              "mean_radiance": round(float(img[..., :3].nan_to_num(0.0, 0.0, 0.0).mean().item()), 5),
                              "nan_texels": int(torch.isnan(img[..., :3]).any(-1).sum().item())}), flush=True)
        # the first segment alone (the debug segment limit: timing only) next to ark_ddgi_rt_reflections on
        # the same scene and camera: a G-buffer of random depths in [0.95, 0.9995] with a tenth sky, normals
        # facing the viewer, roughness 0.2, so nine tenths of the pixels trace one reflection ray
        ctx.check(ctx.lib.ark_ddgi_debug_path_tracer_set_segments(ctx.h, 1), "set_segments")
        first = run(cams["scene"], args.calls)
        paths1, shadows1 = D.path_tracer_last_counts(ctx)
        ctx.check(ctx.lib.ark_ddgi_debug_path_tracer_set_segments(ctx.h, 16), "set_segments")
        rng = np.random.default_rng(5)
        depth = rng.uniform(0.95, 0.9995, (H, W)).astype(np.float32)
        depth[rng.random((H, W)) < 0.1] = 1.0
        material = np.zeros((H, W, 4), np.uint8)
        material[..., 0] = 51
        g = {"depth": torch.from_numpy(depth).cuda(), "material": torch.from_numpy(material).cuda(), "normal_velocity": torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"),
             "out_radiance": torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"), "out_direction": torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")}
        rd = D.reflections_desc(W, H, cams["scene"], {k: v.data_ptr() for k, v in g.items()}, environment_multiplier=1.0)
        for _ in range(2):
            ctx.rt_reflections(rd)
        ctx.synchronize()
        ev[0].record()
        for _ in range(args.calls):
            ctx.rt_reflections(rd)
        ev[1].record()
        ctx.synchronize()
        ev[1].synchronize()
        refl_ms = ev[0].elapsed_time(ev[1]) / args.calls
        print(json.dumps({"config": name, "camera": "scene", "first_segment_ms": round(first, 4), "first_segment_paths": paths1[0], "first_segment_shadow_rays": shadows1[0],
                          "rt_reflections_ms": round(refl_ms, 4), "rt_reflections_rays": int((depth < 1.0 - 1e-6).sum())}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
