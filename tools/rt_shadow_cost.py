"""Cost of the ray-traced local-light shadow masks (ark_ddgi_rt_local_shadows) at
1920 x 1080 on C4 (10 M-triangle soup) and the C3 substitute, with 1 and 4 spot lights
and two depth planes: random depths (shading points scattered through the frustum) and an
analytic plane just above the bottom of the scene's bounding box (a floor).

    python tools/rt_shadow_cost.py [--config c3 c4] [--calls 50] [--reps 5]

Per (config, plane, lights): HIP events around `calls` calls ending in a synchronise, after
a warm-up - ms per call, listed shadow rays (counted by the host restatement over no
triangles: everything but the sky and the pixels outside the cone) and M rays/s. The same
call with every cone closed (cosine 2: every pixel culled, an empty ray list) costs what the
generator's first pass, an empty traversal launch and the resolve cost; the rest - the
traversal and the ray list's writes - is printed as its share.

Batch against single-light calls (the reference's shape, one traceRays per light): at 4
lights the two variants alternate in this process, `reps` repetitions of `calls` calls each;
the medians and the spread (max - min) of each variant are printed.

For context, the DDGI path's own shadow launch on C4: shadow rays of a counting update and
ark_ddgi_get_last_timings [4] of a timed one.
"""
import argparse
import json
import os
import statistics
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


def camera(eye, target, fov_y=1.0, near=0.1, far=100.0):
    """world_from_view / view_from_projection (column-major) of a right-handed look-at camera
    with a [0, 1]-depth perspective projection, and the 4 x 4 matrices themselves."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, (0.0, 1.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -view[:3, :3] @ eye
    t = 1.0 / np.tan(fov_y / 2)
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1] = t / (W / H), t
    proj[2, 2], proj[2, 3] = far / (near - far), far * near / (near - far)
    proj[3, 2] = -1.0
    col = lambda m: np.asarray(m, np.float32).T.reshape(16)  # noqa: E731
    return {"world_from_view": col(np.linalg.inv(view)), "view_from_projection": col(np.linalg.inv(proj))}, view, proj


def floor_depth(view, proj, y):
    """The depth plane of the horizontal plane at height y (1.0 where the pixel's ray misses it)."""
    ys, xs = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xs + 0.5) / W * 2 - 1, (ys + 0.5) / H * 2 - 1, np.full(xs.shape, 0.5), np.ones(xs.shape)], -1).reshape(-1, 4)
    inv = np.linalg.inv(proj @ view)
    p = ndc @ inv.T
    p = p[:, :3] / p[:, 3:]
    eye = np.linalg.inv(view)[:3, 3]
    d = p - eye
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (y - eye[1]) / d[:, 1]
    hit = np.isfinite(t) & (t > 0)
    X = eye + d * np.where(hit, t, 1.0)[:, None]
    clip = np.concatenate([X, np.ones((X.shape[0], 1))], 1) @ (proj @ view).T
    depth = np.where(hit, clip[:, 2] / clip[:, 3], 1.0)
    depth[(depth <= 0.0) | (depth >= 1.0)] = 1.0
    return depth.reshape(H, W).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["c3", "c4"])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from arkoserenderer_amd import ddgi as D

    torch.cuda.set_device(0)
    for name in args.config:
        sc, grid, R, zf = build(name)
        N = grid.probe_count()
        cfg = D.DDGIConfig(rays_per_probe=R, probe_updates_per_frame=N, max_rays_per_probe=R, max_probe_updates=N, compute_probe_offsets=True)
        ctx = D.DDGIContext(grid, zf, cfg)
        ctx.set_scene(sc)
        lo, hi = (np.asarray(v, np.float64) for v in sc.bounds())
        centre, ext = (lo + hi) / 2, hi - lo
        cam, view, proj = camera((centre[0], hi[1] + 0.25 * ext[1], hi[2] + 0.6 * ext[2]), (centre[0], lo[1] + 0.3 * ext[1], centre[2]), far=4.0 * float(ext.max()))
        rng = np.random.default_rng(5)
        random_depth = rng.uniform(0.95, 0.9995, (H, W)).astype(np.float32)
        random_depth[rng.random((H, W)) < 0.1] = 1.0
        planes = {"random": random_depth, "floor": floor_depth(view, proj, lo[1] + 0.01 * ext[1])}
        top = hi[1] + 0.2 * ext[1]
        spots = [D.RTShadowLight((lo[0] + fx * ext[0], top, lo[2] + fz * ext[2]), (0.0, -1.0, 0.0), 1.6, 0.025)
                 for fx, fz in ((0.26, 0.26), (0.52, 0.77), (0.77, 0.39), (0.39, 0.6))]
        masks = [torch.zeros((H, W), dtype=torch.uint8, device="cuda") for _ in spots]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def run(depth_dev, lights, calls, single=False, closed=False):
            """ms per frame (all lights): one batched call, or one call per light; closed: every cone cosine 2."""
            descs = ([D.rt_shadows_desc(W, H, cam, depth_dev.data_ptr(), [l], [masks[k].data_ptr()], 3) for k, l in enumerate(lights)] if single else
                     [D.rt_shadows_desc(W, H, cam, depth_dev.data_ptr(), lights, [m.data_ptr() for m in masks[:len(lights)]], 3)])
            for d in descs:
                for k in range(d.light_count if closed else 0):
                    d.lights[k].outer_cone_angle_cos = 2.0
            for _ in range(3):
                for d in descs:
                    ctx.rt_local_shadows(d)
            ctx.synchronize()
            ev[0].record()
            for _ in range(calls):
                for d in descs:
                    ctx.rt_local_shadows(d)
            ev[1].record()
            ctx.synchronize()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1]) / calls

        for pname, depth in planes.items():
            dev = torch.from_numpy(depth).cuda()
            for n in (1, 4):
                _, counts = D.rt_shadows_host(np.zeros((0, 12), np.uint32), np.zeros(0, np.int32), 1, W, H, cam, depth, spots[:n], 3)
                rays = sum(c["lit"] + c["occluded"] for c in counts)
                base = run(dev, spots[:n], args.calls, closed=True)
                ms = run(dev, spots[:n], args.calls)
                lit = sum(int((m == 255).sum().item()) for m in masks[:n])
                print(json.dumps({"config": name, "plane": pname, "lights": n, "ms_per_call": round(ms, 4), "shadow_rays": rays, "mrays_per_s": round(rays / ms / 1e3, 1),
                                  "ms_all_culled": round(base, 4), "traversal_and_list_share": round(max(0.0, 1.0 - base / ms), 3),
                                  "sky": counts[0]["sky"], "lit_bytes": lit}), flush=True)
            batch, single = [], []
            for _ in range(args.reps):
                batch.append(run(dev, spots, args.calls))
                single.append(run(dev, spots, args.calls, single=True))
            print(json.dumps({"config": name, "plane": pname, "lights": 4, "batch_ms": [round(v, 4) for v in batch], "single_calls_ms": [round(v, 4) for v in single],
                              "batch_median": round(statistics.median(batch), 4), "single_median": round(statistics.median(single), 4),
                              "batch_spread": round(max(batch) - min(batch), 4), "single_spread": round(max(single) - min(single), 4)}), flush=True)
        if name == "c4":
            p = D.frame_params(cfg, grid, D.AppState(0), 0, light_pre_exposure=1.0, ambient_illuminance=0.02, environment_brightness=1.0)
            ctx.set_counting(True)
            ctx.update(p)
            ctx.synchronize()
            shadow_rays = int(ctx.counters().shadow_rays)
            ctx.set_counting(False)
            ctx.set_timing(True)
            for f in range(1, 4):
                ctx.update(D.frame_params(cfg, grid, D.AppState(f), 0, light_pre_exposure=1.0, ambient_illuminance=0.02, environment_brightness=1.0))
                ctx.synchronize()
            t = ctx.last_timings()
            print(json.dumps({"config": name, "ddgi_step_shadow_rays": shadow_rays, "ddgi_step_shadow_launch_ms": round(t[4], 4),
                              "ddgi_step_mrays_per_s": round(shadow_rays / t[4] / 1e3, 1) if t[4] > 0 else None, "ddgi_step_ms": round(t[0], 4)}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
