"""Cost of the per-frame instance update (ark_ddgi_set_instances) at
C4 (10 M-triangle soup, 16 instances, 32^3 x 256) and the C3 substitute: the refit's
wall time and its device part (ArkDdgiBvhStats.refit_ms), and the update throughput
before and after - one instance moved by 0.5 m, then every instance rotated by 2 deg
about y (the refit keeps the topology, so the boxes loosen with the motion).

    python tools/refit_cost.py [--config c4 c3] [--steps 5]
    python tools/refit_cost.py --continuous [--frames 300] [--config c4 c3]

--continuous (VERDICT r05 "do this" #3): the static rate, then `frames` frames that each
move one instance (ark_ddgi_set_instances_async on the update's stream, no host wait)
- the rate under motion, the background rebuilds installed meanwhile - then static
frames until the rebuilds of the final state (world BVHs and the light-space sun BVH)
are installed, and the rate again: it should be back at the static rate.

--deform: --continuous with vertices instead of transforms (ark_ddgi_update_geometry_async):
the instance of the frame has its positions displaced by a sine of small amplitude (5 cm)
and the one of the frame before gets its rest positions back - the same instances dirty
as under --continuous, the same refit. The ranges carry the other vertex data too (as a
skinned mesh's normals change), unless --positions-only; --device-source hands the ranges
over as device tensors. The line also tells the vertices per call and the counts of
ark_ddgi_get_geometry_update_stats. Run --continuous and --deform in turn to compare.

--skin: --deform with the vertices produced on the device (ark_ddgi_skin_geometry_async): every
instance's range is a registered skin - four joints per vertex on a chain of 16 joints, all of
them the identity, and one morph target, the sine displacement - and the frame's call poses two
skins, the instance of the frame with morph weight 1 and the one of the frame before with
weight 0: the same ranges dirty as under --deform, the same refit, no vertex crossing the host
link. The line also tells k_skin_vertices' own time for the largest skin (HIP events around a
run on a stream of its own, ark_ddgi_debug_skin_device_parity) and the byte model's traffic.
--skin-host: the same poses skinned on the host (the serial restatement) and sent as host
ranges, which is what a caller without the device path does. Run --deform --device-source,
--skin and --skin-host in turn to compare.

--gpu-rebuild (with --continuous): ARK_DDGI_FLAG_GPU_REBUILD, the world BVHs rebuilt on the
device while the instances move. The line then also tells the installs' builder, the
device builds' time and footprint (nodes, records per triangle) as installed at the end
of the motion, and the traversal phase's device time (ark_ddgi_get_last_timings [1]) on
the tree traced at the start (set_scene's), right after the motion (the device build, or
with the flag off the refit-loosened one) and once settled (the host rebuild). Run it
with and without the flag in turn to compare.

--gpu-rebuild-sun (combines with --gpu-rebuild): ARK_DDGI_FLAG_GPU_REBUILD_SUN, the
light-space sun BVH rebuilt on the device too. The trees then also tell the sun BVH's
builder and device builds; with --sun-turn each turn records the shadow phase on the world
BVHs (while the build runs), on the device-built tree and on the host rebuild that settles
it, and the time from set_lights to each install.

--gpu-rebuild-sah (with either of the two): ARK_DDGI_FLAG_GPU_REBUILD_SAH, the device builds'
SAH pass over subtrees of at most 256 triangles. Run it with and without in turn: the device
builds' time (rebuild_ms, sun build_ms), the traversal and shadow phases on the tree traced
right after the motion, the footprint and the rate while moving are the ones to compare.

--gpu-rebuild-plan (with --gpu-rebuild-sah): ARK_DDGI_FLAG_GPU_REBUILD_PLAN, the SAH-optimal
collapse plan of those builds. Compare it the same way, against a run without it.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(name):
    from arkoserenderer_amd import ddgi as D
    from arkoserenderer_amd import scene as S
    if name == "c4":
        return S.soup(10_000_000), D.ProbeGrid((32, 32, 32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), 256, 10000.0
    return S.sponza_substitute(), D.ProbeGrid(*S.sponza_substitute_grid()), 256, 10000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["c4", "c3"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--continuous", action="store_true", help="one instance moved every frame for --frames frames, then back to static")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--deform", action="store_true", help="--continuous, the moved instance's positions displaced by a sine instead of translated (update_geometry)")
    ap.add_argument("--positions-only", action="store_true", help="with --deform: the ranges carry no other vertex data")
    ap.add_argument("--device-source", action="store_true", help="with --deform: the ranges are device tensors")
    ap.add_argument("--skin", action="store_true", help="--deform, the vertices skinned on the device from poses (skin_geometry)")
    ap.add_argument("--skin-host", action="store_true", help="--deform, the same poses skinned on the host and sent as host ranges")
    ap.add_argument("--no-background", action="store_true", help="ARK_DDGI_FLAG_NO_BACKGROUND_REBUILD: refits only (isolates the rebuild threads' cost)")
    ap.add_argument("--gpu-rebuild", action="store_true", help="ARK_DDGI_FLAG_GPU_REBUILD: the world BVHs' background rebuilds on the device")
    ap.add_argument("--gpu-rebuild-sun", action="store_true", help="ARK_DDGI_FLAG_GPU_REBUILD_SUN: the light-space sun BVH's background builds on the device")
    ap.add_argument("--gpu-rebuild-sah", action="store_true", help="ARK_DDGI_FLAG_GPU_REBUILD_SAH: the device builds' SAH pass over subtrees of at most 256 triangles")
    ap.add_argument("--gpu-rebuild-plan", action="store_true", help="ARK_DDGI_FLAG_GPU_REBUILD_PLAN: those builds collapse by the SAH-optimal plan")
    ap.add_argument("--sun-turn", action="store_true", help="instead of refits: turn the sun by 10 deg, wait for the background rebuild, turn it back, wait again")
    args = ap.parse_args()
    args.deform = args.deform or args.skin or args.skin_host
    args.continuous = args.continuous or args.deform
    import torch
    from arkoserenderer_amd import ddgi as D

    torch.cuda.set_device(0)
    for name in args.config:
        sc, grid, R, zf = build(name)
        N = grid.probe_count()
        cfg = D.DDGIConfig(rays_per_probe=R, probe_updates_per_frame=N, max_rays_per_probe=R, max_probe_updates=N, compute_probe_offsets=True,
                           background_rebuild=not args.no_background, gpu_rebuild=args.gpu_rebuild, gpu_rebuild_sun=args.gpu_rebuild_sun,
                           gpu_rebuild_sah=args.gpu_rebuild_sah, gpu_rebuild_plan=args.gpu_rebuild_plan)
        node = D.DDGINode(cfg)
        node.construct(sc, grid, zf, light_pre_exposure=1.0, ambient_illuminance=0.02, environment_brightness=1.0)
        app = [D.AppState(0)]

        def rate(nd=None):
            nd = nd or node
            for _ in range(2):
                nd.execute(app[0])
                app[0] = D.AppState(app[0].frame_index + 1)
            nd.ctx.synchronize()
            t = time.perf_counter()
            for _ in range(args.steps):
                nd.execute(app[0])
                app[0] = D.AppState(app[0].frame_index + 1)
            nd.ctx.synchronize()
            return N * R * args.steps / (time.perf_counter() - t) / 1e6

        def trace_ms(nd=None):
            """median device time of the traversal phase and of the shadow rays' launch over 5 timed frames"""
            nd = nd or node
            nd.ctx.set_timing(True)
            rows = []
            for _ in range(5):
                nd.execute(app[0])
                app[0] = D.AppState(app[0].frame_index + 1)
                nd.ctx.synchronize()
                rows.append(nd.ctx.last_timings())
            nd.ctx.set_timing(False)
            return {"traversal": round(float(np.median([r[1] for r in rows])), 4), "shadow": round(float(np.median([r[4] for r in rows])), 4)}

        def tree(st):
            return {"builder": "device" if st.bvh_installed_builder else "host", "rebuilds": int(st.bvh_rebuilds), "device_rebuilds": int(st.bvh_gpu_rebuilds),
                    "fallbacks": int(st.bvh_gpu_fallbacks), "failures": int(st.bvh_rebuild_failures), "rebuild_ms": round(st.bvh_rebuild_ms, 2),
                    "nodes": int(st.node_count), "records_per_triangle": round(st.triangle_bytes / 48 / max(1, sc.triangle_count), 4),
                    "built_refit_version": int(st.bvh_built_refit_version), "refit_version": int(st.refit_version),
                    "sun": {"builder": "device" if st.sun_installed_builder else "host", "rebuilds": int(st.sun_rebuilds), "device_rebuilds": int(st.sun_gpu_rebuilds),
                            "fallbacks": int(st.sun_gpu_fallbacks), "failures": int(st.sun_rebuild_failures), "build_ms": round(st.sun_build_ms, 2),
                            "nodes": int(st.sun_node_count), "built_refit_version": int(st.sun_built_refit_version)}}

        had_sun_bvh = node.ctx.bvh_stats().sun_node_count > 0
        out = {"config": name, "triangles": int(sc.triangle_count), "instances": int(sc.instances.size),
               "build_ms": round(node.ctx.bvh_stats().build_ms, 1), "mrays_per_s_static": round(rate(), 1)}
        if args.continuous:
            sptr = torch.cuda.current_stream().cuda_stream
            static = [out["mrays_per_s_static"], round(rate(), 1)]
            trees = {"start": {**tree(node.ctx.bvh_stats()), "ms": trace_ms()}}
            inst0 = sc.instances.copy()
            n = len(inst0)
            st0 = node.ctx.bvh_stats()
            node.ctx.synchronize()
            stream = torch.cuda.current_stream()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.frames)]
            host_refit = 0.0
            final = sc
            if args.deform:
                # every instance's range of the pools, at rest and deformed (prepared ahead:
                # the loop below times the calls, not numpy)
                inst = inst0
                poses = []
                for i in range(n):
                    mesh = sc.meshes[int(inst0["rt_mesh_index"][i])]
                    fi = int(mesh["first_index"])
                    first, cnt = int(mesh["first_vertex"]), int(sc.indices[fi:fi + 3 * int(inst0["triangle_count"][i])].max()) + 1
                    p0 = np.ascontiguousarray(sc.positions[first:first + cnt], np.float32)
                    p1 = (p0 + np.float32(0.05) * np.sin(np.float32(2.0) * p0[:, [1, 2, 0]])).astype(np.float32)
                    vx = None if args.positions_only else np.ascontiguousarray(sc.vertices[first:first + cnt]).view(np.float32).reshape(-1, 9)
                    lo, hi = np.minimum(p0.min(0), p1.min(0)), np.maximum(p0.max(0), p1.max(0))
                    if args.skin or args.skin_host:
                        rng = np.random.default_rng(i)
                        ji = rng.integers(0, 16, (cnt, 4)).astype(np.uint32)
                        jw = rng.uniform(0.1, 1.0, (cnt, 4))
                        jw = (jw / jw.sum(1, keepdims=True)).astype(np.float32)
                        morph = np.zeros((1, cnt, 9), np.float32)
                        morph[0, :, 0:3] = p1 - p0
                        skin = D.Skin(first, p0, np.ascontiguousarray(sc.vertices[first:first + cnt]), ji, jw, 16, morph)
                        handle = node.ctx.register_skin(skin) if args.skin else i
                        joints = np.tile(np.eye(4, dtype=np.float32), (16, 1, 1))
                        pair = [D.SkinPose(handle, joints, [w]) for w in (0.0, 1.0)]
                        poses.append((first, cnt, skin, pair))
                        continue
                    if args.device_source:
                        p0, p1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
                        vx = None if vx is None else torch.from_numpy(vx).cuda()
                    poses.append((first, cnt, p0, p1, vx, np.concatenate([lo, hi])))
                torch.cuda.synchronize()
                last = (args.frames - 1) % n
                P = sc.positions.copy()
                if args.skin or args.skin_host:
                    P[poses[last][0]:poses[last][0] + poses[last][1]] = D.skin_host(poses[last][2], poses[last][3][1])[0]
                else:
                    P[poses[last][0]:poses[last][0] + poses[last][1]] = poses[last][3].cpu().numpy() if args.device_source else poses[last][3]
                final = dataclasses.replace(sc, positions=P)
                per_call = 0
            t = time.perf_counter()
            for f in range(args.frames):
                if args.skin or args.skin_host:
                    call = [poses[f % n][3][1]] + ([poses[(f - 1) % n][3][0]] if f > 0 and n > 1 else [])
                    per_call = max(per_call, poses[f % n][1] + (poses[(f - 1) % n][1] if len(call) > 1 else 0))
                    ev[f][0].record(stream)
                    th = time.perf_counter()
                    if args.skin:
                        node.ctx.skin_geometry_async(call, None, sptr)
                    else:
                        ups = []
                        for q in call:
                            first, cnt, skin, _ = poses[q.skin]
                            p, v, _, _ = D.skin_host(skin, q)
                            ups.append(D.VertexUpdate(first, p, None if args.positions_only else v))
                        node.ctx.update_geometry_async(ups, None, sptr)
                    host_refit += time.perf_counter() - th
                    ev[f][1].record(stream)
                    node.execute(app[0], sptr)
                    app[0] = D.AppState(app[0].frame_index + 1)
                    continue
                if args.deform:
                    first, cnt, p0, p1, vx, box = poses[f % n]
                    ups = [D.VertexUpdate(first, p1, vx, bounds=box)]
                    if f > 0 and n > 1:
                        first, cnt, p0, p1, vx, box = poses[(f - 1) % n]
                        ups.append(D.VertexUpdate(first, p0, vx, bounds=box))
                    per_call = max(per_call, sum(u.vertex_count for u in ups))
                    ev[f][0].record(stream)
                    th = time.perf_counter()
                    node.ctx.update_geometry_async(ups, None, sptr)
                    host_refit += time.perf_counter() - th
                    ev[f][1].record(stream)
                    node.execute(app[0], sptr)
                    app[0] = D.AppState(app[0].frame_index + 1)
                    continue
                inst = inst0.copy()
                m = inst["object_to_world"].reshape(-1, 3, 4)
                m[f % n, 0, 3] += np.float32(0.3 * np.sin(0.1 * f))  # one instance a frame, back and forth
                m[(f // n) % n, 2, 3] += np.float32(0.2)               # and one left displaced for n frames
                inst["object_to_world"] = m.reshape(-1, 12)
                ev[f][0].record(stream)
                th = time.perf_counter()
                node.ctx.set_instances_async(inst, sptr)
                host_refit += time.perf_counter() - th
                ev[f][1].record(stream)
                node.execute(app[0], sptr)
                app[0] = D.AppState(app[0].frame_index + 1)
                if f % 50 == 49:
                    print(json.dumps({"frame": f + 1, "elapsed_s": round(time.perf_counter() - t, 2)}), flush=True)
            node.ctx.synchronize()
            motion_s = time.perf_counter() - t
            st1 = node.ctx.bvh_stats()
            refit_dev = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            # the tree a moving scene traces, before anything newer is installed
            trees["after_motion"] = {**tree(st1), "ms": trace_ms()}
            # static again: until BVHs built from the final records (after the last refit)
            # are installed - the world BVHs and the light-space sun BVH
            t = time.perf_counter()
            while time.perf_counter() - t < 120.0 and not args.no_background:
                st = node.ctx.bvh_stats()
                if st.bvh_built_refit_version == st.refit_version and (not had_sun_bvh or st.sun_built_refit_version == st.refit_version) and \
                        not st.bvh_installed_builder and not st.sun_installed_builder:  # (until the settle rebuilds have replaced the device builds)
                    break
                node.execute(app[0], sptr)
                app[0] = D.AppState(app[0].frame_index + 1)
                node.ctx.synchronize()
                time.sleep(0.01)
            settle_s = time.perf_counter() - t
            st2 = node.ctx.bvh_stats()
            trees["settled"] = {**tree(st2), "ms": trace_ms()}
            after = [round(rate(), 1) for _ in range(2)]
            # a context built from scratch on the final transforms, measured interleaved
            # with the rebuilt one: what "back at the static rate" means for the moved scene
            fresh_node = D.DDGINode(cfg)
            fresh_node.construct(dataclasses.replace(final, instances=inst), grid, zf, light_pre_exposure=1.0, ambient_illuminance=0.02, environment_brightness=1.0)
            fresh = []
            for _ in range(3):
                fresh.append(round(rate(fresh_node), 1))
                after.append(round(rate(), 1))
            fresh_node.ctx.close()
            out["continuous"] = {
                "frames": args.frames, "mrays_per_s_moving": round(N * R * args.frames / motion_s / 1e6, 1),
                "ms_per_frame_moving": round(motion_s / args.frames * 1e3, 4),
                "refit_device_ms": {"median": round(refit_dev[len(refit_dev) // 2], 4), "max": round(refit_dev[-1], 4)},
                "refit_host_enqueue_ms": round(host_refit / args.frames * 1e3, 4), "background_rebuild": not args.no_background,
                "gpu_rebuild": bool(args.gpu_rebuild), "gpu_rebuild_sun": bool(args.gpu_rebuild_sun), "gpu_rebuild_sah": bool(args.gpu_rebuild_sah), "gpu_rebuild_plan": bool(args.gpu_rebuild_plan),
                "trees": trees,
                "built_refit_version": {"world": int(st2.bvh_built_refit_version), "sun": int(st2.sun_built_refit_version), "refits": int(st2.refit_version)},
                "installs_while_moving": {"world": int(st1.bvh_rebuilds - st0.bvh_rebuilds), "sun": int(st1.sun_rebuilds - st0.sun_rebuilds)},
                "world_rebuild_ms": round(st2.bvh_rebuild_ms, 1), "sun_rebuild_ms": round(st2.sun_build_ms, 1),
                "settled_after_s": round(settle_s, 2), "sun_bvh_installed": bool(st2.sun_node_count > 0),
                "mrays_per_s_static_before": static, "mrays_per_s_static_after": after,
                "after_vs_before": round(max(after) / max(static), 4), "mrays_per_s_fresh_build": fresh,
                "after_vs_fresh": round(sorted(after)[len(after) // 2] / sorted(fresh)[1], 4)}
            if args.deform:
                out["continuous"]["deform"] = {"vertices_per_call": int(per_call), "positions_only": bool(args.positions_only), "device_source": bool(args.device_source),
                                               "stats": list(node.ctx.geometry_update_stats()), "info": node.ctx.geometry_update_info()}
            if args.skin or args.skin_host:
                out["continuous"]["deform"]["source"] = "skin" if args.skin else "skin-host"
            if args.skin:
                # the kernel alone, for the largest skin: bytes by ddgi_skinning.hip's model (K = 1, a previous position)
                first, cnt, skin, pair = max(poses, key=lambda q: q[1])
                prev = D.skin_host(skin, pair[0])[0]
                runs = sorted(D.skin_device_parity(skin, pair[1], prev)["kernel_ns"] for _ in range(5))
                model = cnt * (140 + 36 + 12)
                out["continuous"]["skin"] = {"stats": node.ctx.skin_stats(), "kernel_vertices": int(cnt), "kernel_us": [round(r / 1e3, 2) for r in runs],
                                             "model_bytes": int(model), "model_tb_per_s_at_median": round(model / runs[2] / 1e3, 3)}
            print(json.dumps(out), flush=True)
            node.ctx.close()
            continue
        if args.sun_turn:
            turns = []
            base = node.ctx.bvh_stats().sun_rebuilds
            d0 = np.array(sc.sun[1], np.float64)
            c, s_ = np.cos(np.radians(10.0)), np.sin(np.radians(10.0))
            d1 = np.array([c * d0[0] + s_ * d0[2], d0[1], -s_ * d0[0] + c * d0[2]])
            for label, d in (("turned", d1), ("back", d0)):
                t = time.perf_counter()
                node.ctx.set_lights((sc.sun[0], tuple(float(x) for x in d)), ())
                if args.gpu_rebuild_sun:
                    # each install since set_lights: the device build, then the host rebuild that settles it
                    turn = {"sun": label, "installs": []}
                    # (five timed frames at once: on the world BVHs unless the device build is installed within them)
                    turn["ms_world"] = trace_ms()
                    turn["installed_within_ms_world"] = bool(node.ctx.bvh_stats().sun_rebuilds != base)
                    while time.perf_counter() - t < 120.0:
                        node.execute(app[0])
                        app[0] = D.AppState(app[0].frame_index + 1)
                        node.ctx.synchronize()
                        st = node.ctx.bvh_stats()
                        if st.sun_rebuilds == base:
                            continue
                        base = st.sun_rebuilds
                        after_s = time.perf_counter() - t
                        turn["installs"].append({"builder": "device" if st.sun_installed_builder else "host", "installed_after_s": round(after_s, 3),
                                                 "build_ms": round(st.sun_build_ms, 1), "nodes": int(st.sun_node_count), "ms": trace_ms()})
                        if not st.sun_installed_builder:
                            break
                    turns.append(turn)
                    continue
                world = rate()  # the world BVHs carry the sun's rays meanwhile
                world_ms = trace_ms()
                while node.ctx.bvh_stats().sun_rebuilds == base and time.perf_counter() - t < 60.0:
                    node.execute(app[0])
                    app[0] = D.AppState(app[0].frame_index + 1)
                    node.ctx.synchronize()
                base = node.ctx.bvh_stats().sun_rebuilds
                turns.append({"sun": label, "mrays_per_s_world": round(world, 1), "ms_world": world_ms, "installed_after_s": round(time.perf_counter() - t, 2),
                              "rebuild_ms": round(node.ctx.bvh_stats().sun_build_ms, 1), "mrays_per_s_rebuilt": round(rate(), 1), "ms_rebuilt": trace_ms()})
            out["sun_turns"] = turns
            print(json.dumps(out), flush=True)
            node.ctx.close()
            continue
        inst = sc.instances.copy()
        moves = []
        inst["object_to_world"][0, 3] += 0.5
        c, s_ = np.cos(np.radians(2.0)), np.sin(np.radians(2.0))
        rot = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]], np.float32)
        for label in ("one_moved", "all_rotated"):
            if label == "all_rotated":
                m = inst["object_to_world"].reshape(-1, 3, 4)
                m[:] = np.einsum("ij,njk->nik", rot, m)
                inst["object_to_world"] = m.reshape(-1, 12)
            node.ctx.synchronize()
            t = time.perf_counter()
            node.ctx.set_instances(inst)
            wall = (time.perf_counter() - t) * 1e3
            st = node.ctx.bvh_stats()
            moves.append({"move": label, "set_instances_ms": round(wall, 2), "refit_ms": round(st.refit_ms, 2), "mrays_per_s": round(rate(), 1)})
        out["refits"] = moves
        # the light-space sun BVH, dropped by the refit, comes back from the background
        # rebuild (sceneSunStep): frames until it is installed, then the rate again
        st = node.ctx.bvh_stats()
        if had_sun_bvh:
            t = time.perf_counter()
            while node.ctx.bvh_stats().sun_rebuilds == st.sun_rebuilds and time.perf_counter() - t < 60.0:
                node.execute(app[0])
                app[0] = D.AppState(app[0].frame_index + 1)
                node.ctx.synchronize()
            s2 = node.ctx.bvh_stats()
            out["sun_rebuild"] = {"installed_after_s": round(time.perf_counter() - t, 2), "rebuild_ms": round(s2.sun_build_ms, 1),
                                  "sun_nodes": int(s2.sun_node_count), "mrays_per_s": round(rate(), 1)}
        print(json.dumps(out), flush=True)
        node.ctx.close()


if __name__ == "__main__":
    main()
