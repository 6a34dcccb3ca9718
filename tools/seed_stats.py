"""The probe rays' hit candidates (csrc/seed_cache.h) without a GPU: what a per-probe
direction -> last-hit cache of T x T texels saves k_trace, through the host simulator's dual
step (tools/sim, ark_ddgi_debug_bvh8_trace_seeded).

Rays: a sample of probes of the G^3 grid over the soup, R rays each, a spherical Fibonacci set
under a fresh random rotation per probe and update (what the probe rays are: the exact
rotations of the updates do not matter here, only that they differ from update to update).
For every T and every number of fill updates F the cache is filled by F updates and read by
the next; the row reports that last update: rays holding a candidate, candidates hit, node
visits, triangle tests (the candidates' tests included) and dual-step iterations per ray,
against the same rays traced without a cache.

    python tools/seed_stats.py [--triangles N] [--grid G] [--probes P] [--rays R] [--texels 8 16 24] [--fill 1 3 8] [--threads T]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tools", "sim"))

from bvh_stats import world_triangles  # noqa: E402


def fibonacci_sphere(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = 2.0 * np.pi * i / ((1.0 + 5.0 ** 0.5) / 2.0)
    z = 1.0 - 2.0 * i / n
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([np.cos(phi) * s, np.sin(phi) * s, z], axis=1)


def random_rotations(rng, n):
    """n uniformly random rotation matrices (unit quaternions)."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def probe_rays(origins, rays_per_probe, frames, tmax, seed=5):
    """[frames][probes x R][7] rays (origin, direction, tmax) and the cache row of each ray of a frame."""
    rng = np.random.default_rng(seed)
    fib = fibonacci_sphere(rays_per_probe)
    P = len(origins)
    out = np.zeros((frames, P * rays_per_probe, 7), np.float32)
    for f in range(frames):
        rot = random_rotations(rng, P)
        d = np.einsum("pij,rj->pri", rot, fib)
        out[f, :, 0:3] = np.repeat(np.asarray(origins, np.float32), rays_per_probe, axis=0)
        out[f, :, 3:6] = d.reshape(-1, 3)
        out[f, :, 6] = tmax
    return out, np.repeat(np.arange(P, dtype=np.uint32), rays_per_probe)


def trace(sim, tris, rays, probe_of, probes, texels, threads, candidates=None):
    """One run of the seeded simulator: per-frame stats [frames][8], hit records and distances."""
    frames, n = rays.shape[0], rays.shape[1]
    rays = np.ascontiguousarray(rays, np.float32)
    out = (C.c_uint64 * 9)()
    frame_out = np.zeros((frames, 8), np.uint64)
    hit = np.zeros((frames, n), np.uint32)
    hit_t = np.zeros((frames, n), np.float32)
    cand = None if candidates is None else np.ascontiguousarray(candidates, np.uint32)
    rc = sim.ark_ddgi_debug_bvh8_trace_seeded(tris.ctypes.data, tris.shape[0], rays.ctypes.data, n, frames, probe_of.ctypes.data, probes, texels,
                                              None if cand is None else cand.ctypes.data, threads, out, frame_out.ctypes.data, hit.ctypes.data,
                                              hit_t.ctypes.data, None)
    if rc != 0:
        raise RuntimeError(f"ark_ddgi_debug_bvh8_trace_seeded: {rc}")
    return frame_out, hit, hit_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=10_000_000)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--probes", type=int, default=96)
    ap.add_argument("--rays", type=int, default=256)
    ap.add_argument("--texels", type=int, nargs="+", default=[8, 12, 16, 24, 32])
    ap.add_argument("--fill", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    from arkoserenderer_amd import scene as S
    import bvhsim

    sim = bvhsim.load()
    tris = world_triangles(S.soup(args.triangles))
    G = args.grid
    rng = np.random.default_rng(5)
    idx = rng.choice(G ** 3, args.probes, replace=False)
    origins = np.stack([idx % G, idx // (G * G), (idx // G) % G], axis=1).astype(np.float32)
    frames = max(args.fill) + 1
    rays, probe_of = probe_rays(origins, args.rays, frames, 10000.0)
    n = rays.shape[1]

    def row(fo):
        return {"nodes": round(int(fo[0]) / n, 2), "tris": round(int(fo[1]) / n, 2), "iterations": round(int(fo[3]) / n, 2),
                "holding": round(int(fo[4]) / n, 3), "candidate_hit": round(int(fo[5]) / max(1, int(fo[4])), 3)}

    base, base_hit, _ = trace(sim, tris, rays, probe_of, args.probes, 0, args.threads)
    print("none", json.dumps(row(base[-1])), flush=True)
    for T in args.texels:
        for F in args.fill:
            # the last F + 1 updates: F fill the cache, the last one (the same rays as the base row's) reads it
            fo, hit, _ = trace(sim, tris, rays[frames - 1 - F:], probe_of, args.probes, T, args.threads)
            assert np.array_equal(hit[-1], base_hit[-1]), "the candidates changed a closest hit"
            r = row(fo[-1])
            r["vs_none_iterations"] = round(int(fo[-1][3]) / int(base[-1][3]) - 1.0, 4)
            print(f"{T}x{T} fill {F}", json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
