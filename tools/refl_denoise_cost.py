"""Cost of the reflection denoiser passes (ark_ddgi_rt_reflections_denoise) at 1920 x 1080 on
the three-frame moving-camera sequence of tests/refl_denoise_inputs.py (the bench's G-buffer
generator, tests/reflection_inputs.py, under a translated and rotated camera).

    python tools/refl_denoise_cost.py [--calls 200] [--reps 5]

The planes first go through the sequence once (a first frame and two more), so that the timed
frame reprojects real history. Then, per pass and for the whole call: a warm-up, and `reps`
windows of `calls` launches between two HIP events ending in a synchronise; the median and the
spread (max - min) of the windows are printed, next to the pass's plane-byte floor: the bytes
it must read and write once (every plane it touches, per pixel; reproject's partial stores
counted whole) over 6.3 TB/s, the streaming bandwidth measured on this part. A pass repeated
on the same planes finds them in the 256 MiB last-level cache where they fit, so a time under
the floor of HBM is possible; the whole call (166 MB of planes at 1080p) is the fair figure.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
STREAM_TBPS = 6.3
# bytes per pixel read + written once: RGBA16F 8, R32F / depth / material 4, the average plane 8 / 64
PASSES = [
    ("historyCopy(first)", 0, 8 + 8 + 4 + 4 + 3 * 8),
    ("reproject", 1, 8 + 8 + 4 + 4 + 3 * 8 + 8 + 4 + 4 + 8 / 64),
    ("prefilter", 2, 8 + 4 + 8 + 4 + 4 + 8 / 64 + 8),
    ("resolveTemporal", 3, 8 + 4 + 4 + 4 + 8 + 8 / 64 + 8),
    ("historyCopy", 4, 8 + 8 + 4 + 4 + 4 + 4 + 3 * 8),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from arkoserenderer_amd import ddgi as D
    import refl_denoise_inputs as I

    torch.cuda.set_device(0)
    grid = D.ProbeGrid((4, 4, 4), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    ctx = D.DDGIContext(grid, 100.0, D.DDGIConfig(rays_per_probe=16, probe_updates_per_frame=64, max_rays_per_probe=16, max_probe_updates=64))
    seq = I.sequence(W, H)
    dev = lambda planes: {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int16) if v.dtype == np.uint16 else np.ascontiguousarray(v)).cuda() for k, v in planes.items()}  # noqa: E731
    state = dev(I.fresh_planes(W, H))
    descs = []
    for f, (cam, planes) in enumerate(seq):
        d_in = dev(planes)
        addr = {k: t.data_ptr() for k, t in {**d_in, **state}.items()}
        descs.append((D.refl_denoise_desc(W, H, cam, addr, I.frame_flags(f)), d_in))
        ctx.rt_reflections_denoise(descs[-1][0])
    ctx.synchronize()
    desc = descs[2][0]
    glossy = float(I.glossy(seq[2][1]).mean())
    kept = float((state["num_samples"].cpu().numpy()[I.glossy(seq[2][1])] > 1).mean())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def window(fn):
        for _ in range(10):
            fn()
        ctx.synchronize()
        out = []
        for _ in range(args.reps):
            ev[0].record()
            for _ in range(args.calls):
                fn()
            ev[1].record()
            ctx.synchronize()
            ev[1].synchronize()
            out.append(ev[0].elapsed_time(ev[1]) / args.calls)
        return out

    print(json.dumps({"width": W, "height": H, "glossy_fraction": round(glossy, 3), "history_kept_fraction_of_glossy": round(kept, 3), "calls": args.calls, "reps": args.reps,
                      "streaming_tb_per_s": STREAM_TBPS}), flush=True)
    total_floor = 0.0
    for name, p, bpp in PASSES:
        ms = window(lambda p=p: ctx.check(ctx.lib.ark_ddgi_debug_refl_denoise_pass(ctx.h, C.byref(desc), p, None), "ark_ddgi_debug_refl_denoise_pass"))
        floor = bpp * W * H / (STREAM_TBPS * 1e12) * 1e3
        total_floor += floor if p else 0.0
        print(json.dumps({"pass": name, "ms_median": round(statistics.median(ms), 4), "ms_spread": round(max(ms) - min(ms), 4), "bytes_per_pixel": round(bpp, 3),
                          "floor_ms": round(floor, 4), "times_floor": round(statistics.median(ms) / floor, 1)}), flush=True)
    ms = window(lambda: ctx.rt_reflections_denoise(desc))
    print(json.dumps({"pass": "whole call (reproject, prefilter, resolveTemporal, historyCopy)", "ms_median": round(statistics.median(ms), 4), "ms_spread": round(max(ms) - min(ms), 4),
                      "floor_ms": round(total_floor, 4), "times_floor": round(statistics.median(ms) / total_floor, 1)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
