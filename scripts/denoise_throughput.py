#!/usr/bin/env python3
"""rt_denoise on the C2 frame (bench.py: the Cornell box, 800 x 800, depth 50), fp32 and fp64.

1. Time: ms per call at --iterations passes, device pointers, HIP events around each call, the median of --reps calls
   after --warmup, with var and without. Beside it the traffic model: a pass reads two records a pixel (colour,
   guide) and writes one, npix x (2 + 1) records of 16 B (fp32) or 32 B (fp64); "model_gb_s" is that model's bytes
   over the measured time, not a measured bandwidth (the 25 taps of a pass are served by the caches).
2. Quality: MSE against a --ref-spp render for each of --spps, the noisy image (rt_render_adaptive with threshold 0:
   every pixel with variance takes max_spp = spp samples, and the call returns the noise map) and the denoised one,
   with var = adaptive_variance and without var (sigma_color = --sigma-novar, an absolute colour distance then). "off
   the light": the same over the pixels whose albedo is at most 1, which leaves out the emitter (radiance 15), whose
   aliased edge dominates the frame's MSE and which no spatial filter repairs.

One JSON line per row is printed and appended to --out.

  python scripts/denoise_throughput.py [--width W] [--iterations K] [--spps a,b,c] [--ref-spp S]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "python"))

import torch  # noqa: E402

import rt_amd  # noqa: E402
from rt_amd import abi, scenes  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--spps", default="16,64,256")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--sigma-novar", type=float, default=0.3)
    ap.add_argument("--floor", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_throughput.jsonl"))
    a = ap.parse_args()
    desc, cam, _, _ = scenes.cornell_box(width=a.width)
    ctx = rt_amd.Context(0)
    ctx.upload(desc)
    H, W = cam.image_height, cam.image_width
    npix = W * H
    base = {"scene": "cornell_box", "width": W, "height": H, "depth": a.depth, "iterations": a.iterations}
    with open(a.out, "a") as log:
        def emit(row):
            line = json.dumps(dict(base, **row))
            print(line, flush=True)
            log.write(line + "\n")

        spps = [int(s) for s in a.spps.split(",")]
        # ---- the inputs, on the device: the frames at each spp with their noise maps, the guides, the reference
        truth = torch.from_numpy(ctx.render(cam, a.ref_spp, a.depth, seed=1001, precision=abi.RT_PREC_F32)).cuda().double()
        frames = {}
        for spp in spps:
            noisy = ctx.render_adaptive(cam, spp, a.depth, 0.0, batch=4, min_spp=spp // 2, step_spp=spp // 2,
                                        floor=a.floor, seed=1, precision=abi.RT_PREC_F32, device=True)
            aov = ctx.render_aov(cam, spp, seed=1, precision=abi.RT_PREC_F32, device=True)
            feat = torch.cat([aov["albedo"].reshape(npix, 3), aov["normal"].reshape(npix, 3),
                              aov["depth"].reshape(npix, 1), aov["hit"].reshape(npix, 1)], 1).contiguous()
            frames[spp] = (noisy["rgb"].contiguous(), feat, rt_amd.adaptive_variance(noisy, a.floor).contiguous())
        torch.cuda.synchronize()

        # ---- 1. time
        rgb32, feat, var = frames[spps[0]]
        for pname, rgb, rec in (("f32", rgb32, 16), ("f64", rgb32.double(), 32)):
            for what, v in (("var", var), ("novar", None)):
                t = timed(lambda: ctx.denoise(rgb, feat, v, iterations=a.iterations), a.warmup, a.reps)
                ms = float(np.median(t))
                model = npix * 3 * rec * a.iterations
                emit({"row": "time", "precision": pname, "guide": what, "ms": ms,
                      "spread_ms": [float(t.min()), float(t.max())], "model_bytes": model,
                      "model_gb_s": model / ms / 1e6, "mpix_s": npix / ms / 1e3})

        # ---- 2. quality
        def mse(img, mask=None):
            d = ((img.double() - truth) ** 2).mean(-1)
            return float(d.mean() if mask is None else d[mask].mean())

        for spp in spps:
            rgb, feat, var = frames[spp]
            off = (feat[:, 0:3].max(1).values <= 1.0).reshape(H, W)
            with_var = ctx.denoise(rgb, feat, var, iterations=a.iterations)
            without = ctx.denoise(rgb, feat, None, iterations=a.iterations, sigma_color=a.sigma_novar)
            torch.cuda.synchronize()
            emit({"row": "quality", "precision": "f32", "spp": spp, "ref_spp": a.ref_spp,
                  "sigma_color_novar": a.sigma_novar,
                  "mse_noisy": mse(rgb), "mse_var": mse(with_var), "mse_novar": mse(without),
                  "mse_noisy_off_light": mse(rgb, off), "mse_var_off_light": mse(with_var, off),
                  "mse_novar_off_light": mse(without, off)})
    ctx.close()


if __name__ == "__main__":
    main()
