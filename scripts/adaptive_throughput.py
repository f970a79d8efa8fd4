#!/usr/bin/env python3
"""rt_render_adaptive beside rt_render_tiles on the C2 scene (bench.py: the Cornell box, 800 x 800, depth 50), fp32
and fp64: the frame at --spp samples a pixel through rt_render_tiles, then rt_render_adaptive with max_spp = --spp at
each of --thresholds. Per adaptive run: the time, the mean and the histogram of the samples the pixels took, and the
RMSE of its image against the fixed-spp render (which is itself one sample of the converged image: at threshold 0 the
RMSE is the two calls' summation-order difference, at a large threshold mostly the adaptive image's own noise).

The overhead line: threshold = 0 takes every pixel with variance to max_spp, the same samples in the same items as
rt_render_tiles with samples_per_item = batch; the difference of the two times is what the moments resolve, the select
and the round loop (one host wait a round) cost.

Device pointers out, HIP events around each call, the median of --reps calls after --warmup. One JSON line per
precision and run is printed and appended to --out.

  python scripts/adaptive_throughput.py [--width W] [--spp S] [--depth D] [--batch B] [--step T] [--thresholds a,b,c]
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
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--step", type=int, default=32, help="min_spp and step_spp")
    ap.add_argument("--thresholds", default="0,0.01,0.02,0.05")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_throughput.jsonl"))
    a = ap.parse_args()
    desc, cam, _, _ = scenes.cornell_box(width=a.width)
    ctx = rt_amd.Context(0)
    ctx.upload(desc)
    dev = torch.device("cuda", 0)
    stream = ctx._torch_stream(None, dev)
    n = cam.image_width * cam.image_height
    tiles = abi.TileList([(0, 0, cam.image_width, cam.image_height)])
    base = {"scene": "cornell_box", "width": a.width, "spp": a.spp, "depth": a.depth, "batch": a.batch, "step": a.step}
    with open(a.out, "a") as log:
        def emit(row):
            line = json.dumps(dict(base, **row))
            print(line, flush=True)
            log.write(line + "\n")

        for prec, pname, dtype in ((abi.RT_PREC_F32, "f32", torch.float32), (abi.RT_PREC_F64, "f64", torch.float64)):
            img = torch.empty((n, 3), dtype=dtype, device=dev)
            fixed = {}
            for what, spi in (("render", 0), ("render_items_of_batch", a.batch)):
                prm = ctx.params(a.spp, a.depth, seed=1, precision=prec, samples_per_item=spi)
                t = timed(lambda: ctx.render_tiles(cam, prm, tiles, img.data_ptr(), 1, stream), a.warmup, a.reps)
                fixed[what] = float(np.median(t))
                emit({"precision": pname, "call": what, "kernel": ctx.last_kernel(), "ms": fixed[what],
                      "spread_ms": [float(t.min()), float(t.max())], "gsamples_s": n * a.spp / np.median(t) / 1e6})
            ref = img.to(torch.float64).clone()  # the fixed-spp image in the adaptive call's item layout
            for thr in [float(x) for x in a.thresholds.split(",")]:
                out = {}

                def call():
                    out.update(ctx.render_adaptive(cam, a.spp, a.depth, thr, min_spp=a.step, step_spp=a.step,
                                                   batch=a.batch, seed=1, precision=prec, device=True))
                t = timed(call, a.warmup, a.reps)
                spp = out["spp"].reshape(-1)
                taken = torch.bincount(spp // a.step, minlength=a.spp // a.step + 1)[1:].cpu().numpy()
                # the histogram in eight equal ranges of rounds
                hist = [int(h.sum()) for h in np.array_split(taken, 8)]
                rmse = float(torch.sqrt(((out["rgb"].reshape(-1, 3).to(torch.float64) - ref) ** 2).mean()))
                ms = float(np.median(t))
                row = {"precision": pname, "call": "adaptive", "threshold": thr, "ms": ms,
                       "spread_ms": [float(t.min()), float(t.max())], "mean_spp": float(spp.double().mean()),
                       "rounds": int(spp.max()) // a.step, "spp_hist_8": hist, "rmse_vs_fixed": rmse,
                       "err_mean": float(out["err"].mean()), "err_max": float(out["err"].max()),
                       "gsamples_s": float(spp.double().sum()) / ms / 1e6, "speedup_vs_render": fixed["render"] / ms}
                if thr == 0.0:
                    row["overhead_ms_vs_render_items_of_batch"] = ms - fixed["render_items_of_batch"]
                emit(row)
    ctx.close()


if __name__ == "__main__":
    main()
