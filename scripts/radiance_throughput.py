#!/usr/bin/env python3
"""Throughput of rt_radiance beside rt_render_tiles on the C2 scene (bench.py: the Cornell box, 800 x 800, depth 50):
the batch is the frame's own camera rays (sample 0 of every pixel, on the device), traced at --spp samples a ray; the
render is the same frame at the same spp. Both run the flat program's LL kernel, the batch in its "rays" form, so
the two differ in where a sample's first ray comes from (64 bytes loaded per sample against a pixel base and two
draws), in the jitter (a batch's samples share their first ray, a pixel's do not) and in the launch order (a batch
stays on the caller's stream, consecutive frames overlap on the launch lanes).

Device pointers in and out, HIP events around each call, the median of --reps calls after --warmup. One JSON line per
precision is printed and appended to --out: samples/s of both calls, their ratio, both spreads (min-max of the
timings) and the two kernels' tags.

  python scripts/radiance_throughput.py [--width W] [--spp S] [--depth D] [--reps R] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "radiance_throughput.jsonl"))
    a = ap.parse_args()
    desc, cam, _, _ = scenes.cornell_box(width=a.width)
    ctx = rt_amd.Context(0)
    ctx.upload(desc)
    dev = torch.device("cuda", 0)
    stream = ctx._torch_stream(None, dev)
    rays = ctx.camera_rays(cam, 1, seed=1, device=True)
    n = rays.shape[0]
    tiles = abi.TileList([(0, 0, cam.image_width, cam.image_height)])
    with open(a.out, "a") as log:
        for prec, pname, dtype in ((abi.RT_PREC_F32, "f32", torch.float32), (abi.RT_PREC_F64, "f64", torch.float64)):
            img = torch.empty((n, 3), dtype=dtype, device=dev)
            prm = ctx.params(a.spp, a.depth, seed=1, precision=prec)
            t_render = timed(lambda: ctx.render_tiles(cam, prm, tiles, img.data_ptr(), 1, stream), a.warmup, a.reps)
            k_render = ctx.last_kernel()
            t_batch = timed(lambda: ctx.radiance(rays, a.spp, a.depth, seed=1, precision=prec), a.warmup, a.reps)
            k_batch = ctx.last_kernel()
            samples = float(n) * a.spp
            row = {"scene": "cornell_box", "width": a.width, "spp": a.spp, "depth": a.depth, "precision": pname,
                   "rays": n, "render_kernel": k_render, "radiance_kernel": k_batch,
                   "render_ms": float(np.median(t_render)), "radiance_ms": float(np.median(t_batch)),
                   "render_spread_ms": [float(t_render.min()), float(t_render.max())],
                   "radiance_spread_ms": [float(t_batch.min()), float(t_batch.max())],
                   "render_gsamples_s": samples / np.median(t_render) / 1e6,
                   "radiance_gsamples_s": samples / np.median(t_batch) / 1e6,
                   "radiance_over_render": float(np.median(t_render) / np.median(t_batch))}
            line = json.dumps(row)
            print(line)
            log.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
