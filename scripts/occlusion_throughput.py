#!/usr/bin/env python3
"""Throughput of rt_occluded beside rt_trace_rays on the same rays: every query family and both precisions -- the
Cornell box (flat program; linear program with ORDERED), rtow (wide BVH in LDS; binary BVH with ORDERED) and a
3200-triangle heightfield (wide BVH in HBM). Three ray sets per scene, built on the device from the scene itself:

  camera  the frame's camera rays, tmax = +inf ("does this ray hit anything")
  shadow  segments from the camera rays' first-hit points p to points q on the light (Cornell) or to a fixed point
          above the scene: o = p, d = q - p, tmax just below 1 (so that the light itself does not count)
  ao      cosine-distributed directions about the first-hit normal, tmax a tenth of the scene's extent

Device pointers in and out, HIP events around each call, the median of REPS calls after WARMUP. One JSON line per
(scene, family, precision, set) is printed and appended to --out: rays/s of both calls, their ratio, the occluded
share, both spreads (min-max of the timings), and slower_beyond_spread -- rt_occluded's median above rt_trace_rays'
by more than the larger of the two spreads.

  python scripts/occlusion_throughput.py [--width W] [--spp S] [--reps R] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "python"))

import torch  # noqa: E402

import rt_amd  # noqa: E402
from rt_amd import abi, scenes  # noqa: E402
from rt_amd.scene import SceneBuilder, perspective  # noqa: E402

AUTO, ORDERED = abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED
BELOW_ONE = 1.0 - 2.0 ** -20


def heightfield(width, cells=40, size=20.0, seed=5):
    s = SceneBuilder()
    m = s.lambertian(s.solid((0.5, 0.4, 0.3)))
    rng = np.random.default_rng(seed)
    h = rng.uniform(0.0, 1.5, (cells + 1, cells + 1))
    xs = np.linspace(-size / 2, size / 2, cells + 1)
    tris = []
    for i in range(cells):
        for j in range(cells):
            p = lambda a, b: (xs[a], h[a, b], xs[b])
            tris.append(s.triangle(p(i, j), p(i + 1, j), p(i, j + 1), m))
            tris.append(s.triangle(p(i + 1, j), p(i + 1, j + 1), p(i, j + 1), m))
    cam = perspective(width, 1.0, (0, 9, -16), (0, 0.5, 0), 1, 50.0)
    return s.desc(s.bvh(tris), background=s.solid((0.7, 0.8, 1.0))), cam


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms), out


def ray_sets(ctx, cam, spp, light, extent):
    """name -> (n, 8) device rays, from the camera rays and their fp64 first hits."""
    rays = ctx.camera_rays(cam, spp, seed=1, device=True)
    geom, _ = ctx.trace_rays(rays, precision=abi.RT_PREC_F64, seed=1)
    hit = torch.isfinite(geom[:, 0])
    p, nrm, time = geom[hit][:, 1:4], geom[hit][:, 4:7], rays[hit][:, 6]
    m = p.shape[0]
    g = torch.Generator(device=rays.device).manual_seed(7)
    u = torch.rand((m, 2), dtype=torch.float64, device=rays.device, generator=g)
    lo, du, dv = (torch.tensor(v, dtype=torch.float64, device=rays.device) for v in light)
    q = lo + u[:, 0:1] * du + u[:, 1:2] * dv
    shadow = torch.cat([p, q - p, time[:, None], torch.full((m, 1), BELOW_ONE, dtype=torch.float64, device=rays.device)], 1)
    # random_cosine_direction about the normal (the normal of a moving sphere is not a unit vector: normalised here)
    w = nrm / nrm.norm(dim=1, keepdim=True)
    a = torch.where(w[:, 0:1].abs() > 0.9, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=rays.device),
                    torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=rays.device))
    v = torch.linalg.cross(w, a)
    v = v / v.norm(dim=1, keepdim=True)
    uu = torch.linalg.cross(w, v)
    r = torch.rand((m, 2), dtype=torch.float64, device=rays.device, generator=g)
    phi, sr = 2.0 * math.pi * r[:, 0:1], torch.sqrt(r[:, 1:2])
    d = torch.cos(phi) * sr * uu + torch.sin(phi) * sr * v + torch.sqrt(1.0 - r[:, 1:2]) * w
    ao = torch.cat([p, d, time[:, None], torch.full((m, 1), 0.1 * extent, dtype=torch.float64, device=rays.device)], 1)
    return {"camera": rays, "shadow": shadow.contiguous(), "ao": ao.contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occlusion_throughput.jsonl"))
    a = ap.parse_args()
    # scene, camera, the shadow rays' targets as origin + u edge1 + v edge2, the extent, (traversal, family) rows
    cornell, rtow, field = scenes.cornell_box(width=a.width), scenes.rtow(width=a.width), heightfield(a.width)
    cases = [("cornell_box", cornell[0], cornell[1], ((213.0, 554.0, 227.0), (130.0, 0, 0), (0, 0, 105.0)), 555.0,
              ((AUTO, "FLAT"), (ORDERED, "LINEAR"))),
             ("rtow", rtow[0], rtow[1], ((0.0, 30.0, 0.0), (0, 0, 0), (0, 0, 0)), 22.0,
              ((AUTO, "WIDE_LDS"), (ORDERED, "STACK"))),
             ("heightfield", field[0], field[1], ((0.0, 30.0, 0.0), (0, 0, 0), (0, 0, 0)), 20.0, ((AUTO, "WIDE_HBM"),))]
    ctx = rt_amd.Context(0)
    with open(a.out, "a") as log:
        for name, desc, cam, light, extent, rows in cases:
            ctx.upload(desc)
            sets = ray_sets(ctx, cam, a.spp, light, extent)
            for trav, family in rows:
                for prec, pname in ((abi.RT_PREC_F32, "f32"), (abi.RT_PREC_F64, "f64")):
                    assert ctx.trace_family(prec, trav) == family, (name, ctx.trace_family(prec, trav))
                    for sname, rays in sets.items():
                        n = rays.shape[0]
                        kw = dict(precision=prec, traversal=trav, seed=1)
                        t_ms, (geom, _ids) = timed(lambda: ctx.trace_rays(rays, **kw), a.warmup, a.reps)
                        o_ms, occ = timed(lambda: ctx.occluded(rays, **kw), a.warmup, a.reps)
                        assert torch.equal(occ.bool(), torch.isfinite(geom[:, 0])), (name, family, pname, sname)
                        tm, om = float(np.median(t_ms)), float(np.median(o_ms))
                        spread = max(float(t_ms.max() - t_ms.min()), float(o_ms.max() - o_ms.min()))
                        line = json.dumps({
                            "scene": name, "family": family, "precision": pname, "set": sname, "rays": n,
                            "reps": a.reps, "occluded_share": round(float(occ.float().mean()), 4),
                            "trace_ms_median": round(tm, 4), "trace_ms_min": round(float(t_ms.min()), 4),
                            "trace_ms_max": round(float(t_ms.max()), 4), "trace_grays_per_s": round(n / tm / 1e6, 3),
                            "occluded_ms_median": round(om, 4), "occluded_ms_min": round(float(o_ms.min()), 4),
                            "occluded_ms_max": round(float(o_ms.max()), 4),
                            "occluded_grays_per_s": round(n / om / 1e6, 3), "occluded_over_trace_rate": round(tm / om, 3),
                            "slower_beyond_spread": bool(om - tm > spread)})
                        print(line, flush=True)
                        log.write(line + "\n")
                        log.flush()
    ctx.close()


if __name__ == "__main__":
    main()
