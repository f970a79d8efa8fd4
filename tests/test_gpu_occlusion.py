"""rt_occluded on the GPU: any-hit queries with early exit through every traversal family and both precisions.

The contract (include/rt_hip.h): out_occluded[i] == 1 exactly when rt_trace_rays, called with the same context,
params and ray, reports a hit -- no tolerance, no ray left out. Section 1 holds every family to it, on camera rays
with five tmax values each (the reported t itself must count as occluded, the double just below it must not) and on
segments that start on surfaces and point everywhere. Section 2 ties the answers to the geometry through the numpy
brute force of tests/trace_ref.py, with the project's bounds (test_gpu_aov.py): fp64 off the rays the reference flags
near a decision boundary at 1e-9, at most 0.2 % of them; fp32 off those at EPS32 = 1e-4, at most CAP32 = 2 %. The
reference-alone near shares of the chosen rays (aov_ref.perspective_rays on the CPU): Cornell 0 / 0 / 0 at 1e-9 and
0 / 0.10 % / 0.11 % at 1e-4 for tmax = 0.5 t, 2 t and the segments to (300.3, 420.7, 250.1); the heightfield
0 / 0 / 0 and 0 / 0 / 0.42 % with the segments to (1, 4, 0.5). (A target in the plane of a box face, such as z = 200
in the Cornell box, puts 7 % of the segments inside that plane: exactly on a boundary.)
The rest is plumbing: ray counts, the device path and its stream, errors, counters, and renders left untouched.
"""
import ctypes
import math

import numpy as np
import pytest

import rt_amd
import trace_ref
from rt_amd import abi, scenes
from rt_amd.scene import SceneBuilder, perspective

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
AUTO, ORDERED = abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED
INF = math.inf
EPS32, CAP32 = 1e-4, 0.02
SEED = 3


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- scenes (the builders of test_gpu_aov.py, restated)
def field_scene():
    s = SceneBuilder()
    world = trace_ref.heightfield(s, s.lambertian(s.solid((0.5, 0.4, 0.3))))
    cam = perspective(32, 1.0, (0, 9, -16), (0, 0.5, 0), 1, 50.0)
    return s.desc(world, background=s.solid((0.7, 0.8, 1.0))), cam


def instance_scene():
    """A small bvh with a translated, rotated box, beyond the linear program's size: the binary BVH."""
    s = SceneBuilder()
    m = [s.lambertian(s.solid((0.5, 0.5, 0.5))), s.metal(s.solid((0.8, 0.6, 0.2)), 0.1)]
    members = [s.translate(s.rotate(1, s.box((0, 0, 0), (2, 3, 2), m[0]), 15.0), (1.5, 0, 2.0)),
               s.quad((-8, -0.5, -8), (16, 0, 0), (0, 0, 16), m[1]), s.sphere((-2.5, 1.0, 1.0), 1.0, m[1])]
    members += [s.sphere((3.0 * k, -1000.0 - 3.0 * (k % 7), 2.0 * k), 0.25, m[0]) for k in range(100)]
    cam = perspective(48, 4.0 / 3.0, (3, 6, -11), (1, 1, 2), 1, 45.0)
    return s.desc(s.bvh(members), background=s.solid((0.2, 0.3, 0.4))), cam


ROOM = ([0, 0, 0], [555, 555, 555])
BALLS = ([-11, 0, -11], [11, 1.5, 11])
# name -> (scene and camera, the extent segment targets are drawn in)
SCENES = {
    "cornell": (lambda: scenes.cornell_box(width=32)[:2], ROOM),
    "smoke": (lambda: scenes.cornell_box_with_volume(width=32)[:2], ROOM),
    "rtow": (lambda: scenes.rtow(width=64)[:2], BALLS),
    "rtow_motion": (lambda: scenes.rtow(width=64, moving=True)[:2], BALLS),
    "field": (field_scene, ([-10, 0, -10], [10, 3, 10])),
    "boxes": (instance_scene, ([-4, -0.5, -4], [5, 4, 5])),
}
CASES = [("cornell", AUTO, "FLAT"), ("cornell", ORDERED, "LINEAR"), ("smoke", AUTO, "LINEAR"),
         ("rtow", AUTO, "WIDE_LDS"), ("rtow", ORDERED, "STACK"), ("rtow_motion", AUTO, "WIDE_LDS"),
         ("field", AUTO, "WIDE_HBM"), ("boxes", AUTO, "STACK")]


def with_tmax(rays, tmax):
    r = rays.copy()
    r[:, 7] = tmax
    return r


def segments(rays, p, q, keep):
    """o = p, d = q - p, tmax = 1 for the rays of `keep`, each with its camera ray's time."""
    seg = rays[keep].copy()
    seg[:, 0:3] = p[keep]
    seg[:, 3:6] = q[keep] - p[keep]
    seg[:, 7] = 1.0
    return np.ascontiguousarray(seg)


# ---------------------------------------------------------------- 1. the contract, per family and precision
@pytest.mark.parametrize("name,trav,family", CASES)
def test_equals_the_closest_hit_query(ctx, name, trav, family):
    make, extent = SCENES[name]
    desc, cam = make()
    ctx.upload(desc)
    rays = ctx.camera_rays(cam, 1, seed=SEED)
    n = rays.shape[0]
    assert n in (64 * 36, 48 * 36, 32 * 32)
    q = np.random.default_rng(17).uniform(extent[0], extent[1], (n, 3))
    for prec in (F64, F32):
        assert ctx.trace_family(prec, trav) == family
        kw = dict(precision=prec, traversal=trav, seed=SEED)
        geom, _ = ctx.trace_rays(rays, **kw)
        t = geom[:, 0]
        hit = np.isfinite(t)
        assert 0.05 < hit.mean() <= 1.0
        # set (i): one call per tmax, so that ray i keeps its index (a volume's draw is keyed by it)
        sets = {"inf": np.full(n, INF), "0.5 t": np.where(hit, 0.5 * t, 1.0), "t": np.where(hit, t, 1.0),
                "below t": np.where(hit, np.nextafter(t, 0.0), 1.0), "2 t": np.where(hit, 2.0 * t, INF)}
        for label, tmax in sets.items():
            r = with_tmax(rays, tmax)
            occ = ctx.occluded(r, **kw)
            assert occ.dtype == np.uint8 and occ.shape == (n,)
            want = np.isfinite(ctx.trace_rays(r, **kw)[0][:, 0])
            assert np.array_equal(occ, want), (name, family, prec, label, int((occ != want).sum()))
            if label in ("inf", "t", "2 t"):  # the interval is closed: the reported t itself is inside
                assert np.array_equal(occ, hit), (name, family, prec, label)
            if label == "below t":
                assert not occ[hit].any(), (name, family, prec, label)
        # set (ii): segments from the first hits into the scene's extent, from surfaces and from inside boxes
        seg = segments(rays, geom[:, 1:4], q, hit)
        occ = ctx.occluded(seg, **kw)
        want = np.isfinite(ctx.trace_rays(seg, **kw)[0][:, 0])
        print(f"{name} {family} precision {prec}: hits {hit.mean():.2f}, occluded segments {occ.mean():.2f}")
        assert np.array_equal(occ, want), (name, family, prec, int((occ != want).sum()))
        assert 0.05 < occ.mean() < 0.95


def test_degenerate_tmax_is_never_occluded(ctx):
    desc, cam = SCENES["cornell"][0]()
    ctx.upload(desc)
    rays = ctx.camera_rays(cam, 1, seed=SEED)
    for trav in (AUTO, ORDERED):
        for prec in (F64, F32):
            # 0.001 as a double lies below the float 0.001f: in fp32 no float t fits [0.001f, tmax] either
            for tmax in (math.nan, -1.0, 0.0, 0.0009, -INF, np.nextafter(0.001, 0.0)):
                r = with_tmax(rays, tmax)
                assert not ctx.occluded(r, precision=prec, traversal=trav).any(), (trav, prec, tmax)
                assert not np.isfinite(ctx.trace_rays(r, precision=prec, traversal=trav)[0][:, 0]).any()


# ---------------------------------------------------------------- 2. the numpy brute force
TARGET = {"cornell": (300.3, 420.7, 250.1), "field": (1.0, 4.0, 0.5)}


@pytest.fixture(scope="module")
def brute():
    """Per scene: the rays of section 2 with the brute force's answers at both eps, computed once."""
    cache = {}

    def get(ctx, name):
        if name not in cache:
            desc, cam = SCENES[name][0]()
            rays = ctx.camera_rays(cam, 1, seed=SEED)
            leaves = trace_ref.flatten(desc._owner, desc.world)
            first = trace_ref.trace(leaves, rays, seed=SEED)
            hit = np.isfinite(first["t"])
            t = first["t"]
            q = np.broadcast_to(np.array(TARGET[name]), (rays.shape[0], 3))
            groups = {"0.5 t": with_tmax(rays, np.where(hit, 0.5 * t, 1.0)),
                      "2 t": with_tmax(rays, np.where(hit, 2.0 * t, INF)),
                      "segments": segments(rays, first["p"], q, hit)}
            refs = {g: {eps: trace_ref.trace(leaves, r, seed=SEED, eps=eps) for eps in (1e-9, EPS32)}
                    for g, r in groups.items()}
            cache[name] = (desc, groups, refs)
        return cache[name]
    return get


@pytest.mark.parametrize("prec", [F64, F32])
@pytest.mark.parametrize("name", ["cornell", "field"])
def test_against_brute_force(ctx, brute, name, prec):
    desc, groups, refs = brute(ctx, name)
    ctx.upload(desc)
    eps, cap = (1e-9, 0.002) if prec == F64 else (EPS32, CAP32)
    left_out = total = 0
    for g, r in groups.items():
        ref = refs[g][eps]
        want, near = np.isfinite(ref["t"]), ref["near"]
        occ = ctx.occluded(r, precision=prec)
        print(f"{name} precision {prec} {g}: {int(near.sum())} of {near.size} rays near a boundary at {eps}, "
              f"occluded {occ.mean():.3f} (brute force {want.mean():.3f})")
        assert np.array_equal(occ[~near], want[~near].astype(np.uint8)), (name, prec, g)
        left_out += int(near.sum())
        total += near.size
    assert left_out <= cap * total, (name, prec, left_out, total)
    assert 0.05 < np.isfinite(refs["segments"][eps]["t"]).mean() < 0.95


# ---------------------------------------------------------------- 3. ray counts, 4. the stream
@pytest.fixture(scope="module")
def ball(ctx):
    desc, cam, _, _ = scenes.three_material_ball(width=32)
    return desc, cam


def ball_rays(n, seed=71):
    rng = np.random.default_rng(seed)
    r = np.empty((n, 8))
    r[:, 0:3] = rng.uniform([-3, 0.2, 1], [3, 3, 4], (n, 3))
    r[:, 3:6] = rng.uniform([-2, -0.5, -2], [2, 1.5, 0], (n, 3)) - r[:, 0:3]
    r[:, 6] = 0.0
    r[:, 7] = rng.choice([0.5, 1.0, 2.0, INF], n)
    return r


@pytest.mark.parametrize("n", [0, 1, 255, (1 << 20) + 77])
def test_ray_counts(ctx, ball, n):
    import torch
    ctx.upload(ball[0])
    rays = ball_rays(n)
    host = ctx.occluded(rays)
    assert host.dtype == np.uint8 and host.shape == (n,)
    if n > 1:
        assert 0.05 < host.mean() < 0.95
    buf = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    dev = ctx.occluded(torch.from_numpy(rays).to("cuda"), out=buf)
    torch.cuda.synchronize()
    assert dev.shape == (n,) and dev.dtype == torch.uint8 and (n == 0 or dev.data_ptr() == buf.data_ptr())
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n], host)
    assert (got[n:] == 0xAA).all()  # nothing past the last ray
    if n:
        assert np.array_equal(host, np.isfinite(ctx.trace_rays(rays)[0][:, 0]))


def test_device_path_on_a_stream_is_the_host_path(ctx, ball):
    import torch
    ctx.upload(ball[0])
    rays = ball_rays(5000)
    for prec in (F64, F32):
        host = ctx.occluded(rays, precision=prec)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            dr = torch.from_numpy(rays).to("cuda", non_blocking=False)
            d1 = ctx.occluded(dr, precision=prec)
            d2 = ctx.occluded(dr, precision=prec, stream=stream)
        stream.synchronize()
        for d in (d1, d2):
            assert d.is_cuda and d.dtype == torch.uint8 and d.shape == (5000,)
            assert np.array_equal(d.cpu().numpy(), host)


# ---------------------------------------------------------------- 5. errors
def test_needs_a_scene_and_valid_arguments(ctx, ball):
    import torch
    fresh = rt_amd.Context(0)
    try:
        with pytest.raises(abi.RTError) as e:
            fresh.occluded(ball_rays(4))
        assert e.value.status == abi.RT_ERR_NO_SCENE and "rt_scene_upload" in str(e.value)
    finally:
        fresh.close()
    ctx.upload(ball[0])
    for kw in (dict(precision=7), dict(traversal=5)):
        with pytest.raises(abi.RTError) as e:
            ctx.occluded(ball_rays(4), **kw)
        assert e.value.status == abi.RT_ERR_INVALID_ARGUMENT and "unknown" in str(e.value)
    lib, h = ctx.lib, ctx.h
    prm = abi.rt_trace_params(seed=1, precision=F64)
    rays = ball_rays(4)
    out = np.full(4, 0xAA, np.uint8)
    rp, op = rays.ctypes.data, out.ctypes.data
    dev = torch.from_numpy(ball_rays(5)).to("cuda")
    dout = torch.zeros(8, dtype=torch.uint8, device="cuda")
    dprm = abi.rt_trace_params(seed=1, precision=F64, on_device=1)
    bad = [(ctypes.byref(prm), None, 4, op), (ctypes.byref(prm), rp, 4, None), (None, rp, 4, op),
           (ctypes.byref(prm), rp, -1, op), (ctypes.byref(prm), rp, 1 << 31, op),
           (ctypes.byref(dprm), dev.data_ptr() + 8, 4, dout.data_ptr())]  # a device ray pointer off 16 bytes
    for p, r, n, o in bad:
        assert lib.rt_occluded(h, p, r, n, o, None) == abi.RT_ERR_INVALID_ARGUMENT
        assert lib.rt_last_error(h)
    assert (out == 0xAA).all()
    assert lib.rt_occluded(h, ctypes.byref(prm), rp, 4, op, None) == abi.RT_OK
    assert np.array_equal(out, ctx.occluded(rays))


# ---------------------------------------------------------------- 6. non-interference and counters
def test_render_is_untouched_and_counters_add_up(ctx, ball):
    desc, cam = ball
    ctx.upload(desc)
    before = [ctx.render(cam, 4, 8, seed=3, precision=p) for p in (F32, F64)]
    for prec in (F32, F64):
        ctx.occluded(ball_rays(3000), precision=prec)
        ctx.occluded(ball_rays(3000), precision=prec, traversal=ORDERED)
    after = [ctx.render(cam, 4, 8, seed=3, precision=p) for p in (F32, F64)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    ctx.reset_counters()
    for k in range(3):
        ctx.occluded(ball_rays(777), precision=(F64, F32)[k % 2])
    st = ctx.stats()
    assert st.segments == 3 * 777 and st.launches == 3
