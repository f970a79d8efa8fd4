"""rt_radiance (Context.radiance): path-traced radiance along caller-given rays, on the device.

1. Against the oracle. TABLE holds one scene per persistent kernel family and shade form (material_scenes.py's): a batch
   of 1024 rays at 16 spp, depth 8 -- 512 of the scene camera's own rays and 512 that leave surface points (p, n of
   trace_rays: o = p, d = n + 0.7 f_i, f_i a Fibonacci-sphere direction), all with a NaN time. The reference of ray i is
   oracle.render of tile (i, 0, 1, 1) of a 1024 x 1 perspective camera with pos = o_i, dir = d_i, focal_length = 1 and a
   zero viewport: it generates exactly the ray (o_i, d_i) for every sample of pixel i and keys its path (seed, i,
   sample), which is the call's contract. The 1024 values, as a 32 x 32 frame, are held to
   test_gpu_lights.check_against_oracle's rules as they stand, and the launched kernel's tag to plan_radiance_kernel's.
2. Against the render, without the oracle: radiance along camera_rays' sample s equals the render's sample s.
3. The ray time: a NaN time draws what camera::generate_ray draws, bit for bit; another time moves a moving sphere.
4. Keys and shapes: with samples_per_item given, a ray's value depends on its key alone, bit for bit -- any split of
   a batch past one 65535-wide row, single rays, the device path.
5. The contract: every refused argument, the counters, and renders and batches interleaved on one context.
"""
import ctypes
import math

import numpy as np
import pytest

import material_scenes as S
import oracle
import rt_amd
import test_gpu_materials as materials
import test_material_scenes as cpu
from kernel_tags import (FLAT_GLOBAL, FLAT_LDS, FLAT_LL, LIN_ALL, LIN_LLI, LIN_QUAD, LIN_SPH, LIN_VOL, W_ALL, W_ALL_HBM,
                         W_SPH_NL, W_SPH_NL_HBM, W_TQ_LL, W_TQ_LL_HBM, W_TRI, W_TRI_HBM)
from rt_amd import abi
from test_gpu_lights import check_against_oracle

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
AUTO, ORDERED = abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED
P = {F32: "f32", F64: "f64"}
BOTH = (F32, F64)
N, SPP, DEPTH, SEED = 1024, 16, 8, 11

# (scene, traversal, traversal tag, "camx" or "", precisions): one scene per persistent family and shade form
ROWS = [
    # the flat program: LL, its tables in LDS, its records in global memory (33 materials)
    ("backlight", AUTO, FLAT_LL, "", BOTH),
    ("metal", AUTO, FLAT_LDS, "", BOTH),
    ("mats33", AUTO, FLAT_GLOBAL, "", BOTH),
    # the linear programs
    ("glass_rot", AUTO, LIN_QUAD, "", BOTH),
    ("smoke_thick", AUTO, LIN_LLI, "", BOTH),
    ("smoke_nolight", AUTO, LIN_VOL, "", BOTH),
    ("chain", AUTO, LIN_SPH, "", BOTH),
    ("smoke_ball", AUTO, LIN_ALL, "", BOTH),
    # the wide tree, in LDS and in HBM: NL, general (moving spheres: fp64 only, as in the other tables), LL, triangles
    ("spheres_nl", AUTO, W_SPH_NL, "", BOTH),
    ("spheres_nl_hbm", AUTO, W_SPH_NL_HBM, "", BOTH),
    ("mixed_static", AUTO, W_ALL, "", BOTH),
    ("mixed_static_hbm", AUTO, W_ALL_HBM, "", BOTH),
    ("mixed", AUTO, W_ALL, "", (F64,)),
    ("mesh_ll", AUTO, W_TQ_LL, "", BOTH),
    ("terrain_ll", AUTO, W_TQ_LL_HBM, "", BOTH),
    ("mesh_tris", AUTO, W_TRI, "", BOTH),
    ("terrain", AUTO, W_TRI_HBM, "", BOTH),
    # the binary BVH: 8, 16 and 32 stack entries; fp32 with its nodes in LDS (mesh) and in HBM (spheres_nl_hbm)
    ("instanced", AUTO, materials.B_INST, "", BOTH),
    ("mesh", ORDERED, materials.B_MID, "", BOTH),
    ("spheres_nl_hbm", ORDERED, materials.B_LARGE, "", BOTH),
    ("mesh_deep", ORDERED, materials.B_DEEP, "", BOTH),
    # the extended form, by a picture texture: the linear program and the binary BVH
    ("glass_image", AUTO, LIN_QUAD, "camx", BOTH),
    ("mesh_image", AUTO, materials.B_MID, "camx", BOTH),
]


def tag_of(trav, camx, prec):
    t = (trav[prec] if isinstance(trav, dict) else trav).format(p=P[prec])
    return t + (" camx" if camx else "") + " rays persist"


TABLE = [(name, prec, trav, tag_of(t, camx, prec)) for name, trav, t, camx, precs in ROWS for prec in precs]


def row_id(r):
    return f"{r[0]}-{P[r[1]]}-{'ordered' if r[2] == ORDERED else 'auto'}"


def test_table_covers_every_family_and_form():
    tags = {r[3] for r in TABLE}
    for prec in BOTH:
        for trav in (FLAT_LL, FLAT_LDS, FLAT_GLOBAL, LIN_QUAD, LIN_LLI, LIN_VOL, LIN_SPH, LIN_ALL, W_SPH_NL, W_SPH_NL_HBM,
                     W_ALL, W_ALL_HBM, W_TQ_LL, W_TQ_LL_HBM, W_TRI, W_TRI_HBM):
            assert tag_of(trav, "", prec) in tags, trav
        for stack in ("8,0", "16,0", "32,0"):
            assert f"StackTrav<{P[prec]},{stack}> rays persist" in tags, stack
        assert f"LinearTrav<{P[prec]},0,0,0,0> camx rays persist" in tags
        assert any(t.startswith(f"StackTrav<{P[prec]},") and " camx " in t for t in tags)
    assert "StackTrav<f32,16,1> rays persist" in tags  # the nodes in LDS


# ------------------------------------------------------------------ rays and references
def zero_viewport_camera(n, o, d):
    """The n x 1 perspective camera whose every pixel and sample is the ray (o, d): focal_length 1 and a viewport of
    0 x 0, so that dir00 = dir (+ 0 x right + 0 x up + 0) and du = dv = 0 (camera.h:137-141, 246)."""
    c = abi.rt_camera_desc(mode=abi.RT_CAM_PERSPECTIVE, image_width=n, image_height=1, viewport_width=0.0,
                           viewport_height=0.0, focal_length=1.0, focus_dist=1.0)
    c.pos[:], c.dir[:], c.right[:], c.up[:] = list(o), list(d), [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    return c


def oracle_ray(scene, ray, i, n, spp, depth, seed, first_sample=0):
    img, _ = oracle.render(scene, zero_viewport_camera(n, ray[0:3], ray[3:6]), spp, depth, seed=seed, threads=1,
                           tiles=[(i, 0, 1, 1)], first_sample=first_sample)
    return img[0]


def fibonacci(n):
    i = np.arange(n)
    z = 1.0 - (2.0 * i + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def batch_rays(ctx, cam):
    """N rays of the uploaded scene: N / 2 camera rays (every other pixel of an even spread), then N / 2 rays that leave
    the surface points the other camera rays hit (misses stay camera rays). NaN time, no zero direction component."""
    crays = ctx.camera_rays(cam, 1, seed=SEED)
    pick = (np.arange(N) * crays.shape[0]) // N
    a, b = crays[pick[0::2]].copy(), crays[pick[1::2]].copy()
    geom, _ = ctx.trace_rays(b, precision=F64, seed=SEED)
    hit = np.isfinite(geom[:, 0])
    d = geom[:, 4:7] + 0.7 * fibonacci(N // 2)
    b[hit, 0:3] = geom[hit, 1:4]
    b[hit, 3:6] = d[hit]
    rays = np.ascontiguousarray(np.concatenate([a, b]))
    rays[:, 6] = np.nan
    rays[:, 7] = np.inf
    # (the zero-viewport reference adds +0 to every component: a -0 would become +0 and flip a slab test's infinity)
    rays[:, 3:6][rays[:, 3:6] == 0.0] = 1e-12
    assert np.isfinite(rays[:, :6]).all() and hit.sum() > N // 8
    return rays


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(ctx):
    """scene -> (desc, cam, rays, oracle values (N, 3)): made once per scene, never changed. A ray whose reference is
    not finite (a 0 / 0 weight of the reference) is replaced by the batch's first finite camera ray."""
    cache = {}

    def get(name):
        if name not in cache:
            desc, cam = S.build(name, "perspective")
            ctx.upload(desc)
            rays = batch_rays(ctx, cam)
            scene = oracle.from_desc(desc)
            ref = np.stack([oracle_ray(scene, rays[i], i, N, SPP, DEPTH, SEED) for i in range(N)])
            bad = np.flatnonzero(~np.isfinite(ref).all(-1))
            if bad.size:
                donor = rays[np.flatnonzero(np.isfinite(ref).all(-1))[0]].copy()
                for i in bad:
                    rays[i] = donor
                    ref[i] = oracle_ray(scene, donor, i, N, SPP, DEPTH, SEED)
            assert bad.size < N // 16 and np.isfinite(ref).all(), (name, bad.size)
            rays.setflags(write=False)
            ref.setflags(write=False)
            cache[name] = (desc, cam, rays, ref)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def measured():
    m = {}
    yield m
    for group, vals in sorted(m.items()):
        print(f"[radiance] {group}: " + ", ".join(f"{k} max {max(v):.3g}" for k, v in sorted(vals.items())))


def rules_of(name):
    return dict(bvh=name in S.BVH_SCENES, specular=bool(materials.SPECULAR & set(cpu.EVENTS[(name, "perspective")])))


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("row", TABLE, ids=row_id)
def test_radiance_matches_the_oracle(ctx, refs, measured, row):
    name, prec, trav, tag = row
    desc, cam, rays, ref = refs(name)
    ctx.upload(desc)
    assert rt_amd.plan_radiance_kernel(desc, prec, trav) == tag
    out = ctx.radiance(rays, SPP, DEPTH, seed=SEED, precision=prec, traversal=trav)
    assert ctx.last_kernel() == tag
    assert out.shape == (N, 3) and out.dtype == (np.float64 if prec == F64 else np.float32)
    check_against_oracle(name, prec, out.reshape(32, 32, 3), ref.reshape(32, 32, 3), measured, row_id(row),
                         group=materials.shade_form(tag.replace(" rays", "")).split(" ")[0], **rules_of(name))


# ------------------------------------------------------------------ 2. against the render
@pytest.mark.parametrize("prec", BOTH, ids=P.get)
@pytest.mark.parametrize("name,trav", [("backlight", AUTO), ("smoke_thick", AUTO), ("terrain", AUTO), ("mesh", ORDERED)])
def test_radiance_along_camera_rays_is_the_render(ctx, measured, name, trav, prec):
    desc, cam = S.build(name, "perspective")
    ctx.upload(desc)
    for s in (0, 5):
        rays = ctx.camera_rays(cam, 1, seed=SEED, first_sample=s)  # row y * W + x: ray i is keyed as pixel i
        out = ctx.radiance(rays, 1, DEPTH, seed=SEED, precision=prec, traversal=trav, first_sample=s)
        assert " rays persist" in ctx.last_kernel()
        img = ctx.render(cam, 1, DEPTH, seed=SEED, precision=prec, traversal=trav, first_sample=s)
        assert ctx.last_kernel() == rt_amd.plan_kernel(desc, cam, precision=prec, traversal=trav)
        fin = np.isfinite(img).all(-1)
        diff = np.abs(np.asarray(out, np.float64).reshape(img.shape)[fin] - img[fin])
        # (zero is the expectation; it is not asserted: two instantiations may contract differently)
        print(f"{name} {P[prec]} sample {s}: largest difference from the render {diff.max():.3g}")
        check_against_oracle(name, prec, out.reshape(img.shape), np.asarray(img, np.float64), measured,
                             f"{name}-{P[prec]}-sample{s}", group="render", **rules_of(name))


# ------------------------------------------------------------------ 3. the ray time
def test_nan_time_draws_the_cameras_time_and_a_time_moves_the_spheres(ctx, refs):
    desc, cam, rays, _ = refs("mixed")
    ctx.upload(desc)
    s = 3
    drawn = ctx.radiance(rays, 1, DEPTH, seed=SEED, precision=F64, first_sample=s)
    tag = ctx.last_kernel()
    lib = abi.load()
    timed = rays.copy()
    timed[:, 6] = [(lib.rt_rng_u32(SEED, i, s, 2) >> 8) / 16777216.0 for i in range(N)]  # to_unit of dimension 2
    given = ctx.radiance(timed, 1, DEPTH, seed=SEED, precision=F64, first_sample=s)
    assert ctx.last_kernel() == tag  # the same kernel, the same arithmetic
    assert np.isfinite(drawn).all() and drawn.max() > 0 and np.array_equal(drawn, given)
    # another time: the rays whose first hit is a moving sphere at either time
    other = timed.copy()
    other[:, 6] = (timed[:, 6] + 0.5) % 1.0
    moved = ctx.radiance(other, 1, DEPTH, seed=SEED, precision=F64, first_sample=s)
    moving = np.zeros(N, bool)
    for r in (timed, other):
        _, ids = ctx.trace_rays(np.ascontiguousarray(r), precision=F64, seed=SEED)
        moving |= np.array([o >= 0 and desc.objects[o].moving != 0 for o in ids[:, 0]])
    assert moving.sum() >= 4, int(moving.sum())
    assert (drawn[moving] != moved[moving]).any()


# ------------------------------------------------------------------ 4. keys and shapes
BIG = 65535 + 300


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
@pytest.mark.parametrize("name", ["backlight", "mesh_ll"])
def test_a_rays_value_depends_on_its_key_alone(ctx, refs, name, prec):
    desc, cam, rays, _ = refs(name)
    ctx.upload(desc)
    big = np.ascontiguousarray(rays[np.arange(BIG) % N])
    kw = dict(seed=SEED, precision=prec, samples_per_item=4)
    whole = ctx.radiance(big, 8, 4, **kw)
    assert whole.shape == (BIG, 3) and np.isfinite(whole).all() and whole.mean() > 0.01
    # rays N apart are the same ray under another key: other draws, another value
    assert (whole[:N] != whole[N:2 * N]).any(-1).mean() > 0.1
    cuts = [0, 1, 63, 257, 65535, BIG]
    for a, b in zip(cuts[:-1], cuts[1:]):
        piece = ctx.radiance(np.ascontiguousarray(big[a:b]), 8, 4, ray_base=a, **kw)
        assert np.array_equal(piece, whole[a:b]), (a, b)
    for a, n in ((100, 1), (200, 63), (65534, 3)):
        piece = ctx.radiance(np.ascontiguousarray(big[a:a + n]), 8, 4, ray_base=a, **kw)
        assert np.array_equal(piece, whole[a:a + n]), (a, n)
    # the device path
    import torch
    dev = ctx.radiance(torch.from_numpy(big).to(f"cuda:{ctx.device}"), 8, 4, **kw)
    assert dev.is_cuda and dev.dtype == (torch.float64 if prec == F64 else torch.float32)
    assert np.array_equal(dev.cpu().numpy(), whole)
    # first_sample: the two halves of the samples (fp64: the mean of the halves is the whole to rounding)
    if prec == F64:
        lo = ctx.radiance(big[:N].copy(), 4, 4, first_sample=0, **kw)
        hi = ctx.radiance(big[:N].copy(), 4, 4, first_sample=4, **kw)
        assert (np.abs(0.5 * (lo + hi) - whole[:N]) <= 1e-12 * np.abs(whole[:N])).all()


# ------------------------------------------------------------------ 5. the contract
def call(ctx, prm, rays_ptr, n, out_ptr):
    return ctx.lib.rt_radiance(ctx.h, ctypes.byref(prm) if prm is not None else None, rays_ptr, n, out_ptr, None)


def params(**kw):
    base = dict(seed=SEED, spp=2, first_sample=0, max_depth=4, precision=F64, traversal=AUTO, samples_per_item=0,
                ray_base=0, on_device=0)
    base.update(kw)
    return abi.rt_radiance_params(**base)


def test_refused_arguments_launch_nothing_and_write_nothing(ctx, refs):
    import torch
    desc, cam, rays, _ = refs("backlight")
    ctx.upload(desc)
    r = np.ascontiguousarray(rays[:8])
    out = np.full((8, 3), -7.0)
    rp, op = r.ctypes.data, out.ctypes.data
    before = ctx.stats()
    bad = abi.RT_ERR_INVALID_ARGUMENT
    assert call(ctx, None, rp, 8, op) == bad
    assert call(ctx, params(), None, 8, op) == bad
    assert call(ctx, params(), rp, 8, None) == bad
    assert ctx.lib.rt_radiance(None, ctypes.byref(params()), rp, 8, op, None) == bad
    assert call(ctx, params(), rp, -1, op) == bad
    assert call(ctx, params(ray_base=0xFFFFFFFF), rp, 2, op) == bad       # ray_base + nrays = 2^32 + 1
    assert call(ctx, params(ray_base=0xFFFFFFF9), rp, 8, op) == bad       # 2^32 + 1 again
    assert call(ctx, params(spp=0), rp, 8, op) == bad
    assert call(ctx, params(max_depth=-1), rp, 8, op) == bad
    assert call(ctx, params(), rp, 1 << 31, op) == bad                    # past the item planner's pixels of one call
    assert call(ctx, params(spp=1 << 20), rp, 1 << 31, op) == bad
    assert call(ctx, params(precision=2), rp, 8, op) == bad
    assert call(ctx, params(traversal=2), rp, 8, op) == bad
    drays = torch.zeros((9, 8), dtype=torch.float64, device=f"cuda:{ctx.device}")
    dout = torch.full((9, 3), -7.0, dtype=torch.float64, device=drays.device)
    assert call(ctx, params(on_device=1), drays.data_ptr() + 8, 8, dout.data_ptr()) == bad
    assert call(ctx, params(on_device=1), drays.data_ptr(), 8, dout.data_ptr() + 8) == bad
    after = ctx.stats()
    assert (after.launches, after.samples, after.segments) == (before.launches, before.samples, before.segments)
    assert (out == -7.0).all() and bool((dout == -7.0).all())
    # ray_base + nrays = 2^32 exactly is the last valid batch; nrays = 0 is fine and launches nothing
    assert call(ctx, params(ray_base=0xFFFFFFF8), rp, 8, op) == abi.RT_OK and np.isfinite(out).all()
    launches = ctx.stats().launches
    assert call(ctx, params(), rp, 0, op) == abi.RT_OK and ctx.stats().launches == launches
    assert ctx.radiance(np.zeros((0, 8)), 2, 4).shape == (0, 3)


def test_no_scene():
    c = rt_amd.Context(0)
    try:
        with pytest.raises(abi.RTError) as e:
            c.radiance(np.zeros((1, 8)), 1, 1)
        assert e.value.status == abi.RT_ERR_NO_SCENE
    finally:
        c.close()


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_counters(ctx, refs, prec):
    desc, cam, rays, _ = refs("metal")
    ctx.upload(desc)
    ctx.reset_counters()
    ctx.radiance(rays, 4, DEPTH, seed=SEED, precision=prec)
    st = ctx.stats()
    assert st.samples == N * 4
    assert N * 4 <= st.segments <= N * 4 * DEPTH, st.segments
    assert st.launches == 2  # the path kernel and the resolve of the one pass


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_renders_and_batches_interleave(ctx, refs, prec):
    desc, cam, rays, _ = refs("mesh_ll")
    ctx.upload(desc)
    img0 = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec)
    rad0 = ctx.radiance(rays, 4, DEPTH, seed=SEED, precision=prec)
    img1 = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec)
    rad1 = ctx.radiance(rays, 4, DEPTH, seed=SEED, precision=prec)
    tiles = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec, tiles=[(3, 5, 7, 9)])
    rad2 = ctx.radiance(rays, 4, DEPTH, seed=SEED, precision=prec)
    assert img0.max() > 0 and rad0.max() > 0
    assert np.array_equal(img0, img1) and np.array_equal(rad0, rad1) and np.array_equal(rad0, rad2)
    assert np.array_equal(tiles, img0[5:14, 3:10].reshape(-1, 3))


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_a_batch_between_overlapped_renders(ctx, refs, prec):
    """Device-output renders queued back to back keep the launch lanes live; a device-output batch between them is a
    serial launch on the caller's stream that writes buffer set 0. Every result is, bit for bit, what it is alone."""
    import torch
    desc, cam, rays, _ = refs("mesh_ll")
    ctx.upload(desc)
    alone = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec)
    host = ctx.radiance(rays, 4, DEPTH, seed=SEED, precision=prec)
    assert alone.max() > 0 and host.max() > 0
    dev = torch.device(f"cuda:{ctx.device}")
    dt = torch.float64 if prec == F64 else torch.float32
    bufs = [torch.zeros(alone.shape, dtype=dt, device=dev) for _ in range(6)]
    drays = torch.from_numpy(rays.copy()).to(dev)
    prm = ctx.params(4, DEPTH, SEED, prec)
    stream = ctx._torch_stream(None, dev)
    tl = abi.TileList([(0, 0, cam.image_width, cam.image_height)])
    for b in bufs[:3]:
        ctx.render_tiles(cam, prm, tl, b.data_ptr(), True, stream)
    batch = ctx.radiance(drays, 4, DEPTH, seed=SEED, precision=prec)
    for b in bufs[3:]:
        ctx.render_tiles(cam, prm, tl, b.data_ptr(), True, stream)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        assert np.array_equal(b.cpu().numpy(), alone), k
    assert np.array_equal(batch.cpu().numpy(), host)
