"""rt_camera_rays and rt_render_aov on the GPU: the camera rays against a numpy restatement of camera.h, the feature
buffers against the query path (rt_trace_rays on the same rays), the numpy brute force of tests/trace_ref.py, and the
oracle's render of a clone whose materials are all lights (its image is then the albedo channel).

Bounds are the project's, from test_gpu_trace.py. fp64: decisions and ids equal, values within 1e-9 max(1, |v|).
fp32: rays near a decision boundary at EPS32 = 1e-4 (trace_ref.py) are left out, at most CAP32 = 2 %; on the rest
every decision equals the reference and the values are held to 8 x the error of the same formulas in numpy float32.
"""
import ctypes
import math

import numpy as np
import pytest

import aov_ref
import oracle
import rt_amd
import trace_ref
from rt_amd import abi, scenes
from rt_amd.scene import SceneBuilder, fisheye, lens, orthonormal, perspective

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
AUTO, ORDERED = abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED
EPS32, CAP32 = 1e-4, 0.02
CHANNELS = ("albedo", "normal", "depth", "hit", "ids")


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()) if a.size else 0.0


def flat(aov):
    """The channels as per-pixel rows, whatever the shape render_aov returned them in."""
    return dict(albedo=aov["albedo"].reshape(-1, 3), normal=aov["normal"].reshape(-1, 3), depth=aov["depth"].reshape(-1),
                hit=aov["hit"].reshape(-1), ids=aov["ids"].reshape(-1, 4))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in CHANNELS)


def quadrants(cam):
    """Four tiles of unequal, odd sizes covering the image."""
    W, H = cam.image_width, cam.image_height
    cx, cy = W // 2 - 3, H // 2 + 1
    return [(0, 0, cx, cy), (cx, 0, W - cx, cy), (0, cy, cx, H - cy), (cx, cy, W - cx, H - cy)]


def pixel_index(cam, tiles):
    return np.array([y * cam.image_width + x for x, y in aov_ref.packed_pixels(cam, tiles)])


def ball_cameras(width=64):
    a = 16.0 / 9.0
    return {"perspective": perspective(width, a, (13, 2, 3), (0, 0, 0), 1, 20.0),
            "orthonormal": orthonormal(width, a, 3.0, (13, 2, 3), (0, 0, 0)),  # (every origin above the ground)
            "fisheye": fisheye(width, a, (13, 2, 3), (0, 0, 0), 1, 20.0),
            "lens": lens(width, a, (13, 2, 3), (1, 1, 1), 2.0, 15, 20.0)}


def field_scene():
    s = SceneBuilder()
    world = trace_ref.heightfield(s, s.lambertian(s.solid((0.5, 0.4, 0.3))))
    cam = perspective(64, 1.0, (0, 9, -16), (0, 0.5, 0), 1, 50.0)
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


# ---------------------------------------------------------------- 1. camera rays
def test_perspective_rays_match_camera_h(ctx):
    cam = ball_cameras()["perspective"]
    assert (cam.image_width, cam.image_height) == (64, 36)
    for first in (0, 5):
        got = ctx.camera_rays(cam, 2, seed=7, first_sample=first)
        want = aov_ref.perspective_rays(cam, 2, seed=7, first_sample=first)
        assert got.shape == want.shape == (64 * 36 * 2, 8)
        assert (got[:, 7] == math.inf).all() and np.array_equal(got[:, 0:3], want[:, 0:3])
        assert np.array_equal(got[:, 6], want[:, 6])  # the time draw
        e = float((np.abs(got[:, 3:6] - want[:, 3:6]).max(1) / np.sqrt((want[:, 3:6] ** 2).sum(1))).max())
        print(f"perspective rays, first sample {first}: max rel err {e:.2e}")
        assert e <= 1e-12


@pytest.mark.parametrize("mode", ["perspective", "orthonormal", "fisheye", "lens"])
def test_rays_do_not_depend_on_tiling(ctx, mode):
    cam = ball_cameras()[mode]
    spp = 3
    full = ctx.camera_rays(cam, spp, seed=11)
    assert np.isfinite(full[:, 0:7]).all() and (np.abs(full[:, 3:6]).sum(1) > 0).all()
    if mode == "lens":  # ray(origin, direction): time 0, origins spread over the defocus disk
        assert (full[:, 6] == 0).all() and len(np.unique(full[:, 0])) > 100
    tiles = quadrants(cam)
    for tl in (tiles, tiles[::-1]):
        rows = (pixel_index(cam, tl)[:, None] * spp + np.arange(spp)).reshape(-1)
        assert np.array_equal(ctx.camera_rays(cam, spp, seed=11, tiles=tl), full[rows]), mode
    dev = ctx.camera_rays(cam, spp, seed=11, device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), full)


# ---------------------------------------------------------------- 2. equivalence with the query path
def check_equals_query(ctx, desc, cam, family, trav=AUTO, seed=3):
    ctx.upload(desc)
    rays = ctx.camera_rays(cam, 1, seed=seed)
    dlen = np.sqrt((rays[:, 3:6] ** 2).sum(1))
    for prec in (F64, F32):
        assert ctx.trace_family(prec, trav) == family
        geom, ids = ctx.trace_rays(rays, precision=prec, traversal=trav, seed=seed)
        got = flat(ctx.render_aov(cam, 1, seed=seed, precision=prec, traversal=trav))
        hit = np.isfinite(geom[:, 0])
        assert np.array_equal(got["ids"], ids), (family, prec)
        assert np.array_equal(got["hit"], hit.astype(np.float64)), (family, prec)
        assert np.array_equal(got["normal"], geom[:, 4:7]), (family, prec)
        want = np.where(hit, np.where(hit, geom[:, 0], 0.0) * dlen, 0.0)
        if prec == F64:
            tol = 1e-9
        else:  # 8 x the error of t |d| in float32
            t32, d32 = geom[:, 0].astype(np.float32), rays[:, 3:6].astype(np.float32)
            f32 = np.where(hit, np.where(hit, t32, 0) * np.sqrt((d32 * d32).sum(1, dtype=np.float32)), 0)
            tol = 8 * relerr(f32, want)
        e = relerr(got["depth"], want)
        print(f"{family} precision {prec}: hits {hit.mean():.2f}, depth against t |d| rel err {e:.2e} (bound {tol:.2e})")
        assert e <= tol, (family, prec)
        assert 0.05 < hit.mean() <= 1.0
    return got


def test_equals_query_cornell_flat_and_linear(ctx):
    desc, cam, _, _ = scenes.cornell_box(width=32)
    check_equals_query(ctx, desc, cam, "FLAT")
    check_equals_query(ctx, desc, cam, "LINEAR", ORDERED)


def test_equals_query_volume(ctx):
    desc, cam, _, _ = scenes.cornell_box_with_volume(width=32)
    got = check_equals_query(ctx, desc, cam, "LINEAR")
    vol = got["ids"][:, 2] == abi.RT_OBJ_VOLUME  # the volume draws are the pixel's own: some rays end in the smoke
    assert 0.02 < vol.mean() < 0.9 and (got["normal"][vol] == [1.0, 0.0, 0.0]).all()


def test_equals_query_rtow_wide_lds(ctx):
    desc, cam, _, _ = scenes.rtow(width=64)
    assert (cam.image_width, cam.image_height) == (64, 36)
    check_equals_query(ctx, desc, cam, "WIDE_LDS")


def test_equals_query_heightfield_wide_hbm(ctx):
    desc, cam = field_scene()
    check_equals_query(ctx, desc, cam, "WIDE_HBM")


def test_equals_query_binary_bvh(ctx):
    desc, cam = instance_scene()
    got = check_equals_query(ctx, desc, cam, "STACK")
    assert len(set(got["ids"][:, 0])) >= 5  # box faces, the floor, the sphere, the background


@pytest.mark.parametrize("mode", ["orthonormal", "fisheye", "lens"])
def test_equals_query_other_cameras(ctx, mode):
    desc, _, _, _ = scenes.three_material_ball(width=64)
    check_equals_query(ctx, desc, ball_cameras()[mode], "LINEAR")


# ---------------------------------------------------------------- 3. and 5. the numpy brute force
def brute_scenes():
    c, cc = scenes.cornell_box(width=48), scenes.cornell_triangles(width=48)
    return {"cornell_box": (c[0], c[1], 4), "cornell_triangles": (cc[0], cc[1], 4), "heightfield": field_scene() + (1,)}


@pytest.fixture(scope="module")
def brute():
    """Per scene and spp: the rays' brute-force answer, computed once."""
    cache = {}

    def get(ctx, name, spp):
        if (name, spp) not in cache:
            desc, cam, _ = brute_scenes()[name]
            rays = ctx.camera_rays(cam, spp, seed=5)
            leaves = trace_ref.flatten(desc._owner, desc.world)
            cache[(name, spp)] = (desc, cam, rays, leaves, trace_ref.trace(leaves, rays, seed=5, eps=EPS32))
        return cache[(name, spp)]
    return get


@pytest.mark.parametrize("name", ["cornell_box", "cornell_triangles", "heightfield"])
def test_fp64_against_brute_force(ctx, brute, name):
    spp = brute_scenes()[name][2]
    desc, cam, rays, leaves, ref = brute(ctx, name, spp)
    ctx.upload(desc)
    want = aov_ref.features(desc, rays, ref, spp)
    got = flat(ctx.render_aov(cam, spp, seed=5, precision=F64))
    tight = trace_ref.trace(leaves, rays, seed=5, eps=1e-9)["near"].reshape(-1, spp).any(1)
    print(f"{name}: {int(tight.sum())} pixels with a ray near a boundary at 1e-9, hit share {want['hit'].mean():.2f}")
    assert tight.mean() <= 0.002
    ok = ~tight
    assert np.array_equal(got["hit"][ok], want["hit"][ok]) and np.array_equal(got["ids"][ok], want["ids"][ok])
    e = {k: relerr(got[k][ok], want[k][ok]) for k in ("albedo", "normal", "depth")}
    print(f"{name}: fp64 max rel err " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= 1e-9, e
    assert want["hit"].mean() > 0.3 and len(np.unique(want["albedo"], axis=0)) >= 2


@pytest.mark.parametrize("name", ["cornell_box", "cornell_triangles", "heightfield"])
def test_fp32_against_brute_force(ctx, brute, name):
    desc, cam, rays, leaves, ref = brute(ctx, name, 1)
    ctx.upload(desc)
    want = aov_ref.features(desc, rays, ref, 1)
    floor_ref = trace_ref.trace(leaves, rays, seed=5, dtype=np.float32)
    floor = aov_ref.features(desc, rays, floor_ref, 1, dtype=np.float32)
    got = flat(ctx.render_aov(cam, 1, seed=5, precision=F32))
    keep = ~ref["near"]
    print(f"{name}: {int((~keep).sum())} of {keep.size} rays near a boundary at {EPS32}")
    assert 1.0 - keep.mean() <= CAP32
    assert np.array_equal(got["hit"][keep], want["hit"][keep])
    for col, what in ((0, "object"), (3, "front")):
        assert np.array_equal(got["ids"][keep, col], want["ids"][keep, col]), what
    both = keep & (floor["ids"][:, 0] == want["ids"][:, 0])
    for k in ("albedo", "normal", "depth"):
        f, d = relerr(floor[k][both], want[k][both]), relerr(got[k][keep], want[k][keep])
        print(f"{name}: fp32 {k} rel err {d:.2e} (float32 formulas {f:.2e})")
        assert d <= 8 * f, (name, k, d, f)


# ---------------------------------------------------------------- 4. the oracle: camera + trace + u, v + texture
def check_albedo_is_oracle(ctx, desc, cam, what, spp=8, seed=9, front_only=True):
    """The oracle renders the clone whose materials are all lights with max_depth 1: a sample is then the texture at
    its first hit if that is a front face (material.h:211-215 emits on front faces only), the background on a miss.

    front_only: every hit is a front face (asserted through trace_rays(camera_rays)), so the oracle's image is the
    albedo channel, pixel for pixel. Otherwise (rtow_motion: the reference takes a moving sphere's normal about
    center_ = 0, sphere.h:69, so its face side is arbitrary -- 6.4 % of that frame's rays hit a back face, measured
    here) the oracle's image is the mean of the samples' albedo with the back-face samples at 0; the samples are
    taken one by one (spp = 1, first_sample = s) and that mean is checked for every scene, all-front ones too."""
    ctx.upload(desc)
    _, ids = ctx.trace_rays(ctx.camera_rays(cam, spp, seed=seed), precision=F64, seed=seed)
    back = float((ids[:, 3] == 0).mean())
    print(f"{what}: front-face hits {float((ids[:, 3] == 1).mean()):.3f}, back-face hits {back:.3f} of the rays")
    assert (ids[:, 3] == 1).mean() > 0.2, what
    want, _ = oracle.render(oracle.from_desc(aov_ref.as_lights(desc)), cam, spp, 1, seed=seed, mode=oracle.COUNTER)
    got = ctx.render_aov(cam, spp, seed=seed, precision=F64)
    one = [ctx.render_aov(cam, 1, seed=seed, precision=F64, first_sample=k) for k in range(spp)]
    assert relerr(np.mean([a["albedo"] for a in one], 0), got["albedo"]) <= 1e-14, what
    seen = np.mean([np.where((a["ids"][..., 3] == 0)[..., None], 0.0, a["albedo"]) for a in one], 0)
    e = relerr(seen, want)
    print(f"{what}: samples' albedo (back faces as 0) against the oracle, max rel err {e:.2e}")
    assert e <= 1e-9, what
    if front_only:
        assert back == 0.0, what
        e = relerr(got["albedo"], want)
        print(f"{what}: albedo against the oracle, max rel err {e:.2e}; "
              f"{len(np.unique(want.reshape(-1, 3), axis=0))} colours")
        assert e <= 1e-9, what
    else:
        assert back > 0.0, what
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 4
    return got


@pytest.mark.parametrize("mode", ["perspective", "orthonormal", "fisheye", "lens"])
def test_albedo_is_oracle_ball(ctx, mode):
    desc, _, _, _ = scenes.three_material_ball(width=64)
    check_albedo_is_oracle(ctx, desc, ball_cameras()[mode], "three_material_ball " + mode)


@pytest.mark.parametrize("name", ["rtow", "rtow_motion"])
def test_albedo_is_oracle_rtow(ctx, name):
    desc, cam, _, _ = scenes.SCENES[name](width=64)
    check_albedo_is_oracle(ctx, desc, cam, name, front_only=name != "rtow_motion")


def test_albedo_is_oracle_picture_on_a_sphere(ctx):
    s = SceneBuilder()
    rng = np.random.default_rng(8)
    pic = s.image(rng.uniform(0.05, 0.95, (4, 8, 3)))  # 8 wide, 4 high
    world = s.hlist([s.sphere((0, 0, 0), 1.0, s.lambertian(pic)), s.sphere((1.5, 0.2, 1.0), 0.4, s.metal(pic, 0.0))])
    desc = s.desc(world, background=s.solid((0.1, 0.2, 0.3)))
    cam = perspective(64, 16.0 / 9.0, (0.5, 1.5, -4), (0.3, 0, 0), 1, 40.0)
    got = check_albedo_is_oracle(ctx, desc, cam, "picture on a sphere")
    assert len(np.unique(got["albedo"].reshape(-1, 3), axis=0)) > 12  # several texels and their mixtures


# ---------------------------------------------------------------- 6. invariances, plumbing, errors
@pytest.fixture(scope="module")
def ball():
    desc, _, _, _ = scenes.three_material_ball(width=64)
    return desc, ball_cameras()["perspective"]


@pytest.mark.parametrize("prec", [F64, F32])
def test_tiling_and_sample_ranges(ctx, ball, prec):
    desc, cam = ball
    ctx.upload(desc)
    full = flat(ctx.render_aov(cam, 8, seed=4, precision=prec))
    tiles = quadrants(cam)
    for tl in (tiles, tiles[::-1]):
        got = ctx.render_aov(cam, 8, seed=4, precision=prec, tiles=tl)
        order = pixel_index(cam, tl)
        assert same(got, {k: full[k][order] for k in CHANNELS})
    a = flat(ctx.render_aov(cam, 4, seed=4, precision=prec))
    b = flat(ctx.render_aov(cam, 4, seed=4, precision=prec, first_sample=4))
    for k in ("albedo", "normal", "depth", "hit"):
        assert relerr(0.5 * (a[k] + b[k]), full[k]) <= 1e-14, k
    assert np.array_equal(a["ids"], full["ids"]) and not np.array_equal(a["albedo"], b["albedo"])
    assert 0 < (full["hit"] % 1 != 0).sum()  # edge pixels see both a sphere and the sky


def test_device_path_on_a_stream_is_the_host_path(ctx, ball):
    import torch
    desc, cam = ball
    ctx.upload(desc)
    for prec in (F64, F32):
        host = flat(ctx.render_aov(cam, 4, seed=6, precision=prec))
        stream = torch.cuda.Stream()
        dev = ctx.render_aov(cam, 4, seed=6, precision=prec, device=True, stream=stream)
        assert all(dev[k].is_cuda for k in CHANNELS) and dev["ids"].dtype == torch.int32
        stream.synchronize()
        assert same(flat({k: v.cpu().numpy() for k, v in dev.items()}), host)


def test_render_is_untouched_and_counters_advance(ctx, ball):
    desc, cam = ball
    ctx.upload(desc)
    before = [ctx.render(cam, 4, 8, seed=3, precision=p) for p in (F32, F64)]
    ctx.reset_counters()
    tiles = quadrants(cam)[:2]
    npix = sum(t[2] * t[3] for t in tiles)
    for k, prec in enumerate((F32, F64)):
        ctx.camera_rays(cam, 2, seed=3)  # no counter moves
        ctx.render_aov(cam, 3, seed=3, precision=prec, tiles=tiles)
        st = ctx.stats()
        assert st.segments == (k + 1) * npix * 3 and st.launches == k + 1
    after = [ctx.render(cam, 4, 8, seed=3, precision=p) for p in (F32, F64)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_errors_carry_a_message(ctx, ball):
    import torch
    desc, cam = ball
    fresh = rt_amd.Context(0)
    try:
        assert fresh.camera_rays(cam, 1).shape == (64 * 36, 8)  # needs no scene
        with pytest.raises(abi.RTError) as e:
            fresh.render_aov(cam, 1)
        assert e.value.status == abi.RT_ERR_NO_SCENE and "rt_scene_upload" in str(e.value)
    finally:
        fresh.close()
    ctx.upload(desc)
    bad = [dict(spp=0), dict(tiles=[(60, 0, 8, 8)]), dict(tiles=[(0, -1, 8, 8)]), dict(cam=aov_ref.copy_camera(cam, mode=4))]
    for kw in bad:
        for call in (ctx.camera_rays, ctx.render_aov):
            with pytest.raises(abi.RTError) as e:
                call(kw.get("cam", cam), kw.get("spp", 1), tiles=kw.get("tiles"))
            assert e.value.status == abi.RT_ERR_INVALID_ARGUMENT and len(str(e.value)) > len("rt status 1: "), kw
    for kw in (dict(precision=7), dict(traversal=5)):
        with pytest.raises(abi.RTError) as e:
            ctx.render_aov(cam, 1, **kw)
        assert e.value.status == abi.RT_ERR_INVALID_ARGUMENT and "unknown" in str(e.value)
    # null pointers, and device pointers off a 16-byte boundary
    tile = (abi.rt_tile * 1)(abi.rt_tile(0, 0, 4, 4))
    buf = torch.zeros(16 * 8 + 2, dtype=torch.float64, device="cuda")
    idb = torch.zeros(16 * 4 + 4, dtype=torch.int32, device="cuda")
    prm = abi.rt_aov_params(seed=1, spp=1, precision=F64, on_device=1)
    P = ctypes.c_void_p
    lib, INV = ctx.lib, abi.RT_ERR_INVALID_ARGUMENT
    calls = [lambda: lib.rt_camera_rays(ctx.h, ctypes.byref(cam), 1, 0, 1, tile, 1, P(buf.data_ptr() + 8), 1, None),
             lambda: lib.rt_camera_rays(ctx.h, ctypes.byref(cam), 1, 0, 1, tile, 1, None, 0, None),
             lambda: lib.rt_camera_rays(ctx.h, ctypes.byref(cam), 1, 0, 1, None, 1, P(buf.data_ptr()), 1, None),
             lambda: lib.rt_render_aov(ctx.h, ctypes.byref(cam), ctypes.byref(prm), tile, 1, P(buf.data_ptr() + 8),
                                       P(idb.data_ptr()), None),
             lambda: lib.rt_render_aov(ctx.h, ctypes.byref(cam), ctypes.byref(prm), tile, 1, P(buf.data_ptr()),
                                       P(idb.data_ptr() + 8), None),
             lambda: lib.rt_render_aov(ctx.h, ctypes.byref(cam), None, tile, 1, P(buf.data_ptr()), P(idb.data_ptr()), None),
             lambda: lib.rt_render_aov(ctx.h, None, ctypes.byref(prm), tile, 1, P(buf.data_ptr()), P(idb.data_ptr()), None)]
    # npix * spp = 2^31: refused before anything is sized by it
    big = aov_ref.copy_camera(cam, image_width=2048, image_height=2048)
    mega = (abi.rt_tile * 1)(abi.rt_tile(0, 0, 1024, 1024))
    many = abi.rt_aov_params(seed=1, spp=2048, precision=F64, on_device=1)
    calls += [lambda: lib.rt_camera_rays(ctx.h, ctypes.byref(big), 1, 0, 2048, mega, 1, P(buf.data_ptr()), 1, None),
              lambda: lib.rt_render_aov(ctx.h, ctypes.byref(big), ctypes.byref(many), mega, 1, P(buf.data_ptr()),
                                        P(idb.data_ptr()), None)]
    for k, call in enumerate(calls):
        assert call() == INV, k
        assert len(lib.rt_last_error(ctx.h)) > 0
    # and the aligned call right after them works
    assert lib.rt_render_aov(ctx.h, ctypes.byref(cam), ctypes.byref(prm), tile, 1, P(buf.data_ptr()), P(idb.data_ptr()),
                             None) == abi.RT_OK
    torch.cuda.synchronize()
