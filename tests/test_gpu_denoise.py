"""rt_denoise (Context.denoise): the variance-guided a-trous filter on the device.

The reference is the algorithm in numpy float64 (denoise_reference.py, pinned on the CPU by test_denoise_reference.py)
on its seeded frames: A (33 x 31: floor, box, miss rows, a partial-hit column, a zero-variance patch, a NaN pixel) and
the shapes 1 x 1, 70 x 1, 1 x 70, 65 x 5 (partial waves, a tile boundary, taps that all fall outside the image).

1. The device against the reference: every frame, both precisions, iterations 1, 5, 8, var given and NULL, demodulation
   on and off. fp64 within 1e-9 x max|ref|; fp32 RMSE below 1e-4 x max|ref| against the reference on the float-rounded
   inputs (the bounds of test_denoise_abi.py's host-loop comparison). A NaN only where the reference has one.
2. The same bits from the host-pointer call, the device-pointer call on a side stream and rgb_out == rgb_in; the fp64
   device output against the host loop over the same arithmetic.
3. The context's state around a call: no scene needed, renders around it unchanged, the counters, the scratch regrown,
   the refusals.
4. One end-to-end frame: a 16-spp Cornell box with its noise map and feature buffers, against a 4096-spp render.
"""
import ctypes
import math

import numpy as np
import pytest

import denoise_reference as R
import rt_amd
from rt_amd import abi, scenes

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
P = {F32: "f32", F64: "f64"}
DT = {F32: np.float32, F64: np.float64}
F64_BOUND, F32_BOUND = 1e-9, 1e-4
FRAMES = R.frames()
FRAMES32 = {k: R.rounded_to_float(v) for k, v in FRAMES.items()}
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


def inputs(name, prec):
    """(rgb in the precision's dtype, feat, var): what a call of that precision computes on."""
    fr = (FRAMES if prec == F64 else FRAMES32)[name]
    return fr["rgb"].astype(DT[prec]), fr["feat"], fr["var"]


def reference(name, prec, use_var, **kw):
    """The numpy reference on that precision's inputs, computed once and kept read-only."""
    key = (name, prec, use_var, tuple(sorted(kw.items())))
    if key not in _refs:
        fr = (FRAMES if prec == F64 else FRAMES32)[name]
        _refs[key] = R.denoise(fr["rgb"], fr["feat"], fr["var"] if use_var else None, **kw)
        _refs[key].setflags(write=False)
    return _refs[key]


def compare(out, ref, prec, what):
    """test_denoise_abi.py's two bounds, and a NaN only where the reference has one -> the largest deviation."""
    out = np.asarray(out, np.float64)
    assert out.shape == ref.shape, what
    assert np.array_equal(np.isnan(out), np.isnan(ref)), (what, np.argwhere(np.isnan(out) != np.isnan(ref))[:8])
    assert np.isfinite(out[~np.isnan(ref)]).all(), what
    scale = np.nanmax(np.abs(ref))
    diff = np.where(np.isnan(ref), 0.0, out - ref)
    dev = float(np.abs(diff).max() / scale)
    if prec == F64:
        assert dev < F64_BOUND, (what, dev)
    else:
        rmse = float(np.sqrt((diff ** 2).mean()) / scale)
        assert rmse < F32_BOUND, (what, rmse, dev)
    return dev


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("prec", (F32, F64), ids=P.get)
@pytest.mark.parametrize("name", list(FRAMES))
def test_device_matches_the_reference(ctx, name, prec):
    rgb, feat, var = inputs(name, prec)
    worst = 0.0
    for iterations in (1, 5, 8):
        for use_var in (True, False):
            for demodulate in (True, False):
                kw = dict(iterations=iterations, demodulate=demodulate)
                out = ctx.denoise(rgb, feat, var if use_var else None, **kw)
                assert out.dtype == DT[prec] and out.shape == rgb.shape
                worst = max(worst, compare(out, reference(name, prec, use_var, **kw), prec,
                                           (name, P[prec], iterations, use_var, demodulate)))
    print(f"{name} {P[prec]}: largest deviation {worst:.3g} x max|ref|")


@pytest.mark.parametrize("prec", (F32, F64), ids=P.get)
def test_a_nan_stays_only_where_the_reference_has_one(ctx, prec):
    # a NaN albedo cannot be repaired (the last pass multiplies by it): that pixel stays NaN in the reference, its
    # neighbours, whose variance the 3 x 3 mean poisons, are rebuilt; frame A's NaN colour is repaired as before
    fr = (FRAMES if prec == F64 else FRAMES32)["A"]
    feat = fr["feat"].copy()
    feat[20 * fr["W"] + 5, 1] = np.nan
    ref = R.denoise(fr["rgb"], feat, fr["var"])
    assert np.isnan(ref).any(-1).sum() == 1 and np.isnan(ref[20, 5]).any()
    compare(ctx.denoise(fr["rgb"].astype(DT[prec]), feat, fr["var"]), ref, prec, ("nan albedo", P[prec]))


def test_other_sigmas_and_eps(ctx):
    kw = dict(iterations=4, sigma_color=0.7, sigma_normal=0.2, sigma_depth=3.0, albedo_eps=0.05, color_eps=1e-5,
              depth_eps=0.0)
    for prec in (F32, F64):
        rgb, feat, var = inputs("A", prec)
        compare(ctx.denoise(rgb, feat, var, **kw), reference("A", prec, True, **kw), prec, ("sigmas", P[prec]))


# ------------------------------------------------------------------ 2. equal bits
def raw_call(ctx, prm, rgb_in, feat, var, rgb_out, stream):
    return ctx.lib.rt_denoise(ctx.h, ctypes.byref(prm), rgb_in, feat, var, rgb_out, stream)


def test_host_call_device_call_and_in_place_give_the_same_bits(ctx):
    import torch
    for prec in (F32, F64):
        rgb, feat, var = inputs("A", prec)
        host = ctx.denoise(rgb, feat, var)
        side = torch.cuda.Stream()
        t_rgb, t_feat, t_var = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rgb, feat, var))
        torch.cuda.synchronize()
        dev = ctx.denoise(t_rgb, t_feat.reshape(rgb.shape[0], -1, 8), t_var, stream=side)
        assert dev.is_cuda and dev.dtype == t_rgb.dtype and dev.shape == t_rgb.shape
        side.synchronize()
        assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True), P[prec]
        # rgb_out == rgb_in, on torch's current stream
        prm = abi.rt_denoise_params(width=rgb.shape[1], height=rgb.shape[0], iterations=5, precision=prec, on_device=1,
                                    flags=abi.RT_DENOISE_DEMODULATE, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0,
                                    albedo_eps=1e-2, color_eps=1e-8, depth_eps=1e-3)
        buf = t_rgb.clone()
        cur = torch.cuda.current_stream().cuda_stream
        assert raw_call(ctx, prm, buf.data_ptr(), t_feat.data_ptr(), t_var.data_ptr(), buf.data_ptr(), cur) == abi.RT_OK
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True), P[prec]
        # ... and with host pointers
        hbuf = rgb.copy()
        prm.on_device = 0
        assert raw_call(ctx, prm, hbuf.ctypes.data, feat.ctypes.data, var.ctypes.data, hbuf.ctypes.data,
                        None) == abi.RT_OK
        assert np.array_equal(hbuf, host, equal_nan=True), P[prec]


@pytest.mark.parametrize("name", list(FRAMES))
def test_fp64_device_output_against_the_host_loop(ctx, name):
    rgb, feat, var = inputs(name, F64)
    for use_var in (True, False):
        v = var if use_var else None
        loop = rt_amd.denoise_host(rgb, feat, v, iterations=8)
        compare(ctx.denoise(rgb, feat, v, iterations=8), loop, F64, (name, use_var))


# ------------------------------------------------------------------ 3. the context's state around a call
def test_needs_no_scene_and_regrows_its_scratch():
    c = rt_amd.Context(0)
    try:
        for name in ("1x1", "65x5", "A", "70x1"):  # growing, then smaller again
            rgb, feat, var = inputs(name, F64)
            compare(c.denoise(rgb, feat, var), reference(name, F64, True, iterations=5, demodulate=True), F64, name)
    finally:
        c.close()


def test_renders_around_a_call_are_bit_identical_and_the_counters(ctx):
    desc, cam, _, _ = scenes.cornell_box(width=24)
    ctx.upload(desc)
    for prec in (F32, F64):
        before = ctx.render(cam, 4, 4, seed=3, precision=prec)
        ctx.reset_counters()
        rgb, feat, var = inputs("A", prec)
        for iterations in (1, 3, 8):
            s0 = ctx.stats()
            ctx.denoise(rgb, feat, var, iterations=iterations)
            s1 = ctx.stats()
            assert s1.launches - s0.launches == iterations + 1
            assert (s1.segments, s1.samples, s1.passes) == (s0.segments, s0.samples, s0.passes)
        after = ctx.render(cam, 4, 4, seed=3, precision=prec)
        assert np.array_equal(before, after), P[prec]


def test_refusals_match_the_check(ctx):
    import torch
    lib, INV = ctx.lib, abi.RT_ERR_INVALID_ARGUMENT
    rgb, feat, var = inputs("65x5", F32)
    out = np.full_like(rgb, 7.0)

    def prm(**kw):
        base = dict(width=65, height=5, iterations=5, precision=F32, on_device=0, flags=abi.RT_DENOISE_DEMODULATE,
                    sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, albedo_eps=1e-2, color_eps=1e-8, depth_eps=1e-3)
        base.update(kw)
        return abi.rt_denoise_params(**base)

    launches = ctx.stats().launches
    for kw in (dict(width=0), dict(height=65536), dict(iterations=0), dict(iterations=9), dict(precision=2),
               dict(flags=2), dict(sigma_color=0.0), dict(sigma_normal=math.nan), dict(sigma_depth=math.inf),
               dict(albedo_eps=0.0), dict(color_eps=-1.0), dict(depth_eps=math.nan)):
        why = ctypes.create_string_buffer(256)
        assert lib.rt_denoise_check(ctypes.byref(prm(**kw)), why, len(why)) == INV
        assert raw_call(ctx, prm(**kw), rgb.ctypes.data, feat.ctypes.data, var.ctypes.data, out.ctypes.data, None) == INV
        assert lib.rt_last_error(ctx.h).decode() == why.value.decode() != "", kw
    for args in ((None, feat.ctypes.data, out.ctypes.data), (rgb.ctypes.data, None, out.ctypes.data),
                 (rgb.ctypes.data, feat.ctypes.data, None)):
        assert raw_call(ctx, prm(), args[0], args[1], None, args[2], None) == INV
    # device pointers off a 16-byte boundary, each of the four in turn
    t = [torch.zeros(65 * 5 * 8 + 2, dtype=torch.float64, device="cuda") for _ in range(4)]
    good = [x.data_ptr() for x in t]
    for k in range(4):
        ptrs = list(good)
        ptrs[k] += 8
        assert raw_call(ctx, prm(on_device=1, precision=F64), ptrs[0], ptrs[1], ptrs[2], ptrs[3], None) == INV, k
    assert (out == 7.0).all() and ctx.stats().launches == launches  # nothing launched, nothing written
    assert raw_call(ctx, prm(on_device=1, precision=F64), good[0], good[1], good[2], good[3], None) == abi.RT_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 4. one end-to-end frame
def test_a_16_spp_cornell_box_comes_out_closer_to_the_converged_image(ctx):
    """Cornell box 48 x 48, depth 8: render_adaptive with threshold 0 and max_spp 16 (the image and its noise map),
    render_aov at the same seed and spp, denoised with var = adaptive_variance, against a 4096-spp render. With the CPU
    oracle's renders of the same frame the reference gives MSE 0.0240 -> 0.0206 (ratio 0.86): the error is dominated by
    the 18 pixels of the light (radiance 15, its edge aliased at 16 spp), which no spatial filter repairs; off the
    light it is 0.00197 -> 0.00056 (ratio 0.28)."""
    desc, cam, _, _ = scenes.cornell_box(width=48)
    ctx.upload(desc)
    H, W = cam.image_height, cam.image_width
    floor = 0.01
    noisy = ctx.render_adaptive(cam, 16, 8, 0.0, batch=4, min_spp=8, step_spp=8, floor=floor, seed=5, precision=F32)
    aov = ctx.render_aov(cam, 16, seed=5, precision=F32)
    truth = np.asarray(ctx.render(cam, 4096, 8, seed=1005, precision=F32), np.float64)
    var = rt_amd.adaptive_variance(noisy, floor)
    feat = np.concatenate([aov["albedo"].reshape(-1, 3), aov["normal"].reshape(-1, 3), aov["depth"].reshape(-1, 1),
                           aov["hit"].reshape(-1, 1)], 1)
    mse = lambda img: float(((np.asarray(img, np.float64) - truth) ** 2).mean())
    off_light = (feat[:, 0:3].max(1) <= 1.0).reshape(H, W)
    mse_off = lambda img: float(((np.asarray(img, np.float64) - truth) ** 2)[off_light].mean())
    ref = R.denoise(noisy["rgb"], feat, var)
    assert mse(ref) < mse(noisy["rgb"]), (mse(ref), mse(noisy["rgb"]))  # the reference first
    out = ctx.denoise(noisy["rgb"], aov, var)
    print(f"Cornell 48 x 48, 16 spp: MSE noisy {mse(noisy['rgb']):.4g}, denoised {mse(out):.4g} (ratio "
          f"{mse(out) / mse(noisy['rgb']):.3f}), reference {mse(ref):.4g}; off the light noisy "
          f"{mse_off(noisy['rgb']):.4g}, denoised {mse_off(out):.4g} (ratio {mse_off(out) / mse_off(noisy['rgb']):.3f})")
    assert mse(out) < mse(noisy["rgb"]), (mse(out), mse(noisy["rgb"]))
    compare(out, ref, F32, "cornell")
