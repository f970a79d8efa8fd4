"""rt_temporal (Context.temporal, TemporalAccumulator): reprojected frame accumulation on the device.

The reference is the algorithm in numpy float64 (temporal_reference.py, pinned on the CPU by
test_temporal_reference.py, which also shows that no decision on these frames is borderline) on its seeded sequences of
three frames: A (33 x 31, a sideways translation; NaN colours and a NaN history record), B (a yaw), C (a forward
dolly), D (byte-equal cameras), E (a backward dolly: points behind the camera before) and the shapes 1 x 1, 70 x 1,
1 x 70, 65 x 5 (partial waves, a tile boundary, taps outside the image).

1. The device against the reference: every sequence, both precisions, var and ids given and NULL, demodulation on and
   off, three chained calls; the images and the history's planes. fp64 within 1e-9 x max|ref|; fp32 RMSE below
   1e-4 x max|ref| against the reference on the float-rounded inputs (the bounds of test_temporal_abi.py's host-loop
   comparison). A NaN only where the reference has one; the ids exact, and the counts wherever they are whole numbers.
2. The same bits from the host-pointer call, the device-pointer call on a side stream and the call in place; the fp64
   device output against the host loop over the same arithmetic.
3. The context's state around a call: no scene needed, renders around it unchanged, the counters, the refusals.
4. Progressive rendering over first_sample, and a moving camera through TemporalAccumulator into Context.denoise,
   end to end on the Cornell box.
"""
import ctypes
import math

import numpy as np
import pytest

import denoise_reference as DR
import temporal_reference as R
import rt_amd
from rt_amd import abi, scenes

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
P = {F32: "f32", F64: "f64"}
DT = {F32: np.float32, F64: np.float64}
F64_BOUND, F32_BOUND = 1e-9, 1e-4
INV, UNS = abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_UNSUPPORTED
SEQS = R.sequences()
SEQS32 = {k: [R.rounded_to_float(f) for f in v] for k, v in SEQS.items()}
_refs = {}


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


def frames(name, prec):
    return (SEQS if prec == F64 else SEQS32)[name]


def poke_of(name):
    return R.NAN_HISTORY if name == "A" else None


def reference(name, prec, use_var=True, use_ids=True, **kw):
    """The numpy reference over the sequence on that precision's inputs, computed once."""
    key = (name, prec, use_var, use_ids, tuple(sorted(kw.items())))
    if key not in _refs:
        _refs[key] = R.run(frames(name, prec), use_var, use_ids, poke_of(name), **kw)
    return _refs[key]


def device_run(ctx, name, prec, use_var=True, use_ids=True, **kw):
    """Context.temporal (host pointers) over the sequence, as R.run runs the reference."""
    params = dict(R.DEFAULTS, **kw)
    outs, hist, prev = [], None, None
    for k, fr in enumerate(frames(name, prec)):
        out = ctx.temporal(fr["cam"], prev, fr["rgb"].astype(DT[prec]), fr["feat"], fr["var"] if use_var else None,
                           fr["ids"] if use_ids else None, hist, **params)
        hist, prev = out["hist"], fr["cam"]
        if k == 0 and poke_of(name) is not None:
            hist = hist.copy()
            R.poke_nan(hist, *poke_of(name), fr["W"], fr["H"], DT[prec])
        outs.append(out)
    return outs


def compare(out, ref, prec, what):
    """test_temporal_abi.py's two bounds, and a NaN only where the reference has one -> the largest deviation."""
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


def compare_call(out, ref, W, H, prec, what):
    """A call's images and its history's planes against the reference's -> the largest deviation. The ids are exact;
    so is a count wherever the reference's is a whole number (a weighted mean of equal small counts is exact in any
    precision; a mean of unequal ones is a fraction, compared like the colours)."""
    h, rh = R.unpack_history(out["hist"], W, H, DT[prec]), ref["hist"]
    assert np.array_equal(h["id"], rh["id"]), what
    whole = rh["N"] == np.round(rh["N"])
    assert np.array_equal(h["N"][whole], rh["N"][whole]), what
    assert np.array_equal(np.asarray(out["count"], np.float64), h["N"]), what
    devs = [compare(out["rgb"], ref["rgb"], prec, (what, "rgb")), compare(out["var"], ref["var"], prec, (what, "var")),
            compare(h["N"], rh["N"], prec, (what, "N"))]
    for key in ("c", "v", "n", "z"):
        devs.append(compare(h[key], rh[key], prec, (what, key)))
    return max(devs)


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("prec", (F32, F64), ids=P.get)
@pytest.mark.parametrize("name", list(SEQS))
def test_device_matches_the_reference(ctx, name, prec):
    W, H = SEQS[name][0]["W"], SEQS[name][0]["H"]
    worst = 0.0
    for use_var in (True, False):
        for use_ids in (True, False):
            for demodulate in (True, False):
                refs = reference(name, prec, use_var, use_ids, demodulate=demodulate)
                outs = device_run(ctx, name, prec, use_var, use_ids, demodulate=demodulate)
                for k in range(3):
                    assert outs[k]["rgb"].dtype == DT[prec] and outs[k]["var"].dtype == np.float64
                    worst = max(worst, compare_call(outs[k], refs[k], W, H, prec,
                                                    (name, P[prec], use_var, use_ids, demodulate, k)))
    print(f"{name} {P[prec]}: largest deviation {worst:.3g} x max|ref|")


def test_other_parameters(ctx):
    kw = dict(alpha_min=0.2, max_history=2, depth_tol=0.03, normal_cos=0.5, min_weight=0.6, albedo_eps=0.05)
    for prec in (F32, F64):
        refs, outs = reference("C", prec, **kw), device_run(ctx, "C", prec, **kw)
        for k in range(3):
            compare_call(outs[k], refs[k], 33, 31, prec, ("C", P[prec], k))
        assert outs[2]["count"].max() == 2.0


@pytest.mark.parametrize("prec", (F32, F64), ids=P.get)
def test_byte_equal_cameras_give_the_running_mean(ctx, prec):
    fr = frames("D", prec)
    hist = None
    tol = 1e-12 if prec == F64 else 1e-6
    for k in range(3):
        out = ctx.temporal(fr[0]["cam"], fr[0]["cam"], fr[k]["rgb"].astype(DT[prec]), fr[0]["feat"], fr[k]["var"], None,
                           hist, **dict(R.DEFAULTS, alpha_min=0.0))
        hist = out["hist"]
        mean = np.mean([f["rgb"] for f in fr[:k + 1]], 0)
        var = np.mean([f["var"] for f in fr[:k + 1]], 0) / (k + 1)
        assert np.abs(out["rgb"] - mean).max() <= tol * np.abs(mean).max()
        assert np.abs(out["var"] - var).max() <= tol * var.max()
        assert (out["count"] == k + 1).all()


# ------------------------------------------------------------------ 2. equal bits
def raw_call(ctx, prm, cam, prev, rgb_in, feat, ids, var, hist_in, hist_out, rgb_out, var_out, stream):
    return ctx.lib.rt_temporal(ctx.h, ctypes.byref(prm), ctypes.byref(cam), None if prev is None else ctypes.byref(prev),
                               rgb_in, feat, ids, var, hist_in, hist_out, rgb_out, var_out, stream)


def make_params(W, H, prec, on_device, **kw):
    d = dict(R.DEFAULTS, **kw)
    return abi.rt_temporal_params(width=W, height=H, precision=prec, on_device=on_device,
                                  flags=abi.RT_TEMPORAL_DEMODULATE if d["demodulate"] else 0,
                                  max_history=d["max_history"], alpha_min=d["alpha_min"], depth_tol=d["depth_tol"],
                                  normal_cos=d["normal_cos"], min_weight=d["min_weight"], albedo_eps=d["albedo_eps"])


def test_host_call_device_call_and_in_place_give_the_same_bits(ctx):
    import torch
    for prec in (F32, F64):
        fr = frames("A", prec)
        host = device_run(ctx, "A", prec)
        side = torch.cuda.Stream()
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        first = host[0]["hist"].copy()
        R.poke_nan(first, *R.NAN_HISTORY, 33, 31, DT[prec])
        t_rgb, t_feat, t_var, t_ids, t_hist = (cuda(a) for a in (fr[1]["rgb"].astype(DT[prec]), fr[1]["feat"],
                                                                 fr[1]["var"], fr[1]["ids"], first))
        torch.cuda.synchronize()
        # the second frame with device pointers on a side stream
        dev = ctx.temporal(fr[1]["cam"], fr[0]["cam"], t_rgb, t_feat.reshape(31, 33, 8), t_var, t_ids.reshape(31, 33, 4),
                           t_hist, stream=side, **R.DEFAULTS)
        assert dev["rgb"].is_cuda and dev["rgb"].dtype == t_rgb.dtype and dev["hist"].dtype == torch.uint8
        side.synchronize()
        for key in ("rgb", "var", "hist", "count"):
            assert np.array_equal(dev[key].cpu().numpy(), host[1][key], equal_nan=True), (P[prec], key)
        # rgb_out == rgb_in and var_out == var, on torch's current stream
        prm = make_params(33, 31, prec, 1)
        buf, vbuf, hout = t_rgb.clone(), t_var.clone(), torch.empty_like(t_hist)
        cur = torch.cuda.current_stream().cuda_stream
        assert raw_call(ctx, prm, fr[1]["cam"], fr[0]["cam"], buf.data_ptr(), t_feat.data_ptr(), t_ids.data_ptr(),
                        vbuf.data_ptr(), t_hist.data_ptr(), hout.data_ptr(), buf.data_ptr(), vbuf.data_ptr(),
                        cur) == abi.RT_OK
        torch.cuda.synchronize()
        for got, key in ((buf, "rgb"), (vbuf, "var"), (hout, "hist")):
            assert np.array_equal(got.cpu().numpy().reshape(host[1][key].shape), host[1][key], equal_nan=True), (P[prec], key)
        # ... and with host pointers
        hbuf, hvar, hhist = fr[1]["rgb"].astype(DT[prec]), fr[1]["var"].copy(), np.empty_like(first)
        prm.on_device = 0
        assert raw_call(ctx, prm, fr[1]["cam"], fr[0]["cam"], hbuf.ctypes.data, fr[1]["feat"].ctypes.data,
                        fr[1]["ids"].ctypes.data, hvar.ctypes.data, first.ctypes.data, hhist.ctypes.data,
                        hbuf.ctypes.data, hvar.ctypes.data, None) == abi.RT_OK
        for got, key in ((hbuf, "rgb"), (hvar, "var"), (hhist, "hist")):
            assert np.array_equal(got, host[1][key], equal_nan=True), (P[prec], key)
        # var_out == NULL leaves the rest as it is
        hbuf, hhist = fr[1]["rgb"].astype(DT[prec]), np.empty_like(first)
        assert raw_call(ctx, prm, fr[1]["cam"], fr[0]["cam"], hbuf.ctypes.data, fr[1]["feat"].ctypes.data,
                        fr[1]["ids"].ctypes.data, fr[1]["var"].ctypes.data, first.ctypes.data, hhist.ctypes.data,
                        hbuf.ctypes.data, None, None) == abi.RT_OK
        assert np.array_equal(hbuf, host[1]["rgb"], equal_nan=True) and np.array_equal(hhist, host[1]["hist"])


@pytest.mark.parametrize("name", list(SEQS))
def test_fp64_device_output_against_the_host_loop(ctx, name):
    fr = SEQS[name]
    W, H = fr[0]["W"], fr[0]["H"]
    for use_var, use_ids in ((True, True), (False, False)):
        dev = device_run(ctx, name, F64, use_var, use_ids)
        hist, prev = None, None
        for k, f in enumerate(fr):
            loop = rt_amd.temporal_host(f["cam"], prev, f["rgb"], f["feat"], f["var"] if use_var else None,
                                        f["ids"] if use_ids else None, hist, **R.DEFAULTS)
            hist, prev = loop["hist"], f["cam"]
            if k == 0 and poke_of(name) is not None:
                hist = hist.copy()
                R.poke_nan(hist, *poke_of(name), W, H, np.float64)
            ref = dict(rgb=loop["rgb"], var=loop["var"], hist=R.unpack_history(loop["hist"], W, H, np.float64))
            compare_call(dev[k], ref, W, H, F64, (name, use_var, use_ids, k))


# ------------------------------------------------------------------ 3. the context's state around a call
def test_needs_no_scene_and_regrows_its_staging():
    c = rt_amd.Context(0)
    try:
        for name in ("1x1", "65x5", "A", "70x1"):  # growing, then smaller again
            refs, outs = reference(name, F64), device_run(c, name, F64)
            for k in range(3):
                compare_call(outs[k], refs[k], SEQS[name][0]["W"], SEQS[name][0]["H"], F64, (name, k))
    finally:
        c.close()


def test_renders_around_a_call_are_bit_identical_and_the_counters(ctx):
    desc, cam, _, _ = scenes.cornell_box(width=24)
    ctx.upload(desc)
    for prec in (F32, F64):
        before = ctx.render(cam, 4, 4, seed=3, precision=prec)
        ctx.reset_counters()
        hist, prev = None, None
        for fr in frames("A", prec):
            s0 = ctx.stats()
            out = ctx.temporal(fr["cam"], prev, fr["rgb"].astype(DT[prec]), fr["feat"], fr["var"], fr["ids"], hist,
                               **R.DEFAULTS)
            hist, prev = out["hist"], fr["cam"]
            s1 = ctx.stats()
            assert s1.launches - s0.launches == 1
            assert (s1.segments, s1.samples, s1.passes, s1.iterations) == (s0.segments, s0.samples, s0.passes, s0.iterations)
        after = ctx.render(cam, 4, 4, seed=3, precision=prec)
        assert np.array_equal(before, after), P[prec]


def test_refusals_match_the_check_and_write_nothing(ctx):
    import torch
    lib = ctx.lib
    fr = SEQS32["65x5"]
    cam, prev = fr[1]["cam"], fr[0]["cam"]
    rgb, feat, var, ids = fr[1]["rgb"].astype(np.float32), fr[1]["feat"], fr[1]["var"], fr[1]["ids"]
    first = ctx.temporal(prev, None, fr[0]["rgb"].astype(np.float32), fr[0]["feat"], fr[0]["var"], fr[0]["ids"])["hist"]
    out, vout, hout = np.full_like(rgb, 7.0), np.full_like(var, 7.0), np.full_like(first, 7)
    launches = ctx.stats().launches

    def call(prm, cam=cam, prev=prev, rgb_in=rgb.ctypes.data, f=feat.ctypes.data, hin=first.ctypes.data,
             ho=hout.ctypes.data, ro=out.ctypes.data):
        return raw_call(ctx, prm, cam, prev, rgb_in, f, ids.ctypes.data, var.ctypes.data, hin, ho, ro, vout.ctypes.data, None)

    def checked(prm, cam, prev):
        why = ctypes.create_string_buffer(256)
        st = lib.rt_temporal_check(ctypes.byref(prm), ctypes.byref(cam), ctypes.byref(prev), why, len(why))
        return st, why.value.decode()

    for kw in (dict(width=0), dict(height=65536), dict(precision=2), dict(flags=2), dict(max_history=0),
               dict(alpha_min=1.5), dict(alpha_min=math.nan), dict(depth_tol=0.0), dict(depth_tol=math.inf),
               dict(normal_cos=2.0), dict(min_weight=1.0), dict(albedo_eps=0.0), dict(albedo_eps=-1.0)):
        prm = make_params(65, 5, F32, 0)
        for key, val in kw.items():
            setattr(prm, key, val)
        st, why = checked(prm, cam, prev)
        assert st == INV and call(prm) == INV
        assert lib.rt_last_error(ctx.h).decode() == why != "", kw
    prm = make_params(65, 5, F32, 0)
    # cameras that differ and are not both perspective cameras of the image's size
    lens = abi.rt_camera_desc()
    ctypes.memmove(ctypes.byref(lens), ctypes.byref(cam), ctypes.sizeof(lens))
    lens.mode = abi.RT_CAM_LENS
    other = R.camera(64, 5, (0.0, 1.2, 0.0), (0.2, 0.55, -3.5))
    for a, b in ((lens, prev), (cam, lens), (other, prev), (cam, other)):
        st, why = checked(prm, a, b)
        assert st == UNS and call(prm, cam=a, prev=b) == UNS
        assert lib.rt_last_error(ctx.h).decode() == why != ""
    # null pointers, a history without its camera, histories that overlap
    assert call(prm, rgb_in=None) == INV and call(prm, f=None) == INV and call(prm, ho=None) == INV
    assert call(prm, ro=None) == INV and call(prm, prev=None) == INV
    assert call(prm, ho=first.ctypes.data) == INV and call(prm, ho=first.ctypes.data + first.nbytes - 1) == INV
    assert lib.rt_last_error(ctx.h).decode() == "hist_in and hist_out overlap"
    # device pointers off a 16-byte boundary, each of the eight in turn
    # (each array as long as an fp64 history and two doubles more, so that the two histories cannot overlap and the
    # shifted pointer stays inside its array)
    nbytes = int(lib.rt_temporal_history_bytes(65, 5, F64))
    assert nbytes == 65 * 5 * 76
    t = [torch.zeros(nbytes // 8 + 2, dtype=torch.float64, device="cuda") for _ in range(8)]
    good = [x.data_ptr() for x in t]
    assert all(p % 16 == 0 for p in good)
    dprm = make_params(65, 5, F64, 1)
    for k in range(8):
        ptrs = list(good)
        ptrs[k] += 8
        assert raw_call(ctx, dprm, cam, prev, *ptrs, None) == INV, k
        assert lib.rt_last_error(ctx.h).decode() == "device pointers must be 16-byte aligned", k
    assert (out == 7.0).all() and (vout == 7.0).all() and (hout == 7).all()  # nothing written
    assert ctx.stats().launches == launches  # nothing launched
    assert call(prm) == abi.RT_OK and not (out == 7.0).any()


# ------------------------------------------------------------------ 4. end to end
def feat_rows(aov):
    return np.concatenate([aov["albedo"].reshape(-1, 3), aov["normal"].reshape(-1, 3), aov["depth"].reshape(-1, 1),
                           aov["hit"].reshape(-1, 1)], 1)


def test_progressive_rendering_over_first_sample(ctx):
    """Cornell box 48 x 48, depth 8, fp64: 8 frames of 16 spp, frame k samples [16 k, 16 k + 16), accumulated with
    byte-equal cameras, alpha_min = 0 and normal_cos = -1. After frame k the output is the mean of the k frames and count == k; frame 8
    is the 128-spp render at the same item size, of which only the grouping of the sum differs."""
    desc, cam, _, _ = scenes.cornell_box(width=48)
    ctx.upload(desc)
    aov = ctx.render_aov(cam, 16, seed=5, precision=F64)
    # (normal_cos = -1: the guides are means over 16 samples, and an edge pixel's mean normal is shorter than 1)
    acc = rt_amd.TemporalAccumulator(ctx, alpha_min=0.0, max_history=64, normal_cos=-1.0)
    total, seen = np.zeros((48, 48, 3)), []
    for k in range(8):
        frame = ctx.render(cam, 16, 8, seed=5, precision=F64, first_sample=16 * k, samples_per_item=16)
        total += frame
        out = acc.push(cam, frame, aov)
        mean = total / (k + 1)
        assert np.abs(out["rgb"] - mean).max() <= 1e-9 * np.abs(mean).max(), k
        assert (out["count"] == k + 1).all(), k
        if k >= 2:  # the accumulator's two history buffers ping-pong
            assert out["hist"] is seen[k & 1]
        else:
            seen.append(out["hist"])
    whole = ctx.render(cam, 128, 8, seed=5, precision=F64, samples_per_item=16)
    dev = float(np.abs(out["rgb"] - whole).max() / np.abs(whole).max())
    print(f"progressive: 8 x 16 spp against 128 spp, largest deviation {dev:.3g} x max")
    assert dev <= 1e-9


def test_a_moving_camera_comes_out_closer_to_the_converged_image(ctx):
    """Cornell box 48 x 48, depth 8, fp32: the camera takes 8 steps of 2 units sideways; each frame is render_adaptive
    at 16 spp with threshold 0 (the image and its noise map) and render_aov, pushed through TemporalAccumulator; the
    last output against a 4096-spp render of the last camera.

    The step. As in test_gpu_denoise.py, this frame's MSE is dominated by the pixels along the edge of the light
    (radiance 15 against 0.3 beside it, aliased at 16 spp: single pixels carry squared errors of 10 to 50). A history
    tap across that edge is not rejected by depth, normal or id (the ceiling and the light share a plane, and a pixel's
    id is its first sample's), so the whole-frame figure falls only while such a pixel's history is mostly its own: a
    step of 2 units is 0.12 pixels at the light and 0.10 at the back wall, a slow pan. With the numpy reference on the
    frames of this test: whole frame 0.0191 -> 0.0153, off the light 0.00159 -> 0.00031; at 6 units a step (0.35
    pixels) off the light 0.00159 -> 0.00025, but the whole frame 0.0191 -> 0.0273. Measured on an MI355X: DESIGN.md,
    "Temporal accumulation"."""
    desc, cam0, _, _ = scenes.cornell_box(width=48)
    ctx.upload(desc)
    H, W = cam0.image_height, cam0.image_width
    floor = 0.01
    acc = rt_amd.TemporalAccumulator(ctx)
    seq, ref_hist, ref_prev, ref = [], None, None, None
    for k in range(8):
        cam = abi.rt_camera_desc()
        ctypes.memmove(ctypes.byref(cam), ctypes.byref(cam0), ctypes.sizeof(cam))
        for a in range(3):
            cam.pos[a] = cam0.pos[a] + 2.0 * (k - 7) * cam0.right[a]
        noisy = ctx.render_adaptive(cam, 16, 8, 0.0, batch=4, min_spp=8, step_spp=8, floor=floor, seed=5 + k, precision=F32)
        aov = ctx.render_aov(cam, 16, seed=5 + k, precision=F32)
        var = rt_amd.adaptive_variance(noisy, floor)
        out = acc.push(cam, noisy["rgb"], aov, var)
        # the reference on the same inputs (what an fp32 call computes on: the guides rounded to float)
        feat32 = feat_rows(aov).astype(np.float32).astype(np.float64)
        var32 = var.astype(np.float32).astype(np.float64)
        ref = R.temporal(cam, ref_prev, noisy["rgb"].astype(np.float64), feat32, var32, aov["ids"].reshape(-1, 4),
                         ref_hist, alpha_min=0.05, max_history=64, depth_tol=0.05, normal_cos=0.9, min_weight=0.25)
        ref_hist, ref_prev = ref["hist"], cam
        seq.append((cam, noisy, aov, var))
    info = ref["info"]
    print("reference margins of the last frame: " + ", ".join(f"{k} {info[k]:.3g}" for k in info if k.startswith("margin")))
    cam, noisy, aov, var = seq[-1]
    truth = np.asarray(ctx.render(cam, 4096, 8, seed=1005, precision=F32), np.float64)
    mse = lambda img: float(((np.asarray(img, np.float64) - truth) ** 2).mean())
    m_noisy, m_ref, m_out = mse(noisy["rgb"]), mse(ref["rgb"]), mse(out["rgb"])
    assert m_ref < m_noisy, (m_ref, m_noisy)  # the reference first
    share = float((out["count"] > 1).mean())
    off_light = (feat_rows(aov)[:, 0:3].max(1) <= 1.0).reshape(H, W)
    mse_off = lambda img: float(((np.asarray(img, np.float64) - truth) ** 2)[off_light].mean())
    dn_noisy = ctx.denoise(noisy["rgb"], aov, var)
    dn_out = ctx.denoise(out["rgb"], aov, out["var"])
    ref_dn = DR.denoise(ref["rgb"], feat_rows(aov), ref["var"])
    ref_dn_noisy = DR.denoise(noisy["rgb"], feat_rows(aov), var)
    print(f"Cornell 48 x 48, 8 frames of 16 spp, moving camera: MSE noisy {m_noisy:.4g}, accumulated {m_out:.4g} (ratio "
          f"{m_out / m_noisy:.3f}), reference {m_ref:.4g}; pixels with count > 1: {share:.3f}; denoised alone "
          f"{mse(dn_noisy):.4g}, accumulated then denoised {mse(dn_out):.4g} (reference {mse(ref_dn_noisy):.4g}, "
          f"{mse(ref_dn):.4g}); off the light: noisy {mse_off(noisy['rgb']):.4g}, accumulated {mse_off(out['rgb']):.4g}, "
          f"denoised alone {mse_off(dn_noisy):.4g}, accumulated then denoised {mse_off(dn_out):.4g}")
    assert m_out < m_noisy, (m_out, m_noisy)
    compare(out["rgb"], ref["rgb"], F32, "moving camera")
    if mse(ref_dn) < mse(ref_dn_noisy):  # the reference shows the ordering: accumulation helps the denoiser too
        assert mse(dn_out) < mse(dn_noisy), (mse(dn_out), mse(dn_noisy))
