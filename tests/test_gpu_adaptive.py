"""rt_render_adaptive (Context.render_adaptive): adaptive sampling with a per-pixel noise estimate, on the device.

The reference is the algorithm in numpy (adaptive_reference.py) over batches rendered by the existing call:
item_means(k) = Context.render(cam, spp=4, first_sample=4k, samples_per_item=4), the sums the adaptive call's items
write, so that the estimator, the rounds, the compaction and the outputs are compared like for like. Frames are 33 x 31
(1023 pixels: partial waves and several blocks meet in the compaction), batch = 4, min_spp = step_spp = 8, max_spp = 64,
max_depth = 8 unless a case says otherwise; scenes and thresholds are adaptive_reference.CASES, pinned on the CPU by
test_adaptive_reference.py.

1. Against the reference algorithm, one scene per persistent family, both precisions.
2. threshold = 0 is a fixed-spp render with a noise map.   3. threshold = inf, and a black frame.
4. Round edges: the loop ends early; a round every pixel survives; a 1 x 1 image.
5. A pixel's outputs depend on (seed, pixel) and the parameters alone, bit for bit.
6. The context's state around a call.   7. The contract: refusals, counters, alignment.
"""
import ctypes
import math

import numpy as np
import pytest

import adaptive_reference as ref
import rt_amd
from rt_amd import abi

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
P = {F32: "f32", F64: "f64"}
BOTH = (F32, F64)
W, H, NPIX, DEPTH, SEED = ref.W, ref.H, ref.W * ref.H, ref.DEPTH, ref.SEED
MAX_SPP = 64
ROUNDS = dict(batch=4, min_spp=8, step_spp=8)


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(ctx):
    """(scene, zoom, precision, width, height) -> (desc, cam, the 16 batches' means (npix, 3) in float64): rendered once
    with the existing call, never changed."""
    cache = {}

    def get(name, prec, zoom=1.0, width=W, height=H):
        key = (name, prec, zoom, width, height)
        if key not in cache:
            desc, cam = ref.frame(name, zoom, width, height)
            ctx.upload(desc)
            items = []
            for k in range(MAX_SPP // 4):
                img = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec, first_sample=4 * k, samples_per_item=4)
                items.append(np.asarray(img, np.float64).reshape(-1, 3))
                items[-1].setflags(write=False)
            cache[key] = (desc, cam, items)
        return cache[key]
    return get


def adaptive(ctx, cam, threshold, prec, max_spp=MAX_SPP, depth=DEPTH, **kw):
    args = dict(ROUNDS, seed=SEED, precision=prec)
    args.update(kw)
    return ctx.render_adaptive(cam, max_spp, depth, threshold, **args)


def flat(out):
    return dict(rgb=np.asarray(out["rgb"]).reshape(-1, 3), spp=np.asarray(out["spp"]).reshape(-1),
                err=np.asarray(out["err"]).reshape(-1))


def within(a, b, tol):
    """|a - b| <= tol, a NaN only where the other is one."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a) | np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.where(nan, np.isnan(a) & np.isnan(b), np.abs(a - b) <= tol)


def check_against_reference(out, r, prec, what):
    """The call's outputs against the reference's, outside the comparison band (asserted small from the reference's
    side first). rgb: the device adds the same sums in the same order in double, so its mean is the reference's to
    1e-12 before the one rounding to the precision, which moves a float by at most 2^-24 of itself."""
    n = r["spp"].shape[0]
    assert r["band"].sum() <= 0.01 * n, (what, int(r["band"].sum()))
    ok = ~r["band"]
    spp, rgb, err = out["spp"].reshape(-1), out["rgb"].reshape(-1, 3), out["err"].reshape(-1)
    assert np.array_equal(spp[ok], r["spp"][ok]), (what, np.flatnonzero(spp != r["spp"])[:8])
    tol = 1e-12 * np.abs(r["rgb"]) + (2.0 ** -24 * np.abs(r["rgb"]) + 1e-45 if prec == F32 else 0.0)
    good = within(rgb, r["rgb"], tol)[ok]
    assert good.all(), (what, "rgb", np.argwhere(~good)[:8])
    e2, r2 = err * err, r["err"] * r["err"]
    good = within(e2, r2, 1e-12 + 1e-9 * r2)[ok]
    assert good.all(), (what, "err", np.argwhere(~good)[:8])
    assert rgb.dtype == (np.float64 if prec == F64 else np.float32) and spp.dtype == np.int32 and err.dtype == np.float64


# ------------------------------------------------------------------ 1. against the reference algorithm
@pytest.mark.parametrize("prec", BOTH, ids=P.get)
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_against_the_reference_algorithm(ctx, frames, name, prec):
    desc, cam, items = frames(name, prec)
    thr = ref.CASES[name]
    r = ref.run(lambda k: items[k], NPIX, thr)
    ctx.upload(desc)
    out = adaptive(ctx, cam, thr, prec)
    assert ctx.last_kernel() == rt_amd.plan_kernel(desc, cam, precision=prec)  # the render's kernel, unchanged
    assert out["rgb"].shape == (H, W, 3) and out["spp"].shape == (H, W) and out["err"].shape == (H, W)
    hist = np.bincount(out["spp"].reshape(-1) // 8, minlength=9)[1:]
    print(f"{name} {P[prec]}: pixels by rounds {hist.tolist()}, in the band {int(r['band'].sum())}")
    assert hist[0] > 0 and hist[-1] > 0 and hist[1:-1].sum() > 0  # a graded map: the compaction had work every round
    check_against_reference(out, r, prec, (name, P[prec]))


# ------------------------------------------------------------------ 2. threshold = 0
@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_threshold_zero_is_a_fixed_spp_render_with_a_noise_map(ctx, frames, prec):
    desc, cam, items = frames(ref.FULL_SCENE, prec, ref.FULL_ZOOM)  # every pixel of this frame has variance
    ctx.upload(desc)
    before = ctx.stats()
    out = adaptive(ctx, cam, 0.0, prec)
    after = ctx.stats()
    assert (out["spp"] == MAX_SPP).all()
    assert after.passes - before.passes == 8  # a round in which every pixel survives, seven times over
    assert after.samples - before.samples == NPIX * MAX_SPP
    assert (out["err"] > 0).all() and np.isfinite(out["err"]).all()
    check_against_reference(out, ref.run(lambda k: items[k], NPIX, 0.0), prec, "threshold 0")
    img = ctx.render(cam, MAX_SPP, DEPTH, seed=SEED, precision=prec, samples_per_item=4)
    a, b = np.asarray(out["rgb"], np.float64), np.asarray(img, np.float64)
    # the same 16 item sums, added in double and rounded once here, added in the precision there
    tol = 1e-12 * np.abs(b) if prec == F64 else 2e-6 * np.abs(b) + 1e-12
    assert (np.abs(a - b) <= tol).all(), float(np.abs(a - b).max())


# ------------------------------------------------------------------ 3. threshold = inf, a black frame
@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_threshold_inf_and_a_black_frame(ctx, frames, prec):
    desc, cam, items = frames("backlight", prec)
    ctx.upload(desc)
    before = ctx.stats()
    out = adaptive(ctx, cam, math.inf, prec)
    assert ctx.stats().passes - before.passes == 1
    assert (out["spp"] == 8).all() and np.isfinite(out["err"]).all() and out["err"].max() > 0
    check_against_reference(out, ref.run(lambda k: items[k], NPIX, math.inf), prec, "threshold inf")
    for thr in (0.0, 0.1):
        out = adaptive(ctx, cam, thr, prec, depth=0)
        assert (out["rgb"] == 0).all() and (out["err"] == 0).all() and (out["spp"] == 8).all()


# ------------------------------------------------------------------ 4. round edges
@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_the_loop_ends_when_the_last_survivors_stop(ctx, frames, prec):
    desc, cam, items = frames(ref.EARLY_SCENE, prec)
    r = ref.run(lambda k: items[k], NPIX, ref.EARLY_THRESHOLD)
    assert 2 <= len(r["rounds"]) < 8
    ctx.upload(desc)
    before = ctx.stats()
    out = adaptive(ctx, cam, ref.EARLY_THRESHOLD, prec)
    after = ctx.stats()
    check_against_reference(out, r, prec, "early end")
    if not r["band"].any():
        assert after.passes - before.passes == len(r["rounds"])  # no round after the count reached 0
        assert after.samples - before.samples == 8 * sum(r["rounds"])
    assert out["spp"].max() < MAX_SPP


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_a_one_pixel_image(ctx, frames, prec):
    for name, thr in (("backlight", 0.05), ("backlight", 0.5), ("chain", 0.0)):
        desc, cam, items = frames(name, prec, 0.2, 1, 1)
        ctx.upload(desc)
        out = adaptive(ctx, cam, thr, prec)
        assert out["rgb"].shape == (1, 1, 3) and out["spp"].shape == (1, 1)
        check_against_reference(out, ref.run(lambda k: items[k], 1, thr), prec, ("1 x 1", name, thr))


# ------------------------------------------------------------------ 5. independence, bit for bit
def packed_index(tiles):
    return np.concatenate([(np.arange(y, y + h)[:, None] * W + np.arange(x, x + w)[None, :]).reshape(-1)
                           for x, y, w, h in tiles])


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1), equal_nan=True)
               for k in ("rgb", "spp", "err"))


def pick(whole, idx):
    f = flat(whole)
    return {k: v[idx] for k, v in f.items()}


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
@pytest.mark.parametrize("name", ["backlight", "spheres_nl_hbm"])
def test_a_pixel_depends_on_its_key_and_the_parameters_alone(ctx, monkeypatch, name, prec):
    import torch
    desc, cam = ref.frame(name)
    thr = ref.CASES[name]
    ctx.upload(desc)
    whole = adaptive(ctx, cam, thr, prec)
    assert len(np.unique(whole["spp"])) >= 4
    halves = [(0, 0, W, 15), (0, 15, W, H - 15)]
    columns = [(0, 0, 16, H), (16, 0, W - 16, H)]
    scattered = [(20, 3, 13, 9), (0, 0, 1, 1), (5, 17, 9, 14), (W - 1, H - 1, 1, 1)]
    for tiles in (halves, halves[::-1], columns, columns[::-1], scattered, [(7, 9, 1, 1)]):
        part = adaptive(ctx, cam, thr, prec, tiles=tiles)
        assert part["rgb"].shape == (len(packed_index(tiles)), 3)
        assert same_bits(part, pick(whole, packed_index(tiles))), tiles
    # the device path, and a second identical call
    dev = adaptive(ctx, cam, thr, prec, device=True)
    assert dev["rgb"].is_cuda and dev["spp"].dtype == torch.int32 and dev["err"].dtype == torch.float64
    assert dev["rgb"].dtype == (torch.float64 if prec == F64 else torch.float32) and dev["rgb"].shape == (H, W, 3)
    assert same_bits({k: v.cpu().numpy() for k, v in dev.items()}, whole)
    assert same_bits(adaptive(ctx, cam, thr, prec), whole)
    # the partial-sum budget: one chunk a pass, four passes a round of 16 samples
    rounds16 = dict(min_spp=16, step_spp=16)
    base = adaptive(ctx, cam, thr, prec, **rounds16)
    before = ctx.stats()
    monkeypatch.setenv("RT_PARTIAL_BUDGET", "1")
    split = adaptive(ctx, cam, thr, prec, **rounds16)
    monkeypatch.delenv("RT_PARTIAL_BUDGET")
    passes = ctx.stats().passes - before.passes
    assert passes == 4 * (int(split["spp"].max()) // 16) >= 12
    assert same_bits(split, base)


# ------------------------------------------------------------------ 6. the context's state
@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_renders_around_a_call_are_unchanged(ctx, prec):
    import torch
    desc, cam = ref.frame("backlight")
    thr = ref.CASES["backlight"]
    ctx.upload(desc)
    T = [(3, 5, 7, 9), (0, 0, W, 4)]
    first = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec, tiles=T)
    whole = adaptive(ctx, cam, thr, prec)                 # another pixel map in between
    second = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec, tiles=T)
    part = adaptive(ctx, cam, thr, prec, tiles=T)         # the same tiles: the cached map has to survive the rounds
    third = ctx.render(cam, 4, DEPTH, seed=SEED, precision=prec, tiles=T)
    assert first.max() > 0 and np.array_equal(first, second) and np.array_equal(first, third)
    assert same_bits(part, pick(whole, packed_index(T)))
    # device-output renders queued back to back around the call: the overlap lanes are live on both sides of it
    dt = torch.float64 if prec == F64 else torch.float32
    n = len(packed_index(T))
    bufs = [torch.zeros((n, 3), dtype=dt, device=f"cuda:{ctx.device}") for _ in range(6)]
    prm = ctx.params(4, DEPTH, SEED, prec)
    stream = ctx._torch_stream(None, bufs[0].device)
    tl = abi.TileList(T)
    for b in bufs[:3]:
        ctx.render_tiles(cam, prm, tl, b.data_ptr(), True, stream)
    dev = adaptive(ctx, cam, thr, prec, device=True)
    for b in bufs[3:]:
        ctx.render_tiles(cam, prm, tl, b.data_ptr(), True, stream)
    torch.cuda.synchronize()
    for b in bufs:
        assert np.array_equal(b.cpu().numpy(), first)
    assert same_bits({k: v.cpu().numpy() for k, v in dev.items()}, whole)


# ------------------------------------------------------------------ 7. the contract
def params(**kw):
    base = dict(seed=SEED, max_spp=MAX_SPP, max_depth=DEPTH, precision=F64, traversal=abi.RT_TRAV_AUTO, on_device=0,
                threshold=0.1, floor=0.01, **ROUNDS)
    base.update(kw)
    return abi.rt_adaptive_params(**base)


def test_refused_arguments_launch_nothing_and_write_nothing(ctx):
    import torch
    desc, cam = ref.frame("backlight")
    ctx.upload(desc)
    tiles = abi.TileList([(2, 3, 4, 2)])
    rgb, spp, err = np.full((8, 3), -7.0), np.full(8, -7, np.int32), np.full(8, -7.0)
    drgb = torch.full((9, 3), -7.0, dtype=torch.float64, device=f"cuda:{ctx.device}")
    dspp = torch.full((12,), -7, dtype=torch.int32, device=drgb.device)
    derr = torch.full((9,), -7.0, dtype=torch.float64, device=drgb.device)

    def call(prm=None, cam_=cam, tl=tiles.arr, nt=1, out=None, h=None, no_prm=False):
        o = out or (rgb.ctypes.data, spp.ctypes.data, err.ctypes.data)
        return ctx.lib.rt_render_adaptive(ctx.h if h is None else h, ctypes.byref(cam_) if cam_ is not None else None,
                                          None if no_prm else ctypes.byref(prm or params()), tl, nt, o[0], o[1], o[2],
                                          None)
    before = ctx.stats()
    bad = abi.RT_ERR_INVALID_ARGUMENT
    assert ctx.lib.rt_render_adaptive(None, ctypes.byref(cam), ctypes.byref(params()), tiles.arr, 1, rgb.ctypes.data,
                                      spp.ctypes.data, err.ctypes.data, None) == bad
    assert call(cam_=None) == bad and call(no_prm=True) == bad and call(tl=None) == bad and call(nt=-1) == bad
    for k in range(3):  # no output may be NULL
        o = [rgb.ctypes.data, spp.ctypes.data, err.ctypes.data]
        o[k] = None
        assert call(out=tuple(o)) == bad, k
    for kw in (dict(batch=0), dict(step_spp=6), dict(min_spp=12), dict(max_spp=60), dict(min_spp=4, step_spp=4),
               dict(min_spp=72, max_spp=64), dict(max_depth=-1), dict(precision=2), dict(traversal=2),
               dict(threshold=-0.1), dict(threshold=math.nan), dict(floor=0.0), dict(floor=math.inf)):
        assert call(params(**kw)) == bad, kw
    # the render's camera and tile errors
    wide = abi.rt_camera_desc.from_buffer_copy(cam)
    wide.image_width = 70000
    empty = abi.rt_camera_desc.from_buffer_copy(cam)
    empty.image_height = 0
    mode = abi.rt_camera_desc.from_buffer_copy(cam)
    mode.mode = 9
    assert call(cam_=wide) == bad and call(cam_=empty) == bad and call(cam_=mode) == bad
    assert call(tl=abi.TileList([(30, 3, 4, 2)]).arr) == bad and call(tl=abi.TileList([(-1, 0, 2, 2)]).arr) == bad
    # misaligned device pointers, one at a time
    on = params(on_device=1)
    ptrs = (drgb.data_ptr(), dspp.data_ptr(), derr.data_ptr())
    for k, off in ((0, 8), (1, 4), (2, 8)):
        o = list(ptrs)
        o[k] += off
        assert call(on, out=tuple(o)) == bad, k
    after = ctx.stats()
    assert (after.launches, after.samples, after.segments, after.passes) == \
        (before.launches, before.samples, before.segments, before.passes)
    assert (rgb == -7.0).all() and (spp == -7).all() and (err == -7.0).all()
    torch.cuda.synchronize()
    assert bool((drgb == -7.0).all()) and bool((dspp == -7).all()) and bool((derr == -7.0).all())
    # no pixels: fine, and nothing is launched; the same arguments with pixels: fine
    assert call(nt=0) == abi.RT_OK and call(tl=abi.TileList([(2, 3, 0, 5)]).arr) == abi.RT_OK
    assert ctx.stats().launches == before.launches and (rgb == -7.0).all()
    assert call() == abi.RT_OK and (spp >= 8).all() and (spp <= MAX_SPP).all() and np.isfinite(rgb).all()
    assert call(on, out=ptrs) == abi.RT_OK
    torch.cuda.synchronize()
    assert np.array_equal(dspp[:8].cpu().numpy(), spp) and np.array_equal(derr[:8].cpu().numpy(), err)
    assert bool((dspp[8:] == -7).all()) and bool((derr[8:] == -7.0).all()) and bool((drgb[8:] == -7.0).all())


def test_no_scene():
    c = rt_amd.Context(0)
    try:
        _, cam = ref.frame("backlight")
        with pytest.raises(abi.RTError) as e:
            adaptive(c, cam, 0.1, F32)
        assert e.value.status == abi.RT_ERR_NO_SCENE
    finally:
        c.close()


@pytest.mark.parametrize("prec", BOTH, ids=P.get)
def test_counters(ctx, prec):
    desc, cam = ref.frame("instanced")
    ctx.upload(desc)
    ctx.reset_counters()
    out = adaptive(ctx, cam, ref.CASES["instanced"], prec)
    st = ctx.stats()
    total = int(out["spp"].sum())
    assert st.samples == total
    assert total <= st.segments <= total * DEPTH
    rounds = int(out["spp"].max()) // 8
    assert st.passes == rounds
    # a round: the path launch and the moments resolve of its one pass, then the select (three launches with the
    # compaction; the last possible round has no next list)
    assert st.launches == 5 * rounds - (2 if rounds == 8 else 0)
