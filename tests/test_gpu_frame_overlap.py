"""Consecutive device-output renders overlap: their persistent launches alternate between two internal streams and
two sets of partial sums and dequeue heads (csrc/rt_plan.h lane_plan), while every resolve stays on the caller's
stream. Whatever is in flight, each frame must be the frame rendered alone -- RT_FRAME_OVERLAP=0 (one stream, as
before the lanes) and a sync after it -- bit for bit, and the counters must add up.

Every case is Cornell 64 x 64 in 16 x 16 tiles at 64 spp and depth 8, in both precisions."""
import time

import numpy as np
import pytest

import rt_amd
from rt_amd import abi, scenes
from rt_amd.scene import perspective

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
W, SPP, DEPTH = 64, 64, 8
SEEDS = (11, 12, 13, 14)
TILES = [(x, y, 16, 16) for y in range(0, W, 16) for x in range(0, W, 16)]
TILES_B = TILES[::-1][:9] + [(0, 0, 7, 5)]  # another pixel map: other tiles, another order, an odd one


def _torch():
    import torch
    return torch


def _dtype(prec):
    torch = _torch()
    return torch.float64 if prec == F64 else torch.float32


def _queue(ctx, cam, prec, seed, out, tiles=TILES, spp=SPP):
    """One device-output render on torch's current stream; returns without waiting."""
    torch = _torch()
    ctx.render_tiles(cam, ctx.params(spp, DEPTH, seed, prec), tiles, out.data_ptr(), 1,
                     torch.cuda.current_stream().cuda_stream)


def _buffer(prec, tiles=TILES):
    return _torch().full((sum(t[2] * t[3] for t in tiles), 3), -1.0, dtype=_dtype(prec), device="cuda:0")


def _alone(ctx, mp, cam, prec, seed, tiles=TILES, spp=SPP):
    """(the frame, its segments) rendered with the lanes off and waited for."""
    torch = _torch()
    mp.setenv("RT_FRAME_OVERLAP", "0")
    ctx.reset_counters()
    out = _buffer(prec, tiles)
    _queue(ctx, cam, prec, seed, out, tiles, spp)
    torch.cuda.synchronize()
    segs = ctx.stats().segments
    mp.delenv("RT_FRAME_OVERLAP")
    return out.cpu().numpy(), segs


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell():
    desc, cam, _, _ = scenes.cornell_box(width=W)
    return desc, cam


@pytest.fixture(scope="module")
def alone(ctx, cornell):
    """{precision: [(frame, segments) for SEEDS]}: each frame alone, lanes off. Computed once, never written."""
    desc, cam = cornell
    ctx.upload(desc)
    with pytest.MonkeyPatch.context() as mp:
        ref = {prec: [_alone(ctx, mp, cam, prec, s) for s in SEEDS] for prec in (F32, F64)}
    for frames in ref.values():
        for img, _ in frames:
            img.setflags(write=False)
    return ref


def _differs(a, b):
    return int((a != b).any(-1).sum())


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_four_frames_in_flight_are_the_frames_alone(ctx, cornell, alone, monkeypatch, prec):
    torch = _torch()
    desc, cam = cornell
    ctx.upload(desc)
    monkeypatch.delenv("RT_FRAME_OVERLAP", raising=False)
    outs = [_buffer(prec) for _ in SEEDS]
    torch.cuda.synchronize()
    for s, o in zip(SEEDS, outs):
        _queue(ctx, cam, prec, s, o)  # no sync between
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), alone[prec][k][0]), (k, _differs(o.cpu().numpy(), alone[prec][k][0]))


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_one_buffer_reused_with_stream_ordered_clones(ctx, cornell, alone, monkeypatch, prec):
    # the benchmark's pattern: a resolve must not run before the previous frame's reader of `out`
    torch = _torch()
    desc, cam = cornell
    ctx.upload(desc)
    monkeypatch.delenv("RT_FRAME_OVERLAP", raising=False)
    out = _buffer(prec)
    torch.cuda.synchronize()
    clones = []
    for s in SEEDS:
        _queue(ctx, cam, prec, s, out)
        clones.append(out.clone())  # on the same stream, right behind the render
    torch.cuda.synchronize()
    for k, c in enumerate(clones):
        assert np.array_equal(c.cpu().numpy(), alone[prec][k][0]), (k, _differs(c.cpu().numpy(), alone[prec][k][0]))


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_inputs_changing_between_frames_in_flight(ctx, cornell, monkeypatch, prec):
    torch = _torch()
    desc, cam = cornell
    cam_b = perspective(W, 1.0, (300, 250, -780), (278, 278, 0), 1, 40.0)
    desc_b = scenes.cornell_box_with_volume(width=W)[0]
    # (camera, tiles, spp) per frame: each differs from the one before in one input; the scene changes before frame 4
    frames = [(cam, TILES, SPP), (cam_b, TILES, SPP), (cam_b, TILES_B, SPP), (cam_b, TILES_B, 32), (cam_b, TILES_B, 32),
              (cam, TILES_B, 32), (cam, TILES, SPP)]
    want = []
    for k, (cm, tl, spp) in enumerate(frames):
        if k in (0, 4):
            ctx.upload(desc if k == 0 else desc_b)
        want.append(_alone(ctx, monkeypatch, cm, prec, 20 + k, tl, spp)[0])
    monkeypatch.delenv("RT_FRAME_OVERLAP", raising=False)
    outs = [_buffer(prec, tl) for _, tl, _ in frames]
    torch.cuda.synchronize()
    for k, (cm, tl, spp) in enumerate(frames):
        if k in (0, 4):
            ctx.upload(desc if k == 0 else desc_b)
        _queue(ctx, cm, prec, 20 + k, outs[k], tl, spp)
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), want[k]), (k, _differs(o.cpu().numpy(), want[k]))


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_passes_alternate_lanes_and_give_the_one_pass_image(ctx, cornell, alone, monkeypatch, prec):
    torch = _torch()
    desc, cam = cornell
    ctx.upload(desc)
    monkeypatch.delenv("RT_FRAME_OVERLAP", raising=False)
    item_bytes = 3 * (8 if prec == F64 else 4)
    monkeypatch.setenv("RT_PARTIAL_BUDGET", str(3 * item_bytes * W * W))  # three chunks per pass
    ctx.reset_counters()
    outs = [_buffer(prec) for _ in SEEDS[:2]]
    for s, o in zip(SEEDS, outs):
        _queue(ctx, cam, prec, s, o)  # two multi-pass calls in flight, one behind the other
    torch.cuda.synchronize()
    st = ctx.stats()
    assert st.passes > 2 * 2 and st.partial_bytes == 3 * item_bytes * W * W
    for k, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), alone[prec][k][0]), (k, _differs(o.cpu().numpy(), alone[prec][k][0]))


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_counters_add_up_and_kernel_time_stays_below_wall_time(ctx, cornell, alone, monkeypatch, prec):
    torch = _torch()
    desc, cam = cornell
    ctx.upload(desc)
    monkeypatch.delenv("RT_FRAME_OVERLAP", raising=False)
    outs = [_buffer(prec) for _ in SEEDS]
    _queue(ctx, cam, prec, 1, outs[0])  # (the inputs are on the device before the clock starts)
    ctx.set_timing(True)
    try:
        ctx.reset_counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s, o in zip(SEEDS, outs):
            _queue(ctx, cam, prec, s, o)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
    finally:
        ctx.set_timing(False)
    print(f"step_ms {st.step_ms:.4f} wall_ms {wall_ms:.4f} segments {st.segments}")
    assert st.segments == sum(segs for _, segs in alone[prec])
    assert st.iterations == len(SEEDS) and st.samples == len(SEEDS) * W * W * SPP
    assert 0 < st.step_ms <= wall_ms
