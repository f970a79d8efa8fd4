"""Item runs: the wave queue of the flat LL kernels hands out runs of L bulk items of one pixel (csrc/rt_plan.h RunPlan,
RT_ITEM_RUN=L). The run length is scheduling alone: whatever L, every item holds the same samples and writes its own
partial sum, so the image is the image of L = 1 and of the wavefront schedule bit for bit, and the segments traced are
the same.

Every case is a Cornell box 70 pixels wide at depth 8. At 24 spp the automatic layout of so small a frame has 21 bulk
items of 1 sample and 3 tail items of 1 per pixel (L = 4: five runs, one single bulk item, the tail items); with the
item count target off (RT_ITEMS_TARGET=1) 340 spp gives the benchmark's item sizes, 9 bulk items of 32 and 7 tail items
(test_items_of_the_benchmark_sizes: the one place a chunk inside a run is longer than a sample).

Which kernel ran is read back, not assumed: Context.last_run() is the run length of the units the last launch's queue
handed out, from the instantiated kernel -- L for the runs form, 1 for the kernel whose units are items."""
import numpy as np
import pytest

import rt_amd
from rt_amd import abi, scenes

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
W, SPP, DEPTH, SEED = 70, 24, 8, 7
RUNS = (1, 2, 4)
# a rank of two's share of the frame in 16-pixel tiles (the last column and row are 6 wide): every other tile
TILES = [(x, y, min(16, W - x), min(16, W - y)) for y in range(0, W, 16) for x in range(0, W, 16)][::2]


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


def _render(ctx, mp, cam, prec, run, spp=SPP, tiles=None, runs_kernel=True, **kw):
    """(image, segments, kernel tag) of one host-output render with RT_ITEM_RUN=run (None: unset). The launch must have
    taken the runs form at that run length, or, for 1, unset (a host-output render never overlaps) and `runs_kernel`
    False, the kernel whose units are items."""
    if run is None:
        mp.delenv("RT_ITEM_RUN", raising=False)
    else:
        mp.setenv("RT_ITEM_RUN", str(run))
    ctx.reset_counters()
    img = ctx.render(cam, spp, DEPTH, seed=SEED, precision=prec, tiles=tiles, **kw)
    assert ctx.last_run() == (run if runs_kernel and run else 1), (run, ctx.last_run())
    return img, ctx.stats().segments, ctx.last_kernel()


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_image_and_segments_do_not_depend_on_the_run_length(ctx, monkeypatch, prec):
    desc, cam, _, _ = scenes.cornell_box(width=W)
    ctx.upload(desc)
    base, segs, tag = _render(ctx, monkeypatch, cam, prec, 1)
    assert tag == f"FlatTrav<{'f64' if prec == F64 else 'f32'},1,1> persist"  # the kernel that takes runs
    assert np.isfinite(base).all() and base.max() > 0
    for run in RUNS[1:] + (None,):
        img, s, t = _render(ctx, monkeypatch, cam, prec, run)
        assert t == tag
        assert np.array_equal(img, base), (run, int((img != base).any(-1).sum()))
        assert s == segs, (run, s, segs)
    # the wavefront schedule: slots own items, no queue (and the flat program's general kernel)
    wave, _, t = _render(ctx, monkeypatch, cam, prec, 4, runs_kernel=False, segments_per_launch=4)
    assert t.endswith(" step")
    assert np.array_equal(wave, base), int((wave != base).any(-1).sum())


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_items_of_the_benchmark_sizes(ctx, monkeypatch, prec):
    desc, cam, _, _ = scenes.cornell_box(width=W)
    ctx.upload(desc)
    monkeypatch.setenv("RT_ITEMS_TARGET", "1")  # bulk items of 32 samples, tail items of 8
    base, segs, _ = _render(ctx, monkeypatch, cam, prec, 1, spp=340)
    for run in RUNS[1:]:
        img, s, _ = _render(ctx, monkeypatch, cam, prec, run, spp=340)
        assert np.array_equal(img, base), (run, int((img != base).any(-1).sum()))
        assert s == segs, (run, s, segs)


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_a_tile_subset_with_runs(ctx, monkeypatch, prec):
    # the pixel map: a unit's pixel is looked up once, at the run's first item
    desc, cam, _, _ = scenes.cornell_box(width=W)
    ctx.upload(desc)
    full, _, _ = _render(ctx, monkeypatch, cam, prec, 1)
    want = np.concatenate([full[y:y + h, x:x + w].reshape(-1, 3) for x, y, w, h in TILES])
    for run in RUNS:
        img, _, _ = _render(ctx, monkeypatch, cam, prec, run, tiles=TILES)
        assert np.array_equal(img, want), (run, int((img != want).any(-1).sum()))


def test_a_kernel_that_takes_no_runs_ignores_the_knob(ctx, monkeypatch):
    # Cornell with volumes renders with the linear program, whose queue hands out items whatever RT_ITEM_RUN says
    desc, cam = scenes.cornell_box_with_volume(width=W)[:2]
    ctx.upload(desc)
    base, segs, tag = _render(ctx, monkeypatch, cam, F32, 1)
    assert tag.startswith("LinearTrav<")
    img, s, _ = _render(ctx, monkeypatch, cam, F32, 4, runs_kernel=False)
    assert np.array_equal(img, base) and s == segs

