"""The flat LL kernels' sample and item ends (csrc/rt_kernels.hip shade kInPlace, next_item_dyn, begin_item): which
pixel and which samples an item is, and what a lane regenerates when its sample, its item or its work ends. A
mistake there is a wrong pixel or a wrong RNG key, not a crash, so every case compares whole images bit for bit:
the persistent schedule (the code under test) against the wavefront schedule (k_step, which shades with the general
code), over item sizes, a one-wave pool and tile lists; one fp64 frame is tied to the oracle.

The frame is the Cornell box at 70 x 70: 4,900 pixels are no multiple of the 64-item batch, so batches straddle
chunk boundaries; spp = 70 with items of 32 leaves a short last item.
"""
import numpy as np
import pytest

import oracle
import rt_amd
from rt_amd import abi, scenes
from rt_amd.tiling import pixel_index

pytestmark = pytest.mark.gpu

PRECISIONS = [abi.RT_PREC_F64, abi.RT_PREC_F32]
DEPTH, SEED = 6, 3
KSTEP = dict(segments_per_launch=3, pool_slots=777)  # the wavefront schedule
# edge tiles, partly 6 wide or high: 256 + 96 + 96 = 448 pixels, seven whole batches of 64 per chunk; with a fourth
# tile of 5 x 7, 483 pixels, which are no multiple of 64, so batches straddle the chunks of this call too
TILES = [(0, 0, 16, 16), (64, 48, 6, 16), (32, 64, 16, 6)]
TILE_LISTS = [TILES, TILES + [(48, 0, 5, 7)]]


@pytest.fixture(scope="module")
def frame():
    desc, cam, _, _ = scenes.cornell_box(width=70)
    ctx = rt_amd.Context(0)
    ctx.upload(desc)
    yield ctx, desc, cam
    ctx.close()


@pytest.fixture(scope="module")
def base(frame):
    """the persistent renders the cases share: (precision, spp) -> image, rendered once"""
    ctx, _, cam = frame
    got = {}

    def get(precision, spp):
        if (precision, spp) not in got:
            img = ctx.render(cam, spp, DEPTH, seed=SEED, precision=precision)
            img.setflags(write=False)
            got[precision, spp] = img
        return got[precision, spp]
    return get


@pytest.mark.parametrize("precision", PRECISIONS)
def test_schedule_invariance(frame, base, precision):
    ctx, _, cam = frame
    img = base(precision, 12)
    assert img.max() > 0
    # the wavefront schedule, and one wave running every item (its queue refills after every 64 items)
    for kw in (KSTEP, dict(pool_slots=64)):
        assert np.array_equal(ctx.render(cam, 12, DEPTH, seed=SEED, precision=precision, **kw), img), kw


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("samples_per_item", [0, 1, 3, 32, 70])  # 0: the automatic layout, bulk + tail items
def test_item_sizes(frame, base, precision, samples_per_item):
    ctx, _, cam = frame
    kw = dict(samples_per_item=samples_per_item) if samples_per_item else {}
    img = base(precision, 70) if not kw else ctx.render(cam, 70, DEPTH, seed=SEED, precision=precision, **kw)
    assert np.array_equal(img, ctx.render(cam, 70, DEPTH, seed=SEED, precision=precision, **kw, **KSTEP))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tiles", TILE_LISTS, ids=["448px", "483px"])
def test_tile_list(frame, base, precision, tiles):
    ctx, _, cam = frame
    full = base(precision, 70)
    packed = ctx.render(cam, 70, DEPTH, seed=SEED, precision=precision, tiles=tiles)
    want = full.reshape(-1, 3)[pixel_index(tiles, cam.image_width)]
    assert packed.shape == want.shape == (sum(t[2] * t[3] for t in tiles), 3)
    assert np.array_equal(packed, want)


def test_fp64_matches_oracle(frame, base):
    _, desc, cam = frame
    img = base(abi.RT_PREC_F64, 12).astype(np.float64)
    ref, _ = oracle.render(oracle.from_desc(desc), cam, 12, DEPTH, seed=SEED)
    assert np.all(np.abs(img - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref))), np.abs(img - ref).max()
