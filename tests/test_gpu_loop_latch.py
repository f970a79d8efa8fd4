"""The persistent kernels' segment loop (csrc/rt_kernels.hip persist_body): a segment is counted before shade and the
segment cap is tested after it, in the flat, linear and binary-BVH families. Reordering the two must move neither the
segment count rt_stats reports (a lane that shade retires has traced its last segment) nor a bit of the image.

Every frame is 70 pixels wide at 12 spp, depth 6, seed 3: 4,900 Cornell pixels are several blocks and no multiple
of the 64-item batch. The segment counts were recorded from the build before the loop changed (the parent commit's
library, same calls) and are constants here; the images are compared bit for bit with the wavefront schedule's
(k_step, whose loop did not change). Nothing here drives the cap path, which cannot be reached from a valid call.
"""
import numpy as np
import pytest

import rt_amd
from rt_amd import abi, scenes

pytestmark = pytest.mark.gpu

F64, F32 = abi.RT_PREC_F64, abi.RT_PREC_F32
SPP, DEPTH, SEED = 12, 6, 3
KSTEP = dict(segments_per_launch=3, pool_slots=777)  # the wavefront schedule
ORDERED = dict(traversal=abi.RT_TRAV_ORDERED)  # RTOW in reference order: the binary BVH
# stats().segments of the persistent render, from the parent commit's build: (scene, precision) -> segments
PARENT_SEGMENTS = {
    ("cornell_box", F64): 140051,
    ("cornell_box", F32): 140051,
    ("cornell_box_with_volume", F64): 133716,
    ("cornell_box_with_volume", F32): 133716,
    ("rtow", F64): 86603,
    ("rtow", F32): 86603,
}
CASES = [("cornell_box", {}), ("cornell_box_with_volume", {}), ("rtow", ORDERED)]


@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("precision", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_segments_and_image_unmoved(ctx, name, kw, precision):
    desc, cam, _, _ = scenes.SCENES[name](width=70)
    ctx.upload(desc)
    ctx.reset_counters()
    img = ctx.render(cam, SPP, DEPTH, seed=SEED, precision=precision, **kw)
    segments = ctx.stats().segments
    print(f"{name} precision {precision}: segments {segments}")
    assert img.max() > 0
    assert segments == PARENT_SEGMENTS[name, precision]
    assert np.array_equal(ctx.render(cam, SPP, DEPTH, seed=SEED, precision=precision, **kw, **KSTEP), img)
