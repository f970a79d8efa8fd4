"""The adaptive sampler's algorithm on the CPU (adaptive_reference.py over the oracle's batches; the oracle runs in
counter mode, so its sample keys are the GPU's).

1. The inputs of tests/test_gpu_adaptive.py are pinned here: for every scene, seed and threshold it uses, no pixel's
   decision lies within the comparison band of the threshold, and the sample-count map is not trivial.
2. Estimator honesty: over a frame, is the squared error of the means what the estimator says it is?
   ratio = sum over pixels and channels of (mean - truth)^2 / sum over pixels of se2, expected 1. Measured with the
   oracle on the 32 x 32 Cornell box at 64 spp (threshold = 0, depth 8, batch 4) for seeds 1..8, truth one render at
   8192 spp with seed 1000003:
       1.925  1.233  7.669  1.099  1.538  0.750  2.509  3.037
   The measurements straddle 1, with a heavy upper tail: a frame's squared error is dominated by a few pixels with a
   rare bright path, whose 16 batch sums seldom show it. The test holds the interval [min, max] of these measurements
   widened by 25 % each way.
"""
import numpy as np
import pytest

import adaptive_reference as ref
import oracle
from rt_amd import scenes

NPIX = ref.W * ref.H


def oracle_batches(desc, cam, seed, depth, nbatches=16, batch=4):
    sc = oracle.from_desc(desc)
    tiles = [(0, 0, cam.image_width, cam.image_height)]
    return [oracle.render(sc, cam, batch, depth, seed=seed, tiles=tiles, first_sample=batch * k)[0]
            for k in range(nbatches)]


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_gpu_case_has_an_empty_band_and_a_graded_sample_map(name):
    desc, cam = ref.frame(name)
    items = oracle_batches(desc, cam, ref.SEED, ref.DEPTH)
    assert np.isfinite(np.array(items)).all()
    thr = ref.CASES[name]
    r = ref.run(lambda k: items[k], NPIX, thr)
    hist = np.bincount(r["spp"] // 8, minlength=9)[1:]
    print(f"{name} threshold {thr}: pixels by rounds {hist.tolist()}, smallest |err^2 - thr^2| {r['margin'].min():.3g}")
    assert not r["band"].any()
    assert r["margin"].min() > 1000 * (ref.BAND_ABS + ref.BAND_REL * thr * thr)  # far outside it, not just outside
    assert hist[0] >= 50 and hist[-1] >= 50 and hist[1:-1].sum() >= 50 and (hist[1:-1] > 0).sum() >= 4
    assert r["spp"].sum() == 8 * sum(r["rounds"])


def test_gpu_round_edge_cases():
    # a frame whose every pixel has variance: threshold = 0 takes all of them through every round
    desc, cam = ref.frame(ref.FULL_SCENE, ref.FULL_ZOOM)
    items = oracle_batches(desc, cam, ref.SEED, ref.DEPTH)
    r = ref.run(lambda k: items[k], NPIX, 0.0)
    assert r["rounds"] == [NPIX] * 8 and (r["spp"] == 64).all() and (r["err"] > 0).all()
    # the last survivors stop in a middle round
    desc, cam = ref.frame(ref.EARLY_SCENE)
    items = oracle_batches(desc, cam, ref.SEED, ref.DEPTH)
    r = ref.run(lambda k: items[k], NPIX, ref.EARLY_THRESHOLD)
    assert 2 <= len(r["rounds"]) <= 6 and r["spp"].max() == 8 * len(r["rounds"]) < 64 and not r["band"].any()
    # threshold = inf: one round; a black frame: zeros with err = 0
    r = ref.run(lambda k: items[k], NPIX, np.inf)
    assert r["rounds"] == [NPIX] and (r["spp"] == 8).all() and np.isfinite(r["err"]).all()
    r = ref.run(lambda k: np.zeros((NPIX, 3)), NPIX, 0.0)
    assert r["rounds"] == [NPIX] and (r["rgb"] == 0).all() and (r["err"] == 0).all()


def test_reference_rounds_written_out_by_hand():
    # two pixels, batch 4: pixel 0 has equal batches (stops at min_spp), pixel 1 alternates 0 and 2 (mean 1)
    means = lambda k: np.array([[0.5, 0.5, 0.5], [2.0 * (k & 1)] * 3])
    r = ref.run(means, 2, 0.2, batch=4, min_spp=8, step_spp=8, max_spp=32, floor=0.0625)
    assert r["spp"].tolist() == [8, 32] and r["err"][0] == 0.0 and (r["rgb"][1] == 1.0).all()
    # pixel 1 after K = 8 batch sums of 0 or 8: var = (4 * 64 - 32^2 / 8) / 7 a channel, se2 = 3 var / (8 * 16)
    var = (256.0 - 128.0) / 7.0
    assert r["err"][1] == np.sqrt(((var + var) + var) / 128.0 / 3.0) / (0.0625 + 1.0)
    # a NaN batch: the pixel runs to max_spp whatever the threshold
    nan = lambda k: np.array([[np.nan if k == 1 else 0.5] * 3])
    r = ref.run(nan, 1, np.inf, max_spp=24)
    assert r["spp"].tolist() == [24] and np.isnan(r["err"][0])


# ------------------------------------------------------------------ estimator honesty
HONESTY_MEASURED = (1.925, 1.233, 7.669, 1.099, 1.538, 0.750, 2.509, 3.037)  # seeds 1..8 (the module's docstring)


@pytest.mark.slow
def test_estimator_honesty_on_the_cornell_box():
    desc, cam, _, _ = scenes.cornell_box(width=32)
    assert (cam.image_width, cam.image_height) == (32, 32)
    sc = oracle.from_desc(desc)
    truth = oracle.render(sc, cam, 8192, 8, seed=1000003)[0].reshape(-1, 3)
    lo, hi = 0.75 * min(HONESTY_MEASURED), 1.25 * max(HONESTY_MEASURED)
    assert min(HONESTY_MEASURED) < 1.0 < max(HONESTY_MEASURED)  # the measurements straddle the expectation
    ratios = []
    for seed in range(1, 9):
        items = oracle_batches(desc, cam, seed, 8)
        r = ref.run(lambda k: items[k].reshape(-1, 3), truth.shape[0], 0.0)
        ratios.append(float(((r["rgb"] - truth) ** 2).sum() / r["se2"].sum()))
    print("honesty ratios, seeds 1..8: " + "  ".join(f"{x:.3f}" for x in ratios))
    assert all(lo <= x <= hi for x in ratios), ratios
