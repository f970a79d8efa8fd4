"""The numpy reference of rt_temporal (tests/temporal_reference.py) and its frame sequences, pinned on the CPU before
anything is compared with them: every decision the algorithm takes on these frames is taken with a margin far above
a float's rounding of the stored depths and normals, every branch is taken by a stated number of pixels, and the
properties that follow from the algorithm's text hold."""
import numpy as np
import pytest

import temporal_reference as R

SEQS = R.sequences()
RUNS = {name: R.run(fr, poke=R.NAN_HISTORY if name == "A" else None) for name, fr in SEQS.items()}
RUNS32 = {name: R.run([R.rounded_to_float(f) for f in fr], poke=R.NAN_HISTORY if name == "A" else None)
          for name, fr in SEQS.items()}


@pytest.mark.parametrize("name", list(SEQS))
def test_every_decision_has_a_margin(name):
    """>= 1e-4 for the depth test (relative to depth_tol), the normal test, Wv against min_weight and A against 0, on
    the frames as they are and on the frames rounded to float: a float's rounding of z (6e-8 relative, 6e-7 of
    depth_tol = 0.1) and of n cannot turn a decision."""
    for runs in (RUNS, RUNS32):
        for k, out in enumerate(runs[name]):
            info = out["info"]
            for key in ("margin_depth", "margin_normal", "margin_weight", "margin_A"):
                assert info[key] >= R.MARGIN, (name, k, key, info[key])


# sequence -> the least number of pixels of the second and third frame that take each branch
BRANCHES = {
    "A": dict(depth_rejected=200, normal_rejected=10, id_rejected=15, outside=50, miss_to_miss=300, with_history=900),
    "B": dict(depth_rejected=100, normal_rejected=10, id_rejected=15, outside=150, miss_to_miss=250, with_history=700),
    "C": dict(depth_rejected=100, normal_rejected=5, id_rejected=15, outside=30, miss_to_miss=300, with_history=900),
    "D": dict(miss_to_miss=363, with_history=1023),
    "E": dict(depth_rejected=100, normal_rejected=3, id_rejected=5, outside=300, miss_to_miss=200, behind=150,
              with_history=350),
    "70x1": dict(depth_rejected=10, outside=70, with_history=70),
    "1x70": dict(outside=60, miss_to_miss=20, with_history=25),
    "65x5": dict(depth_rejected=100, outside=40, miss_to_miss=100, with_history=300),
    "1x1": dict(outside=1),
}


@pytest.mark.parametrize("name", list(SEQS))
def test_each_branch_is_taken(name):
    for k in (1, 2):
        info = RUNS[name][k]["info"]
        for key, least in BRANCHES[name].items():
            assert info[key] >= least, (name, k, key, info[key])
    first = RUNS[name][0]["info"]
    assert first["with_history"] == 0  # a first frame
    if name == "A":  # the NaN colours and the NaN put into the first history
        assert [RUNS[name][k]["info"]["bad_current"] for k in range(3)] == [1, 1, 0]
        assert RUNS[name][1]["info"]["bad_history"] >= 2 and RUNS[name][2]["info"]["bad_history"] == 0
    if name == "D":  # byte-equal cameras: nothing is rejected
        for k in (1, 2):
            info = RUNS[name][k]["info"]
            assert info["depth_rejected"] == info["normal_rejected"] == info["id_rejected"] == info["outside"] == 0


def test_the_nan_pixels_do_what_the_header_says():
    outs, fr = RUNS["A"], SEQS["A"]
    y, x = R.NAN_FRAME0
    assert np.isnan(outs[0]["rgb"][y, x]).all() and outs[0]["hist"]["N"][y, x] == 0  # stored as it is, never a tap
    assert np.isnan(outs[0]["rgb"]).any(-1).sum() == 1
    # the second frame's NaN colour lies where there is history: the pixel keeps c_h, and its count does not grow
    y, x = R.NAN_FRAME1
    assert np.isnan(fr[1]["rgb"][y, x]).all() and np.isfinite(outs[1]["rgb"][y, x]).all()
    assert outs[1]["hist"]["N"][y, x] == 1.0
    # no NaN is left in the second and third outputs: neither NaN record is ever a valid tap
    assert np.isfinite(outs[1]["rgb"]).all() and np.isfinite(outs[2]["rgb"]).all()
    assert np.isfinite(outs[1]["var"]).all() and np.isfinite(outs[2]["var"]).all()


def test_byte_equal_cameras_give_the_running_mean():
    """alpha_min = 0: frame k's output is the mean of the k inputs, N = k, and var_out is the variance of that mean
    under independence, the mean of the k var divided by k -- with demodulation and without."""
    fr = SEQS["D"]
    feat = fr[0]["feat"]
    for demodulate in (True, False):
        hist, outs = None, []
        for k in range(3):
            out = R.temporal(fr[0]["cam"], fr[0]["cam"], fr[k]["rgb"], feat, fr[k]["var"], fr[0]["ids"], hist,
                             **dict(R.DEFAULTS, alpha_min=0.0, demodulate=demodulate))
            hist = out["hist"]
            mean = np.mean([f["rgb"] for f in fr[:k + 1]], 0)
            var = np.mean([f["var"] for f in fr[:k + 1]], 0) / (k + 1)
            assert np.abs(out["rgb"] - mean).max() <= 1e-12 * np.abs(mean).max()
            assert np.abs(out["var"] - var).max() <= 1e-12 * var.max()
            assert (hist["N"] == k + 1).all()
    # max_history caps the count, and with it the weight of the history
    hist = None
    for k in range(3):
        out = R.temporal(fr[0]["cam"], fr[0]["cam"], fr[k]["rgb"], feat, None, None, hist,
                         **dict(R.DEFAULTS, alpha_min=0.0, max_history=2))
        hist = out["hist"]
    assert (hist["N"] == 2).all() and (hist["id"] == R.UNKNOWN_ID).all()


def test_alpha_min_bounds_the_history():
    fr = SEQS["D"]
    a = R.run(fr, alpha_min=1.0)  # the history has no weight: the output is the frame
    for k in range(3):
        assert np.abs(a[k]["rgb"] - fr[k]["rgb"]).max() <= 1e-12


def test_ids_separate_what_depth_and_normal_cannot():
    # the rug lies in the floor's plane: without ids nothing tells them apart, and no tap is rejected by id
    fr = SEQS["A"]
    without = R.run(fr, use_ids=False)
    assert without[1]["info"]["id_rejected"] == 0 and RUNS["A"][1]["info"]["id_rejected"] > 0
    assert without[1]["info"]["with_history"] >= RUNS["A"][1]["info"]["with_history"]


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "65x5"])
def test_accumulating_lowers_the_error(name):
    fr, outs = SEQS[name], RUNS[name]
    noisy, acc = R.mse(fr[2]["rgb"], fr[2]), R.mse(outs[2]["rgb"], fr[2])
    print(f"{name}: MSE of the third frame {noisy:.4g}, accumulated {acc:.4g}")
    assert acc < noisy
    # ... and the variance it hands on has shrunk where there is history
    have = outs[2]["hist"]["N"] > 1
    assert (outs[2]["var"][have] < fr[2]["var"][have]).mean() > 0.9


def test_the_frames_have_what_they_say():
    fr = SEQS["A"]
    assert (fr[0]["W"], fr[0]["H"]) == (33, 31)
    ids = fr[0]["ids"].reshape(31, 33, 4)[..., 0]
    assert set(np.unique(ids)) == {-1, 0, 1, 2}  # sky, floor, box, rug
    f = fr[0]["feat"].reshape(31, 33, 8)
    assert ((f[..., 7] == 0) == (ids == -1)).all() and (f[..., 6][ids >= 0] > 0).all()
    assert len(np.unique(f[..., 3:6][ids == 1], axis=0)) >= 2  # two faces of the box
    assert bytes(SEQS["D"][0]["cam"]) == bytes(SEQS["D"][1]["cam"]) and bytes(fr[0]["cam"]) != bytes(fr[1]["cam"])
    for (W, H) in R.EDGE_SHAPES:
        assert (SEQS[f"{W}x{H}"][0]["W"], SEQS[f"{W}x{H}"][0]["H"]) == (W, H)
