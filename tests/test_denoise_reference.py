"""The numpy reference of rt_denoise (tests/denoise_reference.py), pinned on properties that follow from the
algorithm's text, before anything is compared with it."""
import numpy as np

import denoise_reference as R


def flat_feat(W, H, albedo=(0.5, 0.5, 0.5)):
    feat = np.zeros((H * W, 8))
    feat[:, 0:3] = albedo
    feat[:, 4] = 1.0
    feat[:, 6] = 3.0
    feat[:, 7] = 1.0
    return feat


def test_a_constant_image_is_unchanged():
    W, H = 21, 17
    rgb = np.broadcast_to([0.25, 0.5, 0.75], (H, W, 3)).copy()
    for var in (None, np.full((H, W), 0.01)):
        out = R.denoise(rgb, flat_feat(W, H), var, demodulate=False)
        assert np.abs(out - rgb).max() <= 1e-15


def test_one_pass_scales_the_variance_of_a_flat_field():
    # every weight is h_i h_j (the colour distance vanishes against sigma_color = 1e6, normals and depths are equal), so
    # v' = sum (h_i h_j)^2 v = (sum h^2)^2 v = ((1 + 16 + 36 + 16 + 1) / 256)^2 v in the interior
    W, H = 16, 12
    rng = np.random.default_rng(1)
    rgb = 0.5 + 0.1 * rng.standard_normal((H, W, 3))
    st = R.prepare(rgb, flat_feat(W, H), np.full((H, W), 0.03), demodulate=False)
    assert np.allclose(st["v"], 0.01, rtol=0, atol=1e-17)
    out = R.atrous(st, 1, sigma_color=1e6)
    ratio = out["v"][2:-2, 2:-2] / st["v"][2:-2, 2:-2]
    assert np.abs(ratio - (70.0 / 256.0) ** 2).max() < 1e-9
    assert abs((70.0 / 256.0) ** 2 - 0.074768) < 1e-6


def test_the_nan_pixel_comes_out_finite():
    fr = R.frame_a()
    assert np.isnan(fr["rgb"]).any(-1).sum() == 1 == fr["bad"].sum()
    for var in (fr["var"], None):
        for it in (1, 5):
            assert np.isfinite(R.denoise(fr["rgb"], fr["feat"], var, iterations=it)).all()


def test_frame_a_has_what_it_says():
    fr = R.frame_a()
    f = fr["feat"].reshape(fr["H"], fr["W"], 8)
    assert (fr["W"], fr["H"]) == (33, 31)
    assert (f[:4, :, 7] == 0).all() and ((f[..., 7] > 0) & (f[..., 7] < 1)).any(1).sum() == fr["H"] - 4
    assert (fr["var"] == 0).sum() == 35 and len(np.unique(f[4:, :, 3:6].reshape(-1, 3), axis=0)) >= 3
    assert abs(R.mse(fr["rgb"], fr) - R.SIGMA ** 2) < 0.1 * R.SIGMA ** 2


def test_denoising_frame_a_lowers_the_error():
    fr = R.frame_a()
    noisy = R.mse(fr["rgb"], fr)
    with_var = R.mse(R.denoise(fr["rgb"], fr["feat"], fr["var"]), fr)
    without = R.mse(R.denoise(fr["rgb"], fr["feat"], None, sigma_color=0.3), fr)
    print(f"frame A: noisy MSE {noisy:.4g}, denoised with var {with_var:.4g}, without (sigma_color 0.3) {without:.4g}")
    assert with_var < noisy and without < noisy
    assert with_var < without  # (the variance guide is what makes the colour weight usable at this noise)


def test_edge_shapes_run_and_stay_finite():
    for W, H in R.EDGE_SHAPES:
        fr = R.edge_frame(W, H)
        for it in (1, 8):
            out = R.denoise(fr["rgb"], fr["feat"], fr["var"], iterations=it)
            assert out.shape == (H, W, 3) and np.isfinite(out).all()
    fr = R.edge_frame(1, 1)  # every tap but the centre falls outside: the pixel comes back (times a / a)
    assert np.abs(R.denoise(fr["rgb"], fr["feat"], fr["var"]) - fr["rgb"]).max() < 1e-15
