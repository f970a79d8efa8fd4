"""The adaptive sampler's algorithm (include/rt_hip.h, "adaptive sampling") in numpy, for the tests of
rt_render_adaptive: the batch-means estimator and the round logic in float64, every operation in the order the header
writes it, so that the same batch sums give the same bits as the device.

The caller supplies the batches: item_means(k) -> (npix, 3), batch k's mean per pixel (what a render of samples
[k * batch, (k + 1) * batch) with samples_per_item = batch returns). The helper multiplies by `batch` to get the item
sums back, which is exact for a power-of-two batch (the tests use 4)."""
import numpy as np

BAND_ABS, BAND_REL = 1e-12, 1e-9  # the comparison band around threshold^2 (in_band)


def estimate(K, batch, S, Q, floor):
    """K (npix,) batches with the moments S, Q (npix, 3) -> (mean (npix, 3), se2 (npix,), err (npix,))."""
    k = np.asarray(K, np.float64)
    b = np.float64(batch)
    n = k * b
    with np.errstate(all="ignore"):
        mean = S / n[:, None]
        d = Q - (S * S) / k[:, None]
        var = np.where(d < 0.0, 0.0, d) / (k - 1.0)[:, None]  # (keeps a NaN, as the device's select does)
        se2 = ((var[:, 0] + var[:, 1]) + var[:, 2]) / (k * (b * b))
        level = ((mean[:, 0] + mean[:, 1]) + mean[:, 2]) / 3.0
        err = np.sqrt(se2 / 3.0) / (floor + level)
    return mean, se2, err


def in_band(err, threshold):
    """Whether a decision err <= threshold could fall either way under rounding: |err^2 - threshold^2| within
    1e-12 + 1e-9 threshold^2. An infinite threshold has no band (nothing compares close to it)."""
    if not np.isfinite(threshold):
        return np.zeros(np.shape(err), bool)
    t2 = threshold * threshold
    with np.errstate(all="ignore"):
        return np.abs(err * err - t2) <= BAND_ABS + BAND_REL * t2


def run(item_means, npix, threshold, batch=4, min_spp=8, step_spp=8, max_spp=64, floor=0.01):
    """The rounds over npix pixels -> dict(rgb (npix, 3) float64 before the rounding to the precision, spp (npix,)
    int32, err, se2 (npix,) float64 at the pixel's last round, band (npix,) bool: some decision of the pixel lay in the
    band, margin (npix,) the smallest |err^2 - threshold^2| over the pixel's decisions that were the comparison's (not
    max_spp's), rounds: the active count at the start of every round)."""
    S = np.zeros((npix, 3))
    Q = np.zeros((npix, 3))
    K = np.zeros(npix, np.int64)
    active = np.arange(npix)
    out = dict(rgb=np.zeros((npix, 3)), spp=np.zeros(npix, np.int32), err=np.zeros(npix), se2=np.zeros(npix),
               band=np.zeros(npix, bool), margin=np.full(npix, np.inf), rounds=[])
    have, k = 0, 0
    while active.size:
        out["rounds"].append(int(active.size))
        spp = min_spp if have == 0 else step_spp
        for _ in range(spp // batch):  # in batch order
            s = np.asarray(item_means(k), np.float64)[active] * np.float64(batch)
            S[active] += s
            Q[active] += s * s
            K[active] += 1
            k += 1
        have += spp
        mean, se2, err = estimate(K[active], batch, S[active], Q[active], floor)
        last = have >= max_spp
        with np.errstate(all="ignore"):
            stop = (err <= threshold) | last
        if not last:  # (at max_spp the comparison decides nothing)
            out["band"][active] |= in_band(err, threshold)
            if np.isfinite(threshold):
                with np.errstate(all="ignore"):
                    out["margin"][active] = np.fmin(out["margin"][active], np.abs(err * err - threshold * threshold))
        done = active[stop]
        out["rgb"][done], out["spp"][done], out["err"][done], out["se2"][done] = mean[stop], have, err[stop], se2[stop]
        active = active[~stop]
    return out


# ------------------------------------------------------------------ the inputs of the GPU test
# tests/test_gpu_adaptive.py's frames and thresholds, pinned on the CPU by tests/test_adaptive_reference.py: with the
# oracle's batches no decision lies in the band and the sample-count map has pixels at min_spp, at max_spp and between.
W, H = 33, 31  # 1023 pixels: no multiple of the wave or the block, four blocks
DEPTH, SEED = 8, 11
# scene (material_scenes.py) -> threshold: one scene per persistent family
CASES = {"backlight": 0.2, "chain": 0.15, "spheres_nl": 0.1, "spheres_nl_hbm": 0.05, "instanced": 0.1}
# a frame in which every pixel has variance (a view into the room, no background): threshold = 0 takes all to max_spp
FULL_SCENE, FULL_ZOOM = "chain", 0.35
# a threshold at which the last survivors stop in a middle round (the loop ends early on a count of 0)
EARLY_SCENE, EARLY_THRESHOLD = "spheres_nl_hbm", 0.2


def frame(name, zoom=1.0, width=W, height=H):
    """(desc, cam) of a material_scenes scene through its perspective camera at width x height pixels, the viewport
    scaled by `zoom` about its centre."""
    import material_scenes
    desc, cam = material_scenes.build(name, "perspective")
    cam.image_width, cam.image_height = width, height
    cam.viewport_width *= zoom
    cam.viewport_height *= zoom
    return desc, cam
