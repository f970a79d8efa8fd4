"""rt_denoise's algorithm (include/rt_hip.h, "denoising") in numpy float64, for the tests of rt_denoise, and the seeded
synthetic frames they run on. The filter is written from the header's text, whole-image operations per tap, not from
the library's code: the two agree to rounding, not to the bit.

A frame is dict(W, H, rgb (H, W, 3), feat (H * W, 8), var (H, W), clean (H, W, 3), bad (H, W) bool: the pixels whose
input is not finite)."""
import numpy as np

DEFAULTS = dict(iterations=5, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, demodulate=True, albedo_eps=1e-2,
                color_eps=1e-8, depth_eps=1e-3)
H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside, else fill -> (b, inside (H, W) bool)."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((H, W), bool)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def albedo_factor(feat, W, H, demodulate, albedo_eps):
    f = feat.reshape(H, W, 8)
    return f[..., 0:3] + albedo_eps if demodulate else np.ones((H, W, 3))


def prepare(rgb, feat, var, demodulate=True, albedo_eps=1e-2):
    """-> dict(c (H, W, 3), v (H, W), n (H, W, 3), z (H, W), miss (H, W) bool, g (H, W, 2) = (gx, gy), a (H, W, 3))"""
    H, W = rgb.shape[:2]
    f = np.asarray(feat, np.float64).reshape(H, W, 8)
    rgb = np.asarray(rgb, np.float64)
    with np.errstate(all="ignore"):
        hit = f[..., 7]
        miss = ~(hit > 0)
        safe = np.where(miss, 1.0, hit)
        n = np.where(miss[..., None], 0.0, f[..., 3:6] / safe[..., None])
        z = np.where(miss, -1.0, f[..., 6] / safe)
        a = albedo_factor(f, W, H, demodulate, albedo_eps)
        c = rgb / a
        if var is None:
            v = np.ones((H, W))
        else:
            m = (a[..., 0] + a[..., 1] + a[..., 2]) / 3.0
            v0 = np.asarray(var, np.float64).reshape(H, W) / 3.0 / (m * m)
            sv, sw = np.zeros((H, W)), np.zeros((H, W))
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    q, inside = _shift(v0, j, i, 0.0)
                    w = (2.0 if i == 0 else 1.0) * (2.0 if j == 0 else 1.0)
                    sv += np.where(inside, w * q, 0.0)
                    sw += np.where(inside, w, 0.0)
            v = sv / sw
        g = np.zeros((H, W, 2))
        for axis, (dy, dx) in enumerate(((0, 1), (1, 0))):
            zf, inf_ = _shift(z, dy, dx, -1.0)
            zb, inb = _shift(z, -dy, -dx, -1.0)
            mf, _ = _shift(miss, dy, dx, True)
            mb, _ = _shift(miss, -dy, -dx, True)
            ef = inf_ & ~mf & ~miss
            eb = inb & ~mb & ~miss
            df, db = zf - z, z - zb
            g[..., axis] = np.where(ef & eb, (df + db) * 0.5, np.where(ef, df, np.where(eb, db, 0.0)))
    return dict(c=c, v=v, n=n, z=z, miss=miss, g=g, a=a)


def atrous(st, s, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, color_eps=1e-8, depth_eps=1e-3):
    """One pass with step s over prepare's state -> the state with c and v replaced."""
    c, v, n, z, miss, g = st["c"], st["v"], st["n"], st["z"], st["miss"], st["g"]
    H, W = v.shape
    pfin = np.isfinite(c).all(-1) & np.isfinite(v)
    sw, sc, sv = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W))
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                cq, inside = _shift(c, s * j, s * i, 0.0)
                vq, _ = _shift(v, s * j, s * i, 0.0)
                nq, _ = _shift(n, s * j, s * i, 0.0)
                zq, _ = _shift(z, s * j, s * i, 0.0)
                mq, _ = _shift(miss, s * j, s * i, False)
                ok = inside & np.isfinite(cq).all(-1) & np.isfinite(vq) & (mq == miss)
                d_c = np.where(pfin, ((c - cq) ** 2).mean(-1) / (sigma_color ** 2 * v + color_eps), 0.0)
                d_n = ((n - nq) ** 2).sum(-1) / sigma_normal ** 2
                den = sigma_depth * np.abs(g[..., 0] * (s * i) + g[..., 1] * (s * j)) + depth_eps * np.abs(z)
                d_z = np.where(miss | (z == zq), 0.0, np.abs(z - zq) / den)
                w = np.where(ok, H5[i + 2] * H5[j + 2] * np.exp(-(d_c + d_n + d_z)), 0.0)
                sw += w
                sc += w[..., None] * np.where(ok[..., None], cq, 0.0)
                sv += w * w * np.where(ok, vq, 0.0)
        some = sw > 0
        div = np.where(some, sw, 1.0)
        out = dict(st)
        out["c"] = np.where(some[..., None], sc / div[..., None], 0.0)
        out["v"] = np.where(some, sv / (div * div), 0.0)
    return out


def denoise(rgb, feat, var=None, iterations=5, sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, demodulate=True,
            albedo_eps=1e-2, color_eps=1e-8, depth_eps=1e-3):
    """The whole filter -> (H, W, 3) float64."""
    st = prepare(rgb, feat, var, demodulate, albedo_eps)
    for k in range(iterations):
        st = atrous(st, 1 << k, sigma_color, sigma_normal, sigma_depth, color_eps, depth_eps)
    return st["c"] * st["a"]


# ------------------------------------------------------------------ the frames
SIGMA = 0.14   # the noise of a channel of frame A (noisy MSE = SIGMA^2 = 0.0196)
VAR_DOF = 8    # the variance guide is the true variance times chi-square(VAR_DOF) / VAR_DOF
BACKGROUND = np.array([0.3, 0.4, 0.9])


def _finish(W, H, albedo, normal, depth, hit, light, seed, sigma):
    """Noise, the variance guide and the packing shared by the frames. albedo, normal, depth: of the surface, before
    the blend with the background a partial hit share brings."""
    rng = np.random.default_rng(seed)
    alb = hit[..., None] * albedo + (1.0 - hit[..., None]) * BACKGROUND
    feat = np.concatenate([alb, hit[..., None] * normal, (hit * depth)[..., None], hit[..., None]], -1)
    clean = alb * light[..., None]
    sig = np.full((H, W), sigma)
    var = 3.0 * sig * sig * rng.chisquare(VAR_DOF, (H, W)) / VAR_DOF
    rgb = clean + sig[..., None] * rng.standard_normal((H, W, 3))
    return dict(W=W, H=H, rgb=rgb, feat=feat.reshape(H * W, 8).copy(), var=var, clean=clean,
                bad=np.zeros((H, W), bool))


def frame_a(seed=7):
    """33 x 31: a depth-ramp floor, a nearer box with another normal and albedo, four miss rows, a column with
    0 < hit < 1, a zero-variance patch, one NaN pixel, noise of sigma SIGMA and a chi-square-noisy variance guide."""
    W, H = 33, 31
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    albedo = np.broadcast_to([0.7, 0.6, 0.5], (H, W, 3)).copy()
    normal = np.broadcast_to([0.0, 1.0, 0.0], (H, W, 3)).copy()
    depth = 5.0 + 0.1 * y + 0.03 * x
    box = (x >= 8) & (x <= 20) & (y >= 6) & (y <= 18)
    albedo[box], normal[box] = [0.2, 0.5, 0.8], [0.0, 0.0, 1.0]
    depth[box] = (3.0 + 0.02 * x)[box]
    hit = np.ones((H, W))
    hit[:4] = 0.0
    hit[4:, 25] = 0.5
    light = 0.8 + 0.3 * np.sin(x / 6.0) * np.cos(y / 7.0)
    light[:4] = 1.0
    fr = _finish(W, H, albedo, normal, depth, hit, light, seed, SIGMA)
    patch = (x >= 27) & (x <= 31) & (y >= 20) & (y <= 26)
    fr["rgb"][patch], fr["var"][patch] = fr["clean"][patch], 0.0
    fr["rgb"][15, 12] = np.nan
    fr["bad"][15, 12] = True
    return fr


def edge_frame(W, H, seed=3):
    """A small frame for the shapes at which the indexing can go wrong: a depth ramp with a step in normal and albedo
    half way along the longer side, one miss pixel (where there are more than two pixels), noise and variance as A's."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t = x if W >= H else y
    far = t >= max(W, H) / 2.0
    albedo = np.where(far[..., None], [0.25, 0.55, 0.75], [0.7, 0.6, 0.5])
    normal = np.where(far[..., None], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0])
    depth = 4.0 + 0.05 * x + 0.08 * y - 1.0 * far
    hit = np.ones((H, W))
    if W * H > 2:
        hit[H // 2, W // 3] = 0.0
    light = 0.9 + 0.2 * np.sin(t / 5.0)
    return _finish(W, H, albedo, normal, depth, hit, light, seed + W * 131 + H, SIGMA)


EDGE_SHAPES = ((1, 1), (70, 1), (1, 70), (65, 5))  # partial waves, a tile boundary, taps that all fall outside


def frames():
    """name -> frame: A and the edge shapes."""
    out = {"A": frame_a()}
    for W, H in EDGE_SHAPES:
        out[f"{W}x{H}"] = edge_frame(W, H)
    return out


def rounded_to_float(fr):
    """The frame with rgb, feat and var rounded to float32 (kept as float64): what an RT_PREC_F32 call computes on."""
    out = dict(fr)
    for k in ("rgb", "feat", "var"):
        out[k] = fr[k].astype(np.float32).astype(np.float64)
    return out


def mse(img, fr):
    """Mean squared error against the clean image over the pixels whose input was finite."""
    ok = ~fr["bad"]
    return float(((np.asarray(img, np.float64)[ok] - fr["clean"][ok]) ** 2).mean())
