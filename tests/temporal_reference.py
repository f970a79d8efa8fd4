"""rt_temporal's algorithm (include/rt_hip.h, "temporal accumulation") in numpy float64, for the tests of rt_temporal,
and the seeded frame sequences they run on. The algorithm is written from the header's text with whole-image
operations per tap, not from the library's code: the two agree to rounding, not to the bit.

A history is dict(c (H, W, 3), v (H, W), n (H, W, 3), z (H, W), N (H, W), id (H, W) int32): the header's four planes.
A frame is dict(W, H, cam, rgb (H, W, 3), feat (H * W, 8), ids (H * W, 4) int32, var (H, W), clean (H, W, 3)).

The guides are built analytically: a floor plane (object 0) with a rug lying in it (object 2: same plane, same normal,
another id), one box standing on it (object 1) and sky above the horizon, seen by perspective cameras built with
rt_amd.perspective. A sequence is three frames of one camera motion:
  A  33 x 31, a sideways translation: a disocclusion band beside the box
  B  the same scene with a yaw: pixels reproject outside the image
  C  a forward dolly
  D  byte-equal cameras
  E  a backward dolly past the nearest floor: points behind the camera before (A <= 0)
and the partial-wave and border shapes 1 x 1, 70 x 1, 1 x 70, 65 x 5 under A's translation."""
import numpy as np

from rt_amd import abi, perspective

UNKNOWN_ID = -2
# the parameters the tests run with: depth_tol wide enough for the floor's own depth slope between neighbouring pixels
# near the horizon, chosen with the cameras so that every decision's margin is >= MARGIN (test_temporal_reference.py)
DEFAULTS = dict(alpha_min=0.05, max_history=64, depth_tol=0.1, normal_cos=0.9, min_weight=0.25, demodulate=True,
                albedo_eps=1e-2)
MARGIN = 1e-4


# ------------------------------------------------------------------ the algorithm
def _vec(a):
    return np.array(list(a), np.float64)


def same_camera(cam, prev_cam):
    return bytes(cam) == bytes(prev_cam)


def current(rgb, feat, var, ids, demodulate, albedo_eps):
    """Step 1 -> dict(a, c, v, n, z, miss, id, ok)"""
    H, W = rgb.shape[:2]
    f = np.asarray(feat, np.float64).reshape(H, W, 8)
    with np.errstate(all="ignore"):
        a = f[..., 0:3] + albedo_eps if demodulate else np.ones((H, W, 3))
        c = np.asarray(rgb, np.float64) / a
        m = (a[..., 0] + a[..., 1] + a[..., 2]) / 3.0
        v = np.ones((H, W)) if var is None else np.asarray(var, np.float64).reshape(H, W) / 3.0 / (m * m)
        hit = f[..., 7]
        miss = ~(hit > 0)
        safe = np.where(miss, 1.0, hit)
        n = np.where(miss[..., None], 0.0, f[..., 3:6] / safe[..., None])
        z = np.where(miss, -1.0, f[..., 6] / safe)
    pid = np.full((H, W), UNKNOWN_ID, np.int32) if ids is None else np.asarray(ids, np.int32).reshape(H, W, 4)[..., 0]
    ok = np.isfinite(c).all(-1) & np.isfinite(v)
    return dict(a=a, m=m, c=c, v=v, n=n, z=z, miss=miss, id=pid.copy(), ok=ok)


def reproject(cam, prev_cam, z, miss):
    """Step 2 -> (fx, fy, z', A): where each pixel was, the distance from the camera before, and A (+inf where the
    cameras are byte-equal, so that A > 0 holds)."""
    H, W = z.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if same_camera(cam, prev_cam):
        return x, y, z.copy(), np.full((H, W), np.inf)
    u = ((x + 0.5) / W - 0.5)[..., None]
    v = (0.5 - (y + 0.5) / H)[..., None]
    d = cam.focal_length * _vec(cam.dir) + u * cam.viewport_width * _vec(cam.right) + v * cam.viewport_height * _vec(cam.up)
    X = _vec(cam.pos) + d / np.linalg.norm(d, axis=-1, keepdims=True) * z[..., None]
    r = np.where(miss[..., None], d, X - _vec(prev_cam.pos))
    zp = np.where(miss, z, np.linalg.norm(r, axis=-1))
    pd, pr, pu = _vec(prev_cam.dir), _vec(prev_cam.right), _vec(prev_cam.up)
    A, B, C = r @ pd / (pd @ pd), r @ pr / (pr @ pr), r @ pu / (pu @ pu)
    with np.errstate(all="ignore"):
        fx = (B * prev_cam.focal_length / A / prev_cam.viewport_width + 0.5) * W - 0.5
        fy = (0.5 - C * prev_cam.focal_length / A / prev_cam.viewport_height) * H - 0.5
    return fx, fy, zp, A


def temporal(cam, prev_cam, rgb, feat, var=None, ids=None, hist=None, alpha_min=0.05, max_history=64, depth_tol=0.1,
             normal_cos=0.9, min_weight=0.25, demodulate=True, albedo_eps=1e-2):
    """One call -> dict(rgb (H, W, 3), var (H, W), hist (a history), info): info holds each decision's smallest margin
    over the pixels and taps that take it (depth: | |z_q - z'| / (depth_tol z') - 1 |; normal: |n_p . n_q - normal_cos|;
    weight: |Wv - min_weight| over the pixels with a valid tap; A: |A|) and the number of pixels per branch."""
    H, W = rgb.shape[:2]
    cur = current(rgb, feat, var, ids, demodulate, albedo_eps)
    c_cur, v_cur, miss, ok = cur["c"], cur["v"], cur["miss"], cur["ok"]
    Wv = np.zeros((H, W))
    sc, sv, sN = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
    info = dict(margin_depth=np.inf, margin_normal=np.inf, margin_weight=np.inf, margin_A=np.inf, depth_rejected=0,
                normal_rejected=0, id_rejected=0, outside=0, miss_to_miss=0, behind=0, bad_current=int((~ok).sum()),
                bad_history=0, with_history=0)
    if hist is not None:
        fx, fy, zp, A = reproject(cam, prev_cam, cur["z"], miss)
        info["margin_A"] = float(np.abs(A).min())
        with np.errstate(all="ignore"):
            look = (A > 0) & np.isfinite(fx) & np.isfinite(fy) & (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
        info["behind"] = int((~(A > 0)).sum())
        fx, fy = np.where(look, fx, 0.0), np.where(look, fy, 0.0)
        x0, y0 = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0, fy - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        rej = dict(depth=np.zeros((H, W), bool), normal=np.zeros((H, W), bool), id=np.zeros((H, W), bool),
                   outside=~look & (A > 0), bad=np.zeros((H, W), bool))
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                w = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
                live = look & (w != 0)
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                rej["outside"] |= live & ~inside
                live &= inside
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                cq, vq, nq, zq = hist["c"][qy, qx], hist["v"][qy, qx], hist["n"][qy, qx], hist["z"][qy, qx]
                Nq, idq = hist["N"][qy, qx], hist["id"][qy, qx]
                with np.errstate(all="ignore"):
                    good = np.isfinite(cq).all(-1) & np.isfinite(vq) & (Nq > 0)
                    rej["bad"] |= live & ~good
                    live &= good
                    hh = live & ~miss & (zq >= 0)  # hit to hit: the three tests, in the header's order
                    ratio = np.abs(zq - zp) / (depth_tol * zp)
                    near = ratio <= 1.0
                    dot = (cur["n"] * nq).sum(-1)
                    facing = dot >= normal_cos
                    same_id = (cur["id"] == idq) | (cur["id"] == UNKNOWN_ID) | (idq == UNKNOWN_ID)
                if hh.any():
                    info["margin_depth"] = min(info["margin_depth"], float(np.abs(ratio[hh] - 1.0).min()))
                if (hh & near).any():
                    info["margin_normal"] = min(info["margin_normal"], float(np.abs(dot[hh & near] - normal_cos).min()))
                rej["depth"] |= hh & ~near
                rej["normal"] |= hh & near & ~facing
                rej["id"] |= hh & near & facing & ~same_id
                valid = np.where(miss, live & (zq < 0), hh & near & facing & same_id)
                wv = np.where(valid, w, 0.0)
                Wv += wv
                sc += wv[..., None] * np.where(valid[..., None], cq, 0.0)
                sv += wv * wv * np.where(valid, vq, 0.0)
                sN += wv * np.where(valid, Nq, 0.0)
        some = Wv > 0
        if some.any():
            info["margin_weight"] = float(np.abs(Wv[some] - min_weight).min())
        for k in ("depth", "normal", "id", "outside"):
            info[k + "_rejected" if k != "outside" else k] = int(rej[k].sum())
        info["bad_history"] = int(rej["bad"].sum())
    have = (Wv >= min_weight) & (Wv > 0)
    info["with_history"] = int(have.sum())
    info["miss_to_miss"] = int((have & miss).sum())
    div = np.where(have, Wv, 1.0)
    c_h, v_h, N_h = sc / div[..., None], sv / (div * div), sN / div
    with np.errstate(all="ignore"):
        alpha = np.maximum(alpha_min, 1.0 / (N_h + 1.0))
        c_b = (1.0 - alpha)[..., None] * c_h + alpha[..., None] * c_cur
        v_b = (1.0 - alpha) ** 2 * v_h + alpha ** 2 * v_cur
        N_b = np.minimum(N_h + 1.0, float(max_history))
        blend = have & ok
        keep = have & ~ok
        c = np.where(blend[..., None], c_b, np.where(keep[..., None], c_h, c_cur))
        v = np.where(blend, v_b, np.where(keep, v_h, v_cur))
        N = np.where(blend, N_b, np.where(keep, N_h, np.where(ok, 1.0, 0.0)))
        out_rgb = c * cur["a"]
        out_var = 3.0 * cur["m"] ** 2 * v
    new = dict(c=c, v=v, n=cur["n"], z=cur["z"], N=N, id=cur["id"])
    return dict(rgb=out_rgb, var=out_var, hist=new, info=info)


def unpack_history(buf, W, H, dtype):
    """The library's history buffer (uint8, the header's four planes) -> a history in float64."""
    buf = np.asarray(buf)
    size, n = np.dtype(dtype).itemsize, W * H
    col = buf[0:4 * size * n].view(dtype).reshape(H, W, 4).astype(np.float64)
    gui = buf[4 * size * n:8 * size * n].view(dtype).reshape(H, W, 4).astype(np.float64)
    return dict(c=col[..., 0:3], v=col[..., 3], n=gui[..., 0:3], z=gui[..., 3],
                N=buf[8 * size * n:9 * size * n].view(dtype).reshape(H, W).astype(np.float64),
                id=buf[9 * size * n:9 * size * n + 4 * n].view(np.int32).reshape(H, W).copy())


def poke_nan(hist, y, x, W=None, H=None, dtype=None):
    """A NaN in the green channel of pixel (y, x)'s accumulated colour, its count left as it is: in a history dict, or
    in the library's buffer (W, H, dtype given). In place."""
    if isinstance(hist, dict):
        hist["c"][y, x, 1] = np.nan
    else:
        hist[0:4 * np.dtype(dtype).itemsize * W * H].view(dtype).reshape(H, W, 4)[y, x, 1] = np.nan


# ------------------------------------------------------------------ the scene, analytically
SIGMA = 0.14
VAR_DOF = 8
SKY = np.array([0.3, 0.4, 0.9])
ALBEDO = {0: [0.7, 0.6, 0.5], 1: [0.2, 0.5, 0.8], 2: [0.3, 0.6, 0.4]}
BOX = (np.array([0.3, 0.0, -4.0]), np.array([1.3, 1.0, -3.0]))
RUG = (-1.5, 0.2, -5.0, -2.5)  # x0, x1, z0, z1 on the floor y = 0


def camera(W, H, pos, lookat, fovy=70.0):
    """rt_amd.perspective with exactly H rows."""
    cam = perspective(W, W / (H + 0.5), pos, lookat, fovy_degree=fovy)
    assert (cam.image_width, cam.image_height) == (W, H)
    return cam


def guides(cam):
    """The first hit of every pixel's centre ray -> dict(feat (H * W, 8), ids (H * W, 4) int32, X (H, W, 3) the world
    point (0 for the sky), hit (H, W) bool)."""
    W, H = cam.image_width, cam.image_height
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u = ((x + 0.5) / W - 0.5)[..., None]
    v = (0.5 - (y + 0.5) / H)[..., None]
    d = cam.focal_length * _vec(cam.dir) + u * cam.viewport_width * _vec(cam.right) + v * cam.viewport_height * _vec(cam.up)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    o = _vec(cam.pos)
    with np.errstate(all="ignore"):
        t_floor = np.where(d[..., 1] < 0, -o[1] / d[..., 1], np.inf)
        t0 = (BOX[0] - o) / d
        t1 = (BOX[1] - o) / d
        tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
        t_in, t_out = tn.max(-1), tf.min(-1)
        axis = tn.argmax(-1)
        t_box = np.where((t_in <= t_out) & (t_in > 0), t_in, np.inf)
    t = np.minimum(t_floor, t_box)
    hit = np.isfinite(t)
    X = np.where(hit[..., None], o + d * np.where(hit, t, 0.0)[..., None], 0.0)
    on_box = hit & (t_box < t_floor)
    on_rug = hit & ~on_box & (X[..., 0] >= RUG[0]) & (X[..., 0] <= RUG[1]) & (X[..., 2] >= RUG[2]) & (X[..., 2] <= RUG[3])
    obj = np.where(on_box, 1, np.where(on_rug, 2, 0))
    normal = np.zeros((H, W, 3))
    normal[hit & ~on_box] = [0.0, 1.0, 0.0]
    face = -np.sign(np.take_along_axis(d, axis[..., None], -1)[..., 0])
    for k in range(3):
        sel = on_box & (axis == k)
        normal[sel, k] = face[sel]
    albedo = np.where(hit[..., None], np.array([ALBEDO[0], ALBEDO[1], ALBEDO[2]])[obj], SKY)
    feat = np.concatenate([albedo, normal, np.where(hit, t, 0.0)[..., None], hit[..., None].astype(np.float64)], -1)
    ids = np.full((H, W, 4), -1, np.int32)
    ids[hit] = np.stack([obj, obj, np.full_like(obj, 2), np.ones_like(obj)], -1)[hit]
    return dict(feat=feat.reshape(H * W, 8).copy(), ids=ids.reshape(H * W, 4).copy(), X=X, hit=hit)


def frame(cam, seed, sigma=SIGMA):
    """The scene through `cam` with fresh noise: the light is a smooth function of the world point, so the clean
    colour of a surface point is the same in every frame."""
    g = guides(cam)
    W, H = cam.image_width, cam.image_height
    rng = np.random.default_rng(seed)
    X = g["X"]
    light = np.where(g["hit"], 0.8 + 0.3 * np.sin(1.3 * X[..., 0]) * np.cos(0.9 * X[..., 2]), 1.0)
    clean = g["feat"].reshape(H, W, 8)[..., 0:3] * light[..., None]
    var = 3.0 * sigma * sigma * rng.chisquare(VAR_DOF, (H, W)) / VAR_DOF
    rgb = clean + sigma * rng.standard_normal((H, W, 3))
    return dict(W=W, H=H, cam=cam, rgb=rgb, feat=g["feat"], ids=g["ids"], var=var, clean=clean)


# name -> (W, H, positions of the three cameras, what they look at)
_LOOK = np.array([0.2, 0.55, -3.5])
MOTIONS = {
    "A": (33, 31, [(-0.31 + 0.17 * k, 1.2, 0.0) for k in range(3)], [_LOOK + (0.17 * k, 0, 0) for k in range(3)]),
    "B": (33, 31, [(0.0, 1.2, 0.0)] * 3, [_LOOK + (0.47 * k, 0, 0) for k in range(3)]),
    "C": (33, 31, [(0.0, 1.2, 0.3 - 0.23 * k) for k in range(3)], [_LOOK + (0, 0, -0.23 * k) for k in range(3)]),
    "D": (33, 31, [(0.0, 1.2, 0.0)] * 3, [_LOOK] * 3),
    "E": (33, 31, [(0.0, 1.2, -1.9 + 1.7 * k) for k in range(3)], [_LOOK + (0, 0, 1.7 * k) for k in range(3)]),
}
EDGE_SHAPES = ((1, 1), (70, 1), (1, 70), (65, 5))
for _W, _H in EDGE_SHAPES:
    MOTIONS[f"{_W}x{_H}"] = (_W, _H, MOTIONS["A"][2], MOTIONS["A"][3])
# (y, x): a NaN colour in the first frame (stored with N = 0), one in the second frame, a NaN poked into the history
# the first call wrote (its count stays 1). Sequence A only.
NAN_FRAME0, NAN_FRAME1, NAN_HISTORY = (22, 9), (25, 20), (21, 14)


def sequence(name, seed=11):
    """name -> the three frames of the motion."""
    W, H, pos, look = MOTIONS[name]
    frames = [frame(camera(W, H, pos[k], look[k]), seed * 1000 + 17 * k + W * 131 + H) for k in range(3)]
    if name == "A":
        frames[0]["rgb"][NAN_FRAME0] = np.nan
        frames[1]["rgb"][NAN_FRAME1] = np.nan
    return frames


def sequences():
    return {name: sequence(name) for name in MOTIONS}


def rounded_to_float(fr):
    """The frame with rgb, feat and var rounded to float32 (kept as float64): what an RT_PREC_F32 call computes on."""
    out = dict(fr)
    for k in ("rgb", "feat", "var"):
        out[k] = fr[k].astype(np.float32).astype(np.float64)
    return out


def run(frames, use_var=True, use_ids=True, poke=None, **kw):
    """The reference over a sequence, each call on the history of the one before -> the list of temporal()'s dicts.
    poke: (y, x) of a NaN put into the first call's history before the second reads it."""
    params = dict(DEFAULTS, **kw)
    outs, hist, prev = [], None, None
    for k, fr in enumerate(frames):
        out = temporal(fr["cam"], prev, fr["rgb"], fr["feat"], fr["var"] if use_var else None,
                       fr["ids"] if use_ids else None, hist, **params)
        hist, prev = {key: val.copy() for key, val in out["hist"].items()}, fr["cam"]
        if k == 0 and poke is not None:
            poke_nan(hist, *poke)
        outs.append(out)
    return outs


def mse(img, fr):
    """Mean squared error against the clean image over the pixels where both are finite."""
    d = (np.asarray(img, np.float64) - fr["clean"]) ** 2
    return float(d[np.isfinite(d)].mean())
