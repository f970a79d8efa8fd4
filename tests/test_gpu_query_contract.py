"""What the five render and query entry points answer to arguments they refuse, called through the C ABI with ctypes:
rt_render_tiles, rt_trace_rays, rt_occluded, rt_camera_rays and rt_render_aov.

A characterisation table, read off the entry points' code: every row is one call with one invalid argument (or two,
to pin which error wins), its exact status and the exact text of rt_last_error. The entries do not check in the same
order -- rt_render_tiles reports a missing scene before a bad camera, rt_render_aov a bad camera before a missing
scene, rt_trace_rays a misaligned pointer before a missing scene -- and the table holds each to its own order. The last
rows are calls over zero rays or pixels: RT_OK, and rt_counters.launches does not move.

Every row is refused on the host before any launch, or launches nothing. All the same, every pointer that is not the
row's fault points at a buffer large enough for the call the row would otherwise make (one ray, or the 8 x 8 image).
Two things the table cannot hold without a launch and so only notes: rt_render_tiles checks neither the traversal
(anything but RT_TRAV_ORDERED is RT_TRAV_AUTO; pinned below with an empty tile list) nor any alignment, and
rt_camera_rays needs no scene (pinned with an empty tile list on a context without one).
"""
import ctypes

import numpy as np
import pytest

import rt_amd
from rt_amd import abi, scenes

pytestmark = pytest.mark.gpu

OK, INVALID, NO_SCENE = abi.RT_OK, abi.RT_ERR_INVALID_ARGUMENT, abi.RT_ERR_NO_SCENE
M_NULL_CTX = "null context"
M_NULL = "null argument"
M_NO_SCENE = "rt_scene_upload has not succeeded on this context"
M_CAM = "unknown camera mode"
M_EMPTY = "empty image"
M_WIDE = "image wider or taller than 65535 pixels"
M_TILE = "tile 0 outside the image"
M_SPP = "spp must be positive"
M_PREC = "unknown precision"
M_TRAV = "unknown traversal"
M_NRAYS = "nrays outside [0, 2^31)"
M_NPIX = "npix * spp outside [0, 2^31)"
M_PIXELS = "too many pixels in one call"
M_ALIGN = {"trace_rays": "device rays and out_ids must be 16-byte aligned, out_geom 8-byte",
           "occluded": "device rays must be 16-byte aligned",
           "camera_rays": "device out_rays must be 16-byte aligned",
           "render_aov": "device out_feat and out_ids must be 16-byte aligned"}

# the arguments of each entry after the context, in order; the pointer arguments that a device call takes from `dev`
ARGS = {"render_tiles": ("cam", "prm", "tiles", "ntiles", "out", "out_dev", "stream"),
        "trace_rays": ("prm", "rays", "n", "geom", "ids", "stream"),
        "occluded": ("prm", "rays", "n", "out", "stream"),
        "camera_rays": ("cam", "seed", "first_sample", "spp", "tiles", "ntiles", "out", "on_device", "stream"),
        "render_aov": ("cam", "prm", "tiles", "ntiles", "feat", "ids", "stream")}
POINTERS = {"render_tiles": ("out",), "trace_rays": ("rays", "geom", "ids"), "occluded": ("rays", "out"),
            "camera_rays": ("out",), "render_aov": ("feat", "ids")}
BUF_BYTES = 1 << 15  # each buffer: 8 x 8 pixels of 64 B, or one ray, fit many times


@pytest.fixture(scope="module")
def world():
    """Two contexts (`scene`: the Cornell box at 8 x 8 uploaded; `bare`: none), the camera, and for every pointer
    argument a host and a device buffer of BUF_BYTES."""
    import torch
    desc, cam = scenes.cornell_box(width=8)[:2]
    assert (cam.image_width, cam.image_height) == (8, 8)
    ctx, bare = rt_amd.Context(0), rt_amd.Context(0)
    ctx.upload(desc)
    names = sorted({p for ps in POINTERS.values() for p in ps})
    host = {p: np.zeros(BUF_BYTES // 8, dtype=np.float64) for p in names}
    dev = {p: torch.zeros(BUF_BYTES // 8, dtype=torch.float64, device="cuda:0") for p in names}
    host["rays"][:8] = (278, 278, -800, 0, 0, 1, 0, np.inf)  # one ray into the box, should a row ever launch
    dev["rays"][:8] = torch.from_numpy(host["rays"][:8])
    torch.cuda.synchronize()
    for p in names:
        assert dev[p].data_ptr() % 256 == 0
    yield dict(lib=ctx.lib, ctx=ctx, bare=bare, cam=cam, host=host, dev=dev)
    ctx.close()
    bare.close()


def base(entry, w):
    """Valid arguments of a host-path call of `entry`: one ray, or one sample of each of the 8 x 8 pixels."""
    a = {}
    if "cam" in ARGS[entry]:
        a["cam"] = abi.rt_camera_desc.from_buffer_copy(w["cam"])
        a["tiles"] = (abi.rt_tile * 1)(abi.rt_tile(0, 0, 8, 8))
        a["ntiles"] = 1
    if entry == "render_tiles":
        a["prm"] = abi.rt_render_params(spp=1, max_depth=2, seed=1, precision=abi.RT_PREC_F64)
        a["out_dev"] = 0
    elif entry == "render_aov":
        a["prm"] = abi.rt_aov_params(seed=1, spp=1, precision=abi.RT_PREC_F64)
    elif entry == "camera_rays":
        a.update(seed=1, first_sample=0, spp=1, on_device=0)
    else:
        a["prm"] = abi.rt_trace_params(seed=1, precision=abi.RT_PREC_F64)
        a["n"] = 1
    for p in POINTERS[entry]:
        a[p] = w["host"][p].ctypes.data
    a["stream"] = None
    a["_entry"], a["_w"] = entry, w
    return a


# ---- what a row does to the valid arguments
def put(**kw):
    return lambda a: a.update(kw)


def field(arg, name, value):
    return lambda a: setattr(a[arg], name, value)


def on_device(a):
    """The device path: every pointer a device buffer, the flag set."""
    e = a["_entry"]
    for p in POINTERS[e]:
        a[p] = a["_w"]["dev"][p].data_ptr()
    if e == "render_tiles":
        a["out_dev"] = 1
    elif e == "camera_rays":
        a["on_device"] = 1
    else:
        a["prm"].on_device = 1


def misaligned(arg, by=8):
    """The device path with `arg` at a valid device allocation plus `by` bytes."""
    def f(a):
        on_device(a)
        a[arg] += by
    return f


def huge_image(a):  # 65535 x 65535 pixels in one tile: 2^32 - 131071 of them
    a["cam"].image_width = a["cam"].image_height = 65535
    a["tiles"][0] = abi.rt_tile(0, 0, 65535, 65535)


CAM_MODE = [field("cam", "mode", 4)]
CAM_MODE_NEG = [field("cam", "mode", -1)]
EMPTY = [field("cam", "image_width", 0)]
EMPTY_H = [field("cam", "image_height", -3)]
WIDE = [field("cam", "image_width", 65536)]
TALL = [field("cam", "image_height", 65536)]
TILE_OUT = [lambda a: a["tiles"].__setitem__(0, abi.rt_tile(4, 0, 5, 8))]
TILE_NEG = [lambda a: a["tiles"].__setitem__(0, abi.rt_tile(-1, 0, 4, 4))]
NO_TILES = [put(ntiles=0)]
THIN_TILE = [lambda a: a["tiles"].__setitem__(0, abi.rt_tile(3, 3, 0, 5))]


def camera_rows(entry, spp):
    """The camera, tile and spp rows the three entries with a camera share; spp: the row's change that zeroes spp."""
    return [
        (entry, "cam null", [put(cam=None)], "scene", INVALID, M_NULL),
        (entry, "ntiles -1", [put(ntiles=-1)], "scene", INVALID, M_NULL),
        (entry, "camera mode 4", CAM_MODE, "scene", INVALID, M_CAM),
        (entry, "camera mode -1", CAM_MODE_NEG, "scene", INVALID, M_CAM),
        (entry, "image width 0", EMPTY, "scene", INVALID, M_EMPTY),
        (entry, "image height -3", EMPTY_H, "scene", INVALID, M_EMPTY),
        (entry, "image width 65536", WIDE, "scene", INVALID, M_WIDE),
        (entry, "image height 65536", TALL, "scene", INVALID, M_WIDE),
        (entry, "tile past the right edge", TILE_OUT, "scene", INVALID, M_TILE),
        (entry, "tile at x0 -1", TILE_NEG, "scene", INVALID, M_TILE),
        (entry, "spp 0", spp, "scene", INVALID, M_SPP),
        (entry, "bad tile + spp 0", TILE_OUT + spp, "scene", INVALID, M_SPP),
        (entry, "bad camera + bad tile", CAM_MODE + TILE_OUT, "scene", INVALID, M_CAM),
    ]


def ray_rows(entry, outs):
    """The rows rt_trace_rays and rt_occluded share; outs: their output pointers."""
    rows = [
        (entry, "context null", [], "null", INVALID, M_NULL_CTX),
        (entry, "prm null", [put(prm=None)], "scene", INVALID, M_NULL),
        (entry, "rays null", [put(rays=None)], "scene", INVALID, M_NULL),
        (entry, "nrays -1", [put(n=-1)], "scene", INVALID, M_NRAYS),
        (entry, "nrays 2^31", [put(n=1 << 31)], "scene", INVALID, M_NRAYS),
        (entry, "nrays 2^40", [put(n=1 << 40)], "scene", INVALID, M_NRAYS),
        (entry, "precision 2", [field("prm", "precision", 2)], "scene", INVALID, M_PREC),
        (entry, "precision -1", [field("prm", "precision", -1)], "scene", INVALID, M_PREC),
        (entry, "traversal 2", [field("prm", "traversal", 2)], "scene", INVALID, M_TRAV),
        (entry, "traversal -1", [field("prm", "traversal", -1)], "scene", INVALID, M_TRAV),
        (entry, "device rays + 8", [misaligned("rays")], "scene", INVALID, M_ALIGN[entry]),
        (entry, "no scene", [], "bare", NO_SCENE, M_NO_SCENE),
        (entry, "no scene, device path", [on_device], "bare", NO_SCENE, M_NO_SCENE),
        (entry, "no scene, nrays 0", [put(n=0)], "bare", NO_SCENE, M_NO_SCENE),
        # which of two wins
        (entry, "null rays + nrays -1", [put(rays=None, n=-1)], "scene", INVALID, M_NULL),
        (entry, "nrays 2^31 + precision 2", [put(n=1 << 31), field("prm", "precision", 2)], "scene", INVALID, M_NRAYS),
        (entry, "precision 2 + traversal 2", [field("prm", "precision", 2), field("prm", "traversal", 2)], "scene",
         INVALID, M_PREC),
        (entry, "traversal 2 + device rays + 8", [field("prm", "traversal", 2), misaligned("rays")], "scene", INVALID,
         M_TRAV),
        (entry, "no scene + device rays + 8", [misaligned("rays")], "bare", INVALID, M_ALIGN[entry]),
        (entry, "no scene + precision 2", [field("prm", "precision", 2)], "bare", INVALID, M_PREC),
        (entry, "no scene + nrays -1", [put(n=-1)], "bare", INVALID, M_NRAYS),
        (entry, "nrays 0 + device rays + 8", [put(n=0), misaligned("rays")], "scene", INVALID, M_ALIGN[entry]),
        (entry, "nrays 0", [put(n=0)], "scene", OK, None),
        (entry, "nrays 0, device path", [put(n=0), on_device], "scene", OK, None),
    ]
    rows += [(entry, o + " null", [put(**{o: None})], "scene", INVALID, M_NULL) for o in outs]
    return rows


ROWS = (
    # ------------------------------------------------------------ rt_render_tiles
    [("render_tiles", "context null", [], "null", INVALID, M_NULL_CTX),
     ("render_tiles", "prm null", [put(prm=None)], "scene", INVALID, M_NULL),
     ("render_tiles", "tiles null", [put(tiles=None)], "scene", INVALID, M_NULL),
     ("render_tiles", "out null", [put(out=None)], "scene", INVALID, M_NULL),
     ("render_tiles", "no scene", [], "bare", NO_SCENE, M_NO_SCENE),
     ("render_tiles", "no scene, no tiles", NO_TILES, "bare", NO_SCENE, M_NO_SCENE)]
    + camera_rows("render_tiles", [field("prm", "spp", 0)])
    + [("render_tiles", "spp -2", [field("prm", "spp", -2)], "scene", INVALID, M_SPP),
       ("render_tiles", "precision 2", [field("prm", "precision", 2)], "scene", INVALID, M_PREC),
       ("render_tiles", "2^32 pixels", [huge_image], "scene", INVALID, M_PIXELS),
       # which of two wins
       ("render_tiles", "no scene + bad camera", CAM_MODE, "bare", NO_SCENE, M_NO_SCENE),
       ("render_tiles", "no scene + bad tile", TILE_OUT, "bare", NO_SCENE, M_NO_SCENE),
       ("render_tiles", "no scene + cam null", [put(cam=None)], "bare", INVALID, M_NULL),
       ("render_tiles", "bad camera + spp 0", CAM_MODE + [field("prm", "spp", 0)], "scene", INVALID, M_CAM),
       ("render_tiles", "spp 0 + precision 2", [field("prm", "spp", 0), field("prm", "precision", 2)], "scene", INVALID,
        M_SPP),
       ("render_tiles", "precision 2 + bad tile", [field("prm", "precision", 2)] + TILE_OUT, "scene", INVALID, M_PREC),
       # nothing to render; no tiles need no tile list and no output either
       ("render_tiles", "no tiles", NO_TILES, "scene", OK, None),
       ("render_tiles", "no tiles, null list and output", [put(ntiles=0, tiles=None, out=None)], "scene", OK, None),
       ("render_tiles", "no tiles, device output", NO_TILES + [on_device], "scene", OK, None),
       ("render_tiles", "a tile of no width", THIN_TILE, "scene", OK, None),
       ("render_tiles", "no tiles, fp32", NO_TILES + [field("prm", "precision", abi.RT_PREC_F32)], "scene", OK, None),
       ("render_tiles", "no tiles, traversal 2 (unchecked)", NO_TILES + [field("prm", "traversal", 2)], "scene", OK,
        None)]
    # ------------------------------------------------------------ rt_trace_rays, rt_occluded
    + ray_rows("trace_rays", ("geom", "ids"))
    + [("trace_rays", "device out_ids + 8", [misaligned("ids")], "scene", INVALID, M_ALIGN["trace_rays"]),
       ("trace_rays", "device out_geom + 4", [misaligned("geom", 4)], "scene", INVALID, M_ALIGN["trace_rays"]),
       ("trace_rays", "no scene + device out_ids + 8", [misaligned("ids")], "bare", INVALID, M_ALIGN["trace_rays"]),
       ("trace_rays", "no scene, device out_geom + 8 (aligned enough)", [misaligned("geom")], "bare", NO_SCENE,
        M_NO_SCENE)]
    + ray_rows("occluded", ("out",))
    + [("occluded", "no scene, device out + 1 (bytes: no alignment)", [misaligned("out", 1)], "bare", NO_SCENE,
        M_NO_SCENE)]
    # ------------------------------------------------------------ rt_camera_rays
    + [("camera_rays", "context null", [], "null", INVALID, M_NULL_CTX),
       ("camera_rays", "tiles null", [put(tiles=None)], "scene", INVALID, M_NULL),
       ("camera_rays", "tiles null, no tiles", [put(tiles=None, ntiles=0)], "scene", INVALID, M_NULL),
       ("camera_rays", "out null", [put(out=None)], "scene", INVALID, M_NULL)]
    + camera_rows("camera_rays", [put(spp=0)])
    + [("camera_rays", "spp -2", [put(spp=-2)], "scene", INVALID, M_SPP),
       ("camera_rays", "device out_rays + 8", [misaligned("out")], "scene", INVALID, M_ALIGN["camera_rays"]),
       ("camera_rays", "2^32 pixels", [huge_image], "scene", INVALID, M_NPIX),
       ("camera_rays", "64 pixels of 2^25 samples", [put(spp=1 << 25)], "scene", INVALID, M_NPIX),
       # which of two wins
       ("camera_rays", "bad camera + spp 0", CAM_MODE + [put(spp=0)], "scene", INVALID, M_SPP),
       ("camera_rays", "spp 0 + device out_rays + 8", [put(spp=0), misaligned("out")], "scene", INVALID, M_SPP),
       ("camera_rays", "device out_rays + 8 + bad camera", [misaligned("out")] + CAM_MODE, "scene", INVALID,
        M_ALIGN["camera_rays"]),
       ("camera_rays", "no scene + bad camera", CAM_MODE, "bare", INVALID, M_CAM),
       ("camera_rays", "no scene + bad tile", TILE_OUT, "bare", INVALID, M_TILE),
       # nothing to do, and no scene needed for it
       ("camera_rays", "no tiles", NO_TILES, "scene", OK, None),
       ("camera_rays", "no tiles, device path", NO_TILES + [on_device], "scene", OK, None),
       ("camera_rays", "a tile of no width", THIN_TILE, "scene", OK, None),
       ("camera_rays", "no scene, no tiles", NO_TILES, "bare", OK, None)]
    # ------------------------------------------------------------ rt_render_aov
    + [("render_aov", "context null", [], "null", INVALID, M_NULL_CTX),
       ("render_aov", "prm null", [put(prm=None)], "scene", INVALID, M_NULL),
       ("render_aov", "tiles null", [put(tiles=None)], "scene", INVALID, M_NULL),
       ("render_aov", "tiles null, no tiles", [put(tiles=None, ntiles=0)], "scene", INVALID, M_NULL),
       ("render_aov", "feat null", [put(feat=None)], "scene", INVALID, M_NULL),
       ("render_aov", "ids null", [put(ids=None)], "scene", INVALID, M_NULL)]
    + camera_rows("render_aov", [field("prm", "spp", 0)])
    + [("render_aov", "spp -2", [field("prm", "spp", -2)], "scene", INVALID, M_SPP),
       ("render_aov", "precision 2", [field("prm", "precision", 2)], "scene", INVALID, M_PREC),
       ("render_aov", "traversal 2", [field("prm", "traversal", 2)], "scene", INVALID, M_TRAV),
       ("render_aov", "device out_feat + 8", [misaligned("feat")], "scene", INVALID, M_ALIGN["render_aov"]),
       ("render_aov", "device out_ids + 8", [misaligned("ids")], "scene", INVALID, M_ALIGN["render_aov"]),
       ("render_aov", "no scene", [], "bare", NO_SCENE, M_NO_SCENE),
       ("render_aov", "no scene, no tiles", NO_TILES, "bare", NO_SCENE, M_NO_SCENE),
       ("render_aov", "2^32 pixels", [huge_image], "scene", INVALID, M_NPIX),
       ("render_aov", "64 pixels of 2^25 samples", [field("prm", "spp", 1 << 25)], "scene", INVALID, M_NPIX),
       # which of two wins
       ("render_aov", "no scene + bad camera", CAM_MODE, "bare", INVALID, M_CAM),
       ("render_aov", "no scene + bad tile", TILE_OUT, "bare", INVALID, M_TILE),
       ("render_aov", "no scene + device out_feat + 8", [misaligned("feat")], "bare", INVALID, M_ALIGN["render_aov"]),
       ("render_aov", "no scene + 2^32 pixels", [huge_image], "bare", NO_SCENE, M_NO_SCENE),
       ("render_aov", "bad camera + spp 0", CAM_MODE + [field("prm", "spp", 0)], "scene", INVALID, M_SPP),
       ("render_aov", "spp 0 + precision 2", [field("prm", "spp", 0), field("prm", "precision", 2)], "scene", INVALID,
        M_SPP),
       ("render_aov", "precision 2 + traversal 2", [field("prm", "precision", 2), field("prm", "traversal", 2)], "scene",
        INVALID, M_PREC),
       ("render_aov", "precision 2 + bad tile", [field("prm", "precision", 2)] + TILE_OUT, "scene", INVALID, M_PREC),
       ("render_aov", "traversal 2 + device out_ids + 8", [field("prm", "traversal", 2), misaligned("ids")], "scene",
        INVALID, M_TRAV),
       ("render_aov", "device out_ids + 8 + bad camera", [misaligned("ids")] + CAM_MODE, "scene", INVALID,
        M_ALIGN["render_aov"]),
       # nothing to do
       ("render_aov", "no tiles", NO_TILES, "scene", OK, None),
       ("render_aov", "no tiles, device path", NO_TILES + [on_device], "scene", OK, None),
       ("render_aov", "a tile of no width", THIN_TILE, "scene", OK, None)]
)


def call(w, entry, changes, which):
    a = base(entry, w)
    for ch in changes:
        ch(a)
    h = {"scene": w["ctx"].h, "bare": w["bare"].h, "null": None}[which]
    args = []
    for name in ARGS[entry]:
        v = a[name]
        args.append(ctypes.byref(v) if isinstance(v, ctypes.Structure) else v)
    st = getattr(w["lib"], "rt_" + entry)(h, *args)
    return st, w["lib"].rt_last_error(h).decode()


def test_every_row_is_distinct():
    ids = [(e, label) for e, label, *_ in ROWS]
    assert len(set(ids)) == len(ids)
    assert {e for e, _ in ids} == set(ARGS)


@pytest.mark.parametrize("entry", sorted(ARGS))
def test_refusals_and_empty_calls(world, entry):
    """Every row of `entry`: the status, the text, and across the whole table not one launch."""
    rows = [r for r in ROWS if r[0] == entry]
    assert len(rows) >= 20
    before = {k: world[k].stats().launches for k in ("ctx", "bare")}
    got = []
    for _, label, changes, which, status, msg in rows:
        st, text = call(world, entry, changes, which)
        got.append((label, st, text if msg is not None else None))
    want = [(label, status, msg) for _, label, _, _, status, msg in rows]
    wrong = [(g, w_) for g, w_ in zip(got, want) if g != w_]
    assert not wrong, "\n".join(f"rt_{entry} [{w_[0]}]: got {g[1:]}, expected {w_[1:]}" for g, w_ in wrong)
    for k in ("ctx", "bare"):
        assert world[k].stats().launches == before[k], f"rt_{entry}: a row launched on the {k} context"

