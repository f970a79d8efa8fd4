"""Light sampling on the device against the oracle, for every kind of light, every orientation of an axis-aligned
quad light and every path-kernel form that samples one (rt_device.h light_pdf / light_pdf_aligned / light_random,
scene_compile.cpp light_from). The scenes are light_scenes.py's; test_light_scenes.py pins them on the CPU.

TABLE lists (scene, precision, traversal, schedule) -> the tag Context.last_kernel() must report, written out as
rt_plan.h path_kernel selects at the time of writing (test_plan_tables.py holds that function to every row without a
GPU; here the tag is the launched kernel's own): a silent change of selection fails here, and a
test that believes it runs a form knows that it does. test_table_covers_every_light_and_form holds the table itself
to its coverage: every Light::aligned code 1..6, with extents of both signs, in each form of FORMS and both
precisions, and the off-axis, sphere and base-class lights in the families named there.

Each row is one small frame (16 spp, depth 8) rendered by the oracle and by the device:
 - fp64: |d| <= 1e-9 max(1, |ref|); a list, linear or flat scene may miss it in at most 2 pixels, a
   BVH scene in under 5e-3 of its pixels (exact-t ties between the SAH tree and the reference's x-median tree:
   test_wide_fp64_matches_binary_and_oracle's bound).
 - fp32: a pixel is divergent when |d| > 1e-3 (test_fp32_divergent_samples_are_rare's threshold): at most 2 of a
   32x32 frame, at most 1 % of a 64x64 BVH frame (the share test_gloss_matches_oracle allows); over the other
   pixels the per-channel RMSE is below 1e-4.
 - the base-class light over a flat ground, and over triangles seen from behind: the reference's 0 / 0 makes pixels
   NaN. fp64: the device's NaN mask is the oracle's (in the BVH frame a pixel whose mask differs is a missed pixel).
   fp32: a zero mixture pdf ends the path (the documented deviation), so the image is finite everywhere and the
   pixels finite in the oracle are held to the fp32 rule.
 - every oracle frame is lit: mean > 0.05 over its finite pixels.
"""
import numpy as np
import pytest

import light_scenes as L
import oracle
import rt_amd
from rt_amd import abi

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
AUTO, ORDERED = abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED
PERSIST, STEP = 0, 4  # segments_per_launch
SPP, DEPTH, SEED = 16, 8, 11
P = {F32: "f32", F64: "f64"}

# ------------------------------------------------------------------ the forms an aligned quad light is held in
# form -> (scene family, variant, traversal, schedule, tag with the precision left open)
FORMS = {
    "flat_ll": ("room", "ll", AUTO, PERSIST, "FlatTrav<{p},1,1> persist"),             # tables in LDS
    "flat_general": ("room", "metal", AUTO, PERSIST, "FlatTrav<{p},1,0> persist"),     # tables in LDS
    "flat_global": ("room", "ll", AUTO, STEP, "FlatTrav<{p},0,0> step"),               # records in global memory
    "linear_quads": ("room", "ll", ORDERED, PERSIST, "LinearTrav<{p},0,0,0,0> persist"),
    "linear_lli": ("room", "smoke", AUTO, PERSIST, "LinearTrav<{p},0,0,1,1> persist"),
    "linear_vol_general": ("room", "smoke", AUTO, STEP, "LinearTrav<{p},0,0,1,0> step"),
    "wide_ll": ("mesh", "ll", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,1,1,0> persist"),   # the tree in LDS
    "wide_general": ("mesh", "metal", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,1,0,0> persist"),
    "binary": ("mesh", "ll", ORDERED, PERSIST, None),                                  # tag by precision: BINARY
}
# the binary BVH: fp32 with its nodes in LDS (at most 256 nodes, stack <= 16); fp64 by the stack the tree needs (9 to
# 11 entries in the mesh and sphere scenes, 8 in the base-light scene, which the table writes out)
BINARY = {F32: "StackTrav<f32,16,1> persist", F64: "StackTrav<f64,16,0> persist"}


def rooms_by_pair():
    """(axis of u, axis of v) of the light -> the indices of L.MATRICES that give it, in order."""
    out = {}
    for i, M in enumerate(L.MATRICES):
        _, u, v = L.light_quad(L.room(M, "ll")[0])
        out.setdefault((L.axis_of(u)[0], L.axis_of(v)[0]), []).append(i)
    return out


ROOMS_BY_PAIR = rooms_by_pair()


def scene(key):
    """key: "room/<matrix index>/<variant>", "mesh/<u><v>/<variant>", "terrain/<u><v>", "sphere/<variant>",
    "base/<variant>" -> (desc, cam)."""
    w = key.split("/")
    if w[0] == "room":
        return L.room(L.MATRICES[int(w[1])], w[2])
    if w[0] == "mesh":
        return L.mesh((int(w[1][0]), int(w[1][1])), w[2])
    if w[0] == "terrain":
        return L.terrain_hbm((int(w[1][0]), int(w[1][1])), width=64)
    if w[0] == "sphere":
        return L.sphere_light(w[1], width=64 if w[1] == "bvh" else 32)
    assert w[0] == "base", key
    return L.base_light(w[1], width=64 if w[1] == "bvh" else 32)


def is_bvh(key):
    return key.split("/")[0] in ("mesh", "terrain") or key in ("sphere/bvh", "base/bvh")


def build_table():
    """-> rows (scene, precision, traversal, schedule, tag, form or None)."""
    rows = []
    # all 24 rooms on the default path
    for i in range(len(L.MATRICES)):
        for prec in (F32, F64):
            rows.append((f"room/{i}/ll", prec, AUTO, PERSIST, FORMS["flat_ll"][4].format(p=P[prec]), "flat_ll"))
    # the other forms: one scene per (U, V) pair; the rooms alternate through the matrices of their pair (two sign
    # sets each, every extent of either sign in one of them), so negative extents reach every form
    for f, (name, (family, variant, trav, sched, tag)) in enumerate(FORMS.items()):
        for k, uv in enumerate(L.UV_PAIRS):
            if name == "flat_ll":
                continue
            key = (f"room/{ROOMS_BY_PAIR[uv][(f + k) % len(ROOMS_BY_PAIR[uv])]}/{variant}" if family == "room" else
                   f"mesh/{uv[0]}{uv[1]}/{variant}")
            for prec in (F32, F64):
                rows.append((key, prec, trav, sched, (tag or BINARY[prec]).format(p=P[prec]), name))
    # the rest, written out: (scene, traversal, schedule, tag, precisions)
    both = (F32, F64)
    rest = [
        # the wide tree in HBM under a light on an x plane (aligned 4 and 6)
        ("terrain/12", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,0,0,0> persist", both),
        ("terrain/21", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,0,0,0> persist", both),
        # either side of n_mats <= 16: the flat LL form, the LLI form, the wide LL form
        ("room/5/mats16", AUTO, PERSIST, "FlatTrav<{p},1,1> persist", both),
        ("room/5/mats17", AUTO, PERSIST, "FlatTrav<{p},1,0> persist", both),
        ("room/14/smoke16", AUTO, PERSIST, "LinearTrav<{p},0,0,1,1> persist", both),
        ("room/14/smoke17", AUTO, PERSIST, "LinearTrav<{p},0,0,1,0> persist", both),
        ("mesh/12/mats16", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,1,1,0> persist", both),
        ("mesh/12/mats17", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,1,0,0> persist", both),
        # a parallelogram light off the axes: a member of a quad room (no flat program), of the smoke room, of the
        # mesh (wide tree and binary BVH), and apart from the world over the ll room (the flat program's general form;
        # fp32 takes the "sampled direction hits at t = 1" shortcut)
        ("room/5/offaxis", AUTO, PERSIST, "LinearTrav<{p},0,0,0,0> persist", both),
        ("room/18/offaxis", AUTO, STEP, "LinearTrav<{p},0,0,0,0> step", both),
        ("room/5/offaxis_smoke", AUTO, PERSIST, "LinearTrav<{p},0,0,1,0> persist", both),
        ("mesh/02/offaxis", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,1,0,0> persist", both),
        ("mesh/02/offaxis", ORDERED, PERSIST, None, both),
        ("room/5/offaxis_apart", AUTO, PERSIST, "FlatTrav<{p},1,0> persist", both),
        ("room/18/offaxis_apart", AUTO, STEP, "FlatTrav<{p},0,0> step", both),
        # a sphere light: the list of spheres, a quad room (spheres and quads), the smoke room (all kinds), apart from
        # the world over the ll room (the flat program), 150 spheres under a bvh_node (the wide kernel of spheres
        # without NL, and the binary BVH), and a moving sphere (centre 0; fp64 only: the reference's normals of a
        # moving sphere make radiance ill-conditioned in fp32, test_wide_mixed_primitives_match_oracle)
        ("sphere/list", AUTO, PERSIST, "LinearTrav<{p},1,0,0,0> persist", both),
        ("sphere/list", AUTO, STEP, "LinearTrav<{p},1,0,0,0> step", both),
        ("room/5/sphere", AUTO, PERSIST, "LinearTrav<{p},1,0,0,0> persist", both),
        ("room/5/sphere_smoke", AUTO, PERSIST, "LinearTrav<{p},1,1,1,0> persist", both),
        ("room/5/sphere_apart", AUTO, PERSIST, "FlatTrav<{p},1,0> persist", both),
        ("sphere/bvh", AUTO, PERSIST, "WideTrav<{p},1,0,0,0,1,0,0> persist", both),
        ("sphere/bvh", ORDERED, PERSIST, None, both),
        ("sphere/moving", AUTO, PERSIST, "LinearTrav<{p},1,0,0,0> persist", (F64,)),
        # the base-class light: the linear program (tilted ground), the flat program in LDS and in global memory and
        # the linear program (flat ground)
        ("base/tilted", AUTO, PERSIST, "LinearTrav<{p},0,0,0,0> persist", both),
        ("base/flat", AUTO, PERSIST, "FlatTrav<{p},1,0> persist", both),
        ("base/flat", AUTO, STEP, "FlatTrav<{p},0,0> step", both),
        ("base/flat", ORDERED, PERSIST, "LinearTrav<{p},0,0,0,0> persist", both),
        # ... and under a bvh_node: the wide tree's general triangle + quad kernel and the binary BVH
        ("base/bvh", AUTO, PERSIST, "WideTrav<{p},0,1,1,0,1,0,0> persist", both),
        ("base/bvh", ORDERED, PERSIST, {F32: "StackTrav<f32,16,1> persist", F64: "StackTrav<f64,8,0> persist"}, both),
    ]
    for key, trav, sched, tag, precs in rest:
        for prec in precs:
            tag_p = tag[prec] if isinstance(tag, dict) else (tag or BINARY[prec])
            rows.append((key, prec, trav, sched, tag_p.format(p=P[prec]), None))
    return rows


TABLE = build_table()


def row_id(r):
    return f"{r[0]}-{P[r[1]]}-{'ordered' if r[2] == ORDERED else 'auto'}-{'step' if r[3] else 'persist'}"


def light_class(key):
    """-> ("aligned", code, sign of u's extent, sign of v's), ("offaxis",), ("sphere",) or ("base",)."""
    desc, _ = scene(key)
    o = desc.objects[desc.light]
    if o.kind == abi.RT_OBJ_SPHERE:
        return ("sphere",)
    if o.kind != abi.RT_OBJ_QUAD:
        return ("base",)
    u, v = np.array(o.b[:]), np.array(o.c[:])
    if np.count_nonzero(u) != 1 or np.count_nonzero(v) != 1:
        return ("offaxis",)
    (U, su), (V, sv) = L.axis_of(u), L.axis_of(v)
    return ("aligned", 1 + L.UV_PAIRS.index((U, V)), su, sv)


def family_of(tag):
    return tag.split("<")[0]


def test_table_covers_every_light_and_form():
    cls = {key: light_class(key) for key in {r[0] for r in TABLE}}
    for name in FORMS:
        for prec in (F32, F64):
            seen = [cls[r[0]] for r in TABLE if r[5] == name and r[1] == prec]
            assert all(c[0] == "aligned" for c in seen)
            assert {c[1] for c in seen} == {1, 2, 3, 4, 5, 6}, (name, prec)
            assert {c[2] for c in seen} == {1, -1} and {c[3] for c in seen} == {1, -1}, (name, prec)
    # the default path: every code with every sign pair its rooms have (two of the four each)
    seen = {cls[r[0]][1:] for r in TABLE if r[5] == "flat_ll" and r[1] == F64}
    assert len(seen) == 12 and all(sum(1 for s in seen if s[0] == code) == 2 for code in range(1, 7))
    # the tree in HBM: a light on an x plane (aligned 4 and 6, not the y plane's 2 of every earlier test)
    assert {cls[r[0]][1] for r in TABLE if r[0].startswith("terrain/")} == {4, 6}
    reach = {"offaxis": {"FlatTrav", "LinearTrav", "WideTrav", "StackTrav"},
             "sphere": {"FlatTrav", "LinearTrav", "WideTrav", "StackTrav"},
             "base": {"FlatTrav", "LinearTrav", "WideTrav", "StackTrav"}}
    for kind, fams in reach.items():
        for prec in (F32, F64):
            got = {family_of(r[4]) for r in TABLE if cls[r[0]][0] == kind and r[1] == prec}
            assert got == fams, (kind, prec, got)
    # the forms by tag: each of these kernels is in the table in both precisions
    for tag in ("FlatTrav<{p},1,1> persist", "FlatTrav<{p},1,0> persist", "FlatTrav<{p},0,0> step",
                "LinearTrav<{p},0,0,0,0> persist", "LinearTrav<{p},0,0,1,1> persist", "LinearTrav<{p},0,0,1,0> persist",
                "LinearTrav<{p},0,0,1,0> step", "LinearTrav<{p},1,0,0,0> persist", "LinearTrav<{p},1,1,1,0> persist",
                "WideTrav<{p},0,1,1,0,1,1,0> persist", "WideTrav<{p},0,1,1,0,1,0,0> persist",
                "WideTrav<{p},0,1,1,0,0,0,0> persist", "WideTrav<{p},1,0,0,0,1,0,0> persist"):
        for prec in (F32, F64):
            assert any(r[4] == tag.format(p=P[prec]) for r in TABLE), tag


# ------------------------------------------------------------------ renders
@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """scene key -> (desc, cam, oracle frame): rendered once per scene, never changed."""
    cache = {}

    def get(key):
        if key not in cache:
            desc, cam = scene(key)
            ref, _ = oracle.render(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=8)
            ref.setflags(write=False)
            cache[key] = (desc, cam, ref)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def measured():
    """What the rows measured, printed once at the end (DESIGN.md section 6 quotes the maxima)."""
    m = {}
    yield m
    for group, vals in sorted(m.items()):
        print(f"[lights] {group}: " + ", ".join(f"{k} max {max(v):.3g}" for k, v in sorted(vals.items())))


def note(measured, group, **kw):
    for k, v in kw.items():
        measured.setdefault(group, {}).setdefault(k, []).append(float(v))


def render(ctx, cam, prec, trav, sched, **kw):
    return ctx.render(cam, SPP, DEPTH, seed=SEED, precision=prec, traversal=trav, segments_per_launch=sched, **kw)


def check_against_oracle(key, prec, img, ref, measured, rid, bvh=None, specular=False, group=None):
    """The module docstring's rules for one frame. test_gpu_materials.py holds its rows to them too: it says itself
    whether its scene is a BVH scene (bvh; None: is_bvh(key)), names its group of measurements, and sets specular for
    a frame with metal, dielectric or gloss-specular bounces, whose fp32 cap is 1 % of the pixels at any size (the
    share test_gloss_matches_oracle allows)."""
    bvh = is_bvh(key) if bvh is None else bvh
    npix = ref.shape[0] * ref.shape[1]
    fin = np.isfinite(ref).all(-1)
    assert ref[fin].mean() > 0.05, "the frame is not lit"
    if key in ("base/flat", "base/bvh"):
        assert 0.2 < fin.mean() < 0.8, fin.mean()  # NaN pixels and finite pixels: neither check below is vacuous
    else:
        assert fin.all()
    group = (group or ("bvh" if bvh else "list")) + " " + P[prec]
    img = np.asarray(img, np.float64)
    if prec == F64:
        other = np.isfinite(img).all(-1) != fin
        if not bvh:  # (in a BVH frame a tie may change a pixel's mask: it counts as a missed pixel)
            assert not other.any(), f"the NaN mask differs from the oracle's in {int(other.sum())} pixels"
        both = fin & ~other
        rel = np.abs(img[both] - ref[both]) / np.maximum(1.0, np.abs(ref[both]))
        miss = int((rel > 1e-9).any(-1).sum()) + int(other.sum())
        print(f"{rid}: fp64 max rel err {rel.max():.2e}, pixels beyond 1e-9: {miss} of {npix}")
        note(measured, group, rel_err=np.where(rel > 1e-9, 0.0, rel).max(), missed_pixels=miss)
        if bvh:
            assert miss < 5e-3 * npix, (miss, float(rel.max()))
        else:
            assert miss <= 2, (miss, float(rel.max()))
        return
    assert np.isfinite(img).all(), "fp32: a zero mixture pdf ends the path, no pixel is NaN"
    d = np.abs(img[fin] - ref[fin])
    div = (d > 1e-3).any(-1)
    rmse = np.sqrt((d[~div] ** 2).mean(0))
    print(f"{rid}: fp32 divergent pixels {int(div.sum())} of {npix}, rmse over the others {rmse}")
    note(measured, group, divergent_pixels=div.sum(), rmse=rmse.max())
    cap = 0.01 * npix if (bvh or specular) else 2
    assert div.sum() <= cap, int(div.sum())
    assert (rmse < 1e-4).all(), rmse


@pytest.mark.parametrize("row", TABLE, ids=row_id)
def test_light_matches_the_oracle(ctx, refs, measured, row):
    key, prec, trav, sched, tag, _ = row
    desc, cam, ref = refs(key)
    ctx.upload(desc)
    img = render(ctx, cam, prec, trav, sched)
    assert ctx.last_kernel() == tag
    check_against_oracle(key, prec, img, ref, measured, row_id(row))


def shade_form(tag):
    """The shade program a tag names: the traversal family and its LL / LLI / NL arguments."""
    name, args = tag.split(" ")[0].rstrip(">").split("<")
    a = args.split(",")[1:]
    return {"FlatTrav": lambda: ("flat", a[1]), "LinearTrav": lambda: ("linear", a[3]),
            "WideTrav": lambda: ("wide", a[5], a[6]), "StackTrav": lambda: ("stack",)}[name]()


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("key,trav", [("room/9/metal", AUTO), ("mesh/21/metal", ORDERED)])
def test_schedules_give_the_same_image(ctx, key, trav, prec):
    # the persistent and the wavefront schedule run the same shade form here (the general one): bit-equal images
    desc, cam = scene(key)
    ctx.upload(desc)
    persistent = render(ctx, cam, prec, trav, PERSIST)
    tag_p = ctx.last_kernel()
    wavefront = render(ctx, cam, prec, trav, STEP)
    tag_w = ctx.last_kernel()
    assert tag_p.endswith(" persist") and tag_w.endswith(" step") and shade_form(tag_p) == shade_form(tag_w), (tag_p, tag_w)
    assert persistent.max() > 0 and np.array_equal(persistent, wavefront)


@pytest.mark.parametrize("key,depth,trav,sched", [("base/flat", 1, AUTO, PERSIST), ("base/flat", 1, AUTO, STEP),
                                                  ("base/flat", 1, ORDERED, PERSIST), ("base/bvh", 2, AUTO, PERSIST),
                                                  ("base/bvh", 2, ORDERED, PERSIST)])
def test_a_zero_over_zero_weight_on_the_last_bounce_is_nan_in_fp64(ctx, key, depth, trav, sched):
    # At depth 1 every path ends at the depth cap on its first hit (the flat ground: (1, 0, 0) lies in its plane); at
    # depth 2 on its second (the triangles: met from behind after the first bounce). ray_color(.., 0) returns 0 and
    # the caller multiplies it by the bounce's weight (camera.h:238), the 0 / 0 of the base-class light wherever the
    # light half of the mixture was drawn and (1, 0, 0) is not above the surface. fp64 keeps that NaN (the general
    # shade forms; the LL and NL forms have no such light); fp32 ends the path at the zero pdf and stays finite.
    desc, cam = scene(key)
    ref, _ = oracle.render(oracle.from_desc(desc), cam, SPP, depth, seed=SEED, threads=8)
    fin = np.isfinite(ref).all(-1)
    assert 0.2 < fin.mean() < 0.8, fin.mean()
    ctx.upload(desc)
    img = ctx.render(cam, SPP, depth, seed=SEED, precision=F64, traversal=trav, segments_per_launch=sched)
    other = int((np.isfinite(img).all(-1) != fin).sum())
    assert other == 0, f"the NaN mask differs from the oracle's in {other} pixels"
    assert (np.abs(img[fin] - ref[fin]) <= 1e-9 * np.maximum(1.0, np.abs(ref[fin]))).all()
    img32 = ctx.render(cam, SPP, depth, seed=SEED, precision=F32, traversal=trav, segments_per_launch=sched)
    divergent = int((np.abs(img32[fin] - ref[fin]) > 1e-3).any(-1).sum())
    assert np.isfinite(img32).all() and divergent <= (0.01 * fin.size if is_bvh(key) else 2), divergent
