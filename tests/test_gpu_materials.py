"""Every material's scatter on the device against the oracle, in every path-kernel form that shades it (rt_kernels.hip
shade: emission, lambertian, metal, dielectric, gloss, isotropic, own_pdf without a light, the miss paths). The scenes
are material_scenes.py's; test_material_scenes.py pins them on the CPU and counts, with the oracle's event counters,
the branches each one reaches.

TABLE lists (scene, precision, traversal, segments_per_launch, camera or None) -> the tag Context.last_kernel() must
report, written out by hand from rt_plan.h path_kernel (test_plan_tables.py holds that function to every row without a
GPU; here the tag is the launched kernel's own): a silent change of selection fails here, and a row that believes it
runs a form knows that it does. test_table_covers_every_branch_and_form holds the
table to its coverage: each event of REQUIRED, by the CPU test's counts, in a row of each shade form that compiles the
branch in, in both precisions; and, with test_gpu_lights.py's table, every tag launch_step can launch
(kernel_tags.all_tags): LEFT_OUT, the tags no row launches with their reasons, is empty.

Each row is one small frame (16 spp, depth 8), held to test_gpu_lights.check_against_oracle's rules:
 - fp64: |d| <= 1e-9 max(1, |ref|); a flat, list or linear scene may miss it in at most 2 pixels, a BVH scene in under
   5e-3 of its pixels. The segment counter obeys 0 < segments <= the oracle's, with equality in a scene without a
   light (test_fp64_device_matches_oracle's rule).
 - fp32: a pixel is divergent when |d| > 1e-3. A row without a metal, dielectric or gloss-specular event: at most 2
   pixels of 32 x 32 (1 % of a BVH frame); a row with one: at most 1 % of the pixels (test_gloss_matches_oracle's
   share). The per-channel RMSE over the other pixels is below 1e-4.
"""
import re

import numpy as np
import pytest

import material_scenes as S
from kernel_tags import (FLAT_GLOBAL, FLAT_LDS, FLAT_LL, LIN_ALL, LIN_LLI, LIN_QUAD, LIN_SPH, LIN_VOL, W_ALL, W_ALL_HBM,
                         W_SPH, W_SPH_HBM, W_SPH_NL, W_SPH_NL_HBM, W_TQ, W_TQ_HBM, W_TQ_LL, W_TQ_LL_HBM, W_TRI,
                         W_TRI_HBM, all_tags)
import oracle
import rt_amd
import test_gpu_lights as lights
import test_material_scenes as cpu
from rt_amd import abi
from test_gpu_lights import check_against_oracle

pytestmark = pytest.mark.gpu

F32, F64 = abi.RT_PREC_F32, abi.RT_PREC_F64
AUTO, ORDERED = abi.RT_TRAV_AUTO, abi.RT_TRAV_ORDERED
PERSIST, STEP = 0, 4  # segments_per_launch
SPP, DEPTH, SEED = cpu.SPP, cpu.DEPTH, cpu.SEED
P = {F32: "f32", F64: "f64"}
BOTH = (F32, F64)

# ------------------------------------------------------------------ the traversals by name
# (FLAT_*, LIN_*, W_*: kernel_tags.py)
# the binary BVH of a scene, by precision: fp32 keeps at most 256 nodes in LDS when the stack needs at most 16 entries;
# otherwise the stack the tree needs (8, 16 or 32 entries)
B_SMALL = {F32: "StackTrav<f32,16,1>", F64: "StackTrav<f64,8,0>"}    # spheres_small, mixed: 34 to 43 nodes, 8 entries
B_MID = {F32: "StackTrav<f32,16,1>", F64: "StackTrav<f64,16,0>"}     # mesh: under 256 nodes, 9 to 11 entries
B_LARGE = {F32: "StackTrav<f32,16,0>", F64: "StackTrav<f64,16,0>"}   # spheres_nl_hbm: 1,022 nodes, 15 entries
B_DEEP = {F32: "StackTrav<f32,32,0>", F64: "StackTrav<f64,32,0>"}    # mesh_deep: 19 entries
# more than 256 nodes on 8 entries: no single tree (8 entries are at most 7 levels, 127 nodes), but many small ones, each
# translate's own, whose nodes add up while the need grows with the nesting alone (instanced: 401 nodes)
B_INST = {F32: "StackTrav<f32,8,0>", F64: "StackTrav<f64,8,0>"}

# (scene, traversal, segments_per_launch, camera or None, traversal tag, "camx" or "", precisions)
ROWS = [
    # ---- the flat program. LL: lambertian + light only; its tables in LDS hold 32 materials and 64 quads (fp64 holds the
    # room's five walls as one room record, so its 64th quad is the scene's 69th); past them the records stay in global
    # memory; the wavefront schedule reads them there too
    ("backlight", AUTO, PERSIST, None, FLAT_LL, "", BOTH),
    ("glass", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("glass_neg", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("glass067", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("gloss", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("metal", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("nolight", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("nolight_checker", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("dark", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("nobg", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("backlight_metal", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("checker_light", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("mats32", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("mats33", AUTO, PERSIST, None, FLAT_GLOBAL, "", BOTH),
    ("quads64", AUTO, PERSIST, None, FLAT_LDS, "", BOTH),
    ("quads65", AUTO, PERSIST, None, FLAT_GLOBAL, "", (F32,)),
    ("quads65", AUTO, PERSIST, None, FLAT_LDS, "", (F64,)),
    ("quads69", AUTO, PERSIST, None, FLAT_GLOBAL, "", (F32,)),
    ("quads69", AUTO, PERSIST, None, FLAT_LDS, "", (F64,)),
    ("quads70", AUTO, PERSIST, None, FLAT_GLOBAL, "", BOTH),
    ("glass", AUTO, STEP, None, FLAT_GLOBAL, "", BOTH),
    ("gloss", AUTO, STEP, None, FLAT_GLOBAL, "", BOTH),
    ("metal", AUTO, STEP, None, FLAT_GLOBAL, "", BOTH),
    ("nolight", AUTO, STEP, None, FLAT_GLOBAL, "", BOTH),
    # ---- the linear program of quads: instances, and the flat scenes in reference order
    ("glass_rot", AUTO, PERSIST, None, LIN_QUAD, "", BOTH),
    ("glass067_rot", AUTO, PERSIST, None, LIN_QUAD, "", BOTH),
    ("gloss_rot", AUTO, PERSIST, None, LIN_QUAD, "", BOTH),
    ("glass", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("metal", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("nolight", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("nolight_checker", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("dark", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("nobg", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("checker_light", ORDERED, PERSIST, None, LIN_QUAD, "", BOTH),
    ("glass_rot", AUTO, STEP, None, LIN_QUAD, "", BOTH),
    ("gloss_rot", AUTO, STEP, None, LIN_QUAD, "", BOTH),
    ("metal", ORDERED, STEP, None, LIN_QUAD, "", BOTH),
    # ... and its extended form: another camera, or a picture or noise texture (which also end the flat program)
    ("glass", AUTO, PERSIST, "orthonormal", LIN_QUAD, "camx", BOTH),
    ("gloss", AUTO, PERSIST, "fisheye", LIN_QUAD, "camx", BOTH),
    ("metal", AUTO, PERSIST, "lens", LIN_QUAD, "camx", BOTH),
    ("nolight", AUTO, PERSIST, "fisheye", LIN_QUAD, "camx", BOTH),
    ("glass_image", AUTO, PERSIST, None, LIN_QUAD, "camx", BOTH),
    ("metal_perlin", AUTO, PERSIST, None, LIN_QUAD, "camx", BOTH),
    ("gloss_value", AUTO, PERSIST, None, LIN_QUAD, "camx", BOTH),
    ("glass_worley", AUTO, PERSIST, None, LIN_QUAD, "camx", BOTH),
    ("glass_image", AUTO, STEP, None, LIN_QUAD, "camx", BOTH),
    ("metal_perlin", AUTO, STEP, None, LIN_QUAD, "camx", BOTH),
    ("gloss", AUTO, STEP, "fisheye", LIN_QUAD, "camx", BOTH),
    # ---- volumes: LLI (lambertian + isotropic + an aligned quad light, solid textures, the persistent schedule), and the
    # general form without a light, under the wavefront schedule and with a noise texture
    ("smoke_thick", AUTO, PERSIST, None, LIN_LLI, "", BOTH),
    ("smoke_thin", AUTO, PERSIST, None, LIN_LLI, "", BOTH),
    ("smoke_thick", AUTO, PERSIST, "orthonormal", LIN_LLI, "camx", BOTH),
    ("smoke_nolight", AUTO, PERSIST, None, LIN_VOL, "", BOTH),
    ("smoke_thick", AUTO, STEP, None, LIN_VOL, "", BOTH),
    ("smoke_thin", AUTO, STEP, None, LIN_VOL, "", BOTH),
    ("smoke_nolight", AUTO, STEP, None, LIN_VOL, "", BOTH),
    ("smoke_value", AUTO, PERSIST, None, LIN_VOL, "camx", BOTH),
    ("smoke_nolight", AUTO, PERSIST, "lens", LIN_VOL, "camx", BOTH),
    ("smoke_value", AUTO, STEP, None, LIN_VOL, "camx", BOTH),
    # ---- the linear program with spheres: the rotate_x / y / z + translate chain about a glass box and a metal sphere,
    # the list of metal (fuzz 0, 0.5, 1) and glass spheres under a sphere light; with a volume, the program of all kinds
    ("chain", AUTO, PERSIST, None, LIN_SPH, "", BOTH),
    ("spheres_list", AUTO, PERSIST, None, LIN_SPH, "", BOTH),
    ("chain", AUTO, STEP, None, LIN_SPH, "", BOTH),
    ("spheres_list", AUTO, STEP, None, LIN_SPH, "", BOTH),
    ("chain_image", AUTO, PERSIST, None, LIN_SPH, "camx", BOTH),
    ("chain", AUTO, PERSIST, "lens", LIN_SPH, "camx", BOTH),
    ("spheres_list", AUTO, PERSIST, "fisheye", LIN_SPH, "camx", BOTH),
    ("chain_image", AUTO, STEP, None, LIN_SPH, "camx", BOTH),
    ("smoke_chain", AUTO, PERSIST, None, LIN_ALL, "", BOTH),
    ("smoke_ball", AUTO, PERSIST, None, LIN_ALL, "", BOTH),
    ("smoke_chain", AUTO, STEP, None, LIN_ALL, "", BOTH),
    ("smoke_ball", AUTO, STEP, None, LIN_ALL, "", BOTH),
    ("smoke_ball", AUTO, PERSIST, "lens", LIN_ALL, "camx", BOTH),
    ("smoke_chain", AUTO, STEP, "fisheye", LIN_ALL, "camx", BOTH),
    # ---- the wide tree (the persistent schedule, the perspective camera): in LDS, and in HBM past 4,096 primitive words
    ("spheres_nl", AUTO, PERSIST, None, W_SPH_NL, "", BOTH),
    ("spheres_nl_hbm", AUTO, PERSIST, None, W_SPH_NL_HBM, "", BOTH),
    ("spheres_light", AUTO, PERSIST, None, W_SPH, "", BOTH),
    ("spheres_small", AUTO, PERSIST, None, W_SPH, "", BOTH),
    ("spheres_light_hbm", AUTO, PERSIST, None, W_SPH_HBM, "", BOTH),
    ("mesh_tris", AUTO, PERSIST, None, W_TRI, "", BOTH),
    ("terrain", AUTO, PERSIST, None, W_TRI_HBM, "", BOTH),
    ("mesh", AUTO, PERSIST, None, W_TQ, "", BOTH),
    ("mesh_small", AUTO, PERSIST, None, W_TQ, "", BOTH),
    # (mesh_deep: the wide stack of its deep tree, 22 entries of every lane, is counted in the LDS budget. With fp32 words
    # nodes, primitives and stack are 30,336 bytes; with fp64 words 41,488, past the 40 KiB: the fp64 tree goes to HBM)
    ("mesh_deep", AUTO, PERSIST, None, W_TQ, "", (F32,)),
    ("mesh_deep", AUTO, PERSIST, None, W_TQ_HBM, "", (F64,)),
    ("terrain_ll", AUTO, PERSIST, None, W_TQ_LL_HBM, "", BOTH),
    ("mixed_static", AUTO, PERSIST, None, W_ALL, "", BOTH),
    ("mixed_static_hbm", AUTO, PERSIST, None, W_ALL_HBM, "", BOTH),
    # (moving spheres in fp64 only: the reference's normal of a moving sphere makes radiance ill-conditioned in fp32,
    # test_wide_mixed_primitives_match_oracle)
    ("mixed", AUTO, PERSIST, None, W_ALL, "", (F64,)),
    ("mixed_hbm", AUTO, PERSIST, None, W_ALL_HBM, "", (F64,)),
    # ---- the binary BVH: in reference order, under the wavefront schedule, and (extended) for another camera or a
    # picture or noise texture
    ("mesh", ORDERED, PERSIST, None, B_MID, "", BOTH),
    ("mesh_tris", ORDERED, PERSIST, None, B_MID, "", BOTH),
    ("mixed_static", ORDERED, PERSIST, None, B_SMALL, "", BOTH),
    ("mixed", ORDERED, PERSIST, None, B_SMALL, "", (F64,)),
    ("mesh", ORDERED, STEP, None, B_MID, "", BOTH),
    ("mesh_small", AUTO, STEP, None, B_MID, "", BOTH),
    ("mesh", AUTO, PERSIST, "fisheye", B_MID, "camx", BOTH),
    ("mesh_tris", AUTO, PERSIST, "fisheye", B_MID, "camx", BOTH),
    ("mixed_static", AUTO, PERSIST, "fisheye", B_SMALL, "camx", BOTH),
    ("mesh_image", AUTO, PERSIST, None, B_MID, "camx", BOTH),
    ("mesh_perlin", AUTO, STEP, None, B_MID, "camx", BOTH),
    ("mesh", ORDERED, STEP, "fisheye", B_MID, "camx", BOTH),
    ("spheres_small", ORDERED, PERSIST, None, B_SMALL, "", BOTH),
    ("spheres_small", ORDERED, STEP, None, B_SMALL, "", BOTH),
    ("spheres_small", AUTO, PERSIST, "fisheye", B_SMALL, "camx", BOTH),
    ("spheres_small", AUTO, STEP, "fisheye", B_SMALL, "camx", BOTH),
    ("spheres_nl_hbm", ORDERED, PERSIST, None, B_LARGE, "", BOTH),
    ("spheres_nl_hbm", ORDERED, STEP, None, B_LARGE, "", BOTH),
    ("spheres_nl_hbm", AUTO, PERSIST, "fisheye", B_LARGE, "camx", BOTH),
    ("spheres_nl_hbm", AUTO, STEP, "fisheye", B_LARGE, "camx", BOTH),
    ("mesh_deep", ORDERED, PERSIST, None, B_DEEP, "", BOTH),
    ("mesh_deep", ORDERED, STEP, None, B_DEEP, "", BOTH),
    ("mesh_deep", AUTO, PERSIST, "fisheye", B_DEEP, "camx", BOTH),
    ("mesh_deep", AUTO, STEP, "fisheye", B_DEEP, "camx", BOTH),
]
# ---- the rows that carry every branch into every form: the miss paths ("scene@none": no background, "@black": a solid
# black one, "@checker": a checker on miss's unit sphere), a light that emits through a checker, a light seen from
# behind, an instance and a volume under a bvh_node
ROWS += [(name, AUTO, PERSIST, None, FLAT_LL, "", BOTH) for name in ("backlight@none", "backlight@black")]
ROWS += [(name, AUTO, STEP, None, FLAT_GLOBAL, "", BOTH)
         for name in ("dark", "nobg", "nolight_checker", "checker_light", "backlight_metal")]
ROWS += [(name, ORDERED, STEP, None, LIN_QUAD, "", BOTH)
         for name in ("glass", "gloss", "nolight", "nolight_checker", "dark", "nobg", "checker_light")]
CAMX_ROOMS = [("glass@checker", "fisheye"), ("glass@none", "lens"), ("glass@black", "orthonormal"),
              ("checker_light", "fisheye")]
ROWS += [(name, AUTO, sched, cam, LIN_QUAD, "camx", BOTH) for name, cam in CAMX_ROOMS for sched in (PERSIST, STEP)]
ROWS += [(name, AUTO, STEP, cam, LIN_QUAD, "camx", BOTH)
         for name, cam in (("metal", "lens"), ("glass", "orthonormal"), ("nolight", "fisheye"), ("gloss_value", None),
                           ("glass_worley", None))]
ROWS += [("smoke_nolight", AUTO, STEP, "lens", LIN_VOL, "camx", BOTH)]
ROWS += [(name, AUTO, PERSIST, cam, LIN_LLI, "camx" if cam else "", BOTH)
         for name in ("smoke_thick@none", "smoke_thick@black") for cam in (None, "orthonormal")]
ROWS += [(name, AUTO, PERSIST, None, W_TQ, "", BOTH)
         for name in ("mesh@none", "mesh@black", "mesh@checker", "mesh_checker_light")]
ROWS += [(name, AUTO, PERSIST, None, W_TQ_LL, "", BOTH) for name in ("mesh_ll", "mesh_ll@none", "mesh_ll@black")]
ROWS += [(name, AUTO, PERSIST, None, W_SPH_NL, "", BOTH) for name in ("spheres_nl_small", "spheres_nl_small@checker")]
# the binary BVH's four forms (reference order or, for another camera, the default path; either schedule)
BVH_FORMS = [(ORDERED, PERSIST, None, ""), (ORDERED, STEP, None, ""), (AUTO, PERSIST, "fisheye", "camx"),
             (AUTO, STEP, "fisheye", "camx")]
HAVE = {r[:4] for r in ROWS}
ROWS += [(name, trav, sched, cam, tag, camx, BOTH)
         for name, tag in (("mesh", B_MID), ("mesh_tris", B_MID), ("mixed_static", B_SMALL), ("mesh@none", B_MID),
                           ("mesh@black", B_MID), ("mesh@checker", B_MID), ("mesh_checker_light", B_MID),
                           ("mesh_extras", B_MID), ("mesh_tris_extras", B_MID))
         for trav, sched, cam, camx in BVH_FORMS if (name, trav, sched, cam) not in HAVE]
ROWS += [("instanced", AUTO, sched, cam, B_INST, camx, BOTH)
         for sched, cam, camx in ((PERSIST, None, ""), (STEP, None, ""), (PERSIST, "fisheye", "camx"), (STEP, "fisheye", "camx"))]
ROWS += [("mesh_image", AUTO, STEP, None, B_MID, "camx", BOTH), ("mesh_perlin", AUTO, PERSIST, None, B_MID, "camx", BOTH)]


def tag_of(trav, camx, sched, prec):
    t = (trav[prec] if isinstance(trav, dict) else trav).format(p=P[prec])
    return t + (" camx" if camx else "") + (" step" if sched else " persist")


# rows (scene, precision, traversal, segments_per_launch, camera or None, tag)
TABLE = [(name, prec, trav, sched, cam, tag_of(t, camx, sched, prec))
         for name, trav, sched, cam, t, camx, precs in ROWS for prec in precs]


def row_id(r):
    return (f"{r[0]}{'-' + r[4] if r[4] else ''}-{P[r[1]]}-{'ordered' if r[2] == ORDERED else 'auto'}-"
            f"{'step' if r[3] else 'persist'}")


# ------------------------------------------------------------------ the coverage the table is held to
# tags no row of either table launches, each with its reason
LEFT_OUT = {}  # none: every tag is launched

# The events (oracle.h ORC_EV_*) of the branches shade compiles into each form; every form must be seen with each of
# its events, in fp32 and in fp64.
SCATTER = {"emit_front", "emit_back", "lamb_light_half", "lamb_cosine_half", "lamb_no_light", "metal_mirror",
           "metal_fuzz", "metal_below", "diel_cant", "diel_schlick", "diel_refract_front", "diel_refract_back",
           "gloss_specular", "gloss_diffuse", "tex_solid"}
MISSES = {"miss_none", "miss_black", "miss_solid", "miss_textured", "tex_checker"}
GENERAL = SCATTER | MISSES  # the general shade program: every material but isotropic, emission, every miss path
ISO = {"iso_light", "iso_no_light", "instance"}  # volumes and instances: the linear program and the binary BVH
EXT_TEX = {"tex_image", "tex_perlin", "tex_value", "tex_worley"}
LL = {"lamb_light_half", "lamb_cosine_half", "emit_front", "emit_back", "miss_none", "miss_black", "miss_solid"}
NL = {"lamb_no_light", "metal_mirror", "metal_fuzz", "metal_below", "diel_cant", "diel_schlick", "diel_refract_front",
      "diel_refract_back", "miss_solid", "miss_textured", "tex_solid", "tex_checker"}
REQUIRED = {
    "flat general": GENERAL | {"instance"},
    "flat general step": GENERAL | {"instance"},
    "flat LL": LL,
    "linear": GENERAL | ISO,
    "linear step": GENERAL | ISO,
    "linear camx": GENERAL | ISO | EXT_TEX | {"miss_short"},
    "linear camx step": GENERAL | ISO | EXT_TEX | {"miss_short"},
    "linear LLI": LL | {"iso_light"},
    "linear LLI camx": LL | {"iso_light"},
    "stack": GENERAL | ISO,
    "stack step": GENERAL | ISO,
    "stack camx": GENERAL | ISO | {"tex_image", "tex_perlin"},
    "stack camx step": GENERAL | ISO | {"tex_image", "tex_perlin"},
    "wide general": GENERAL,
    "wide NL": NL,
    "wide LL": LL,
}
# a hit on a moving sphere: fp64 only (see the rows)
REQUIRED_F64 = {"wide general": {"moving_sphere", "miss_short"}, "stack": {"moving_sphere"}}
# what REQUIRED leaves out of a form that compiles the branch in, and why
EVENTS_LEFT_OUT = {
    ("wide NL", "miss_none, miss_black"):
        "NL is a scene without a light: with no background or a black one every path returns 0, the frame is black and "
        "a row would compare zeros (every scene here is lit)",
    ("flat LL, wide LL, linear LLI", "miss_textured, tex_checker and the other texture kinds"):
        "rt_plan.h lamb_light_scene / lamb_iso_light_scene select these forms for solid textures only, the background's "
        "included: with any other texture the scene takes the general form",
    ("flat", "iso_light, iso_no_light"): "a volume ends the flat program (scene_compile.cpp flat_program)",
    ("wide", "instance, iso_light, iso_no_light"):
        "the wide tree holds world-level spheres, triangles and quads only (scene_compile.cpp: prims_only)",
    ("stack camx", "tex_value, tex_worley"):
        "tex_sample<R, true> is one function for every extended kernel; the linear camx rows run these two kinds",
    ("every form but linear camx and wide general (fp64)", "miss_short"):
        "it needs a direction longer than 1000: the lens camera's, or a reflection off a moving sphere's long normal",
    ("every form but wide general and stack in fp64", "moving_sphere"):
        "the reference's normal of a moving sphere is (p - 0) / radius, not a unit vector (sphere.h:69): radiance is "
        "ill-conditioned in fp32 (test_wide_mixed_primitives_match_oracle), so no fp32 row has one; a hit on one differs "
        "from a static sphere's in the traversal's centre at the ray's time alone, not in shade, so fp64 has it once "
        "per BVH traversal (the wide tree and the binary one) and test_gpu_lights.py's sphere/moving row in the linear "
        "program; the step and camx forms share those traversals",
}


def shade_form(tag):
    """The shade program a tag names: the family, its LL / LLI / NL argument, the extended form, the schedule."""
    trav, _, rest = tag.partition(" ")
    name, args = trav.rstrip(">").split("<")
    a = args.split(",")[1:]
    if name == "FlatTrav":
        form = "flat LL" if a[1] == "1" else "flat general"
    elif name == "LinearTrav":
        form = "linear LLI" if a[3] == "1" else "linear"
    elif name == "StackTrav":
        form = "stack"
    else:
        form = "wide NL" if a[6] == "1" else "wide LL" if a[5] == "1" else "wide general"
    return form + (" camx" if "camx" in rest else "") + (" step" if rest.endswith("step") else "")


def test_table_covers_every_branch_and_form():
    assert len({r[:5] for r in TABLE}) == len(TABLE)  # no row twice
    for r in TABLE:
        assert (r[0], r[4] or "perspective") in cpu.EVENTS, r  # the CPU test counted this scene under this camera
    seen = {}
    for name, prec, _, _, cam, tag in TABLE:
        seen.setdefault((shade_form(tag), prec), set()).update(cpu.EVENTS[(name, cam or "perspective")])
    assert {f for f, _ in seen} == set(REQUIRED), {f for f, _ in seen} ^ set(REQUIRED)
    for form, events in REQUIRED.items():
        for prec in BOTH:
            want = events | (REQUIRED_F64.get(form, set()) if prec == F64 else set())
            assert want <= seen[(form, prec)], (form, P[prec], sorted(want - seen[(form, prec)]))
    # every scene of the module is rendered, in both precisions but for the two with moving spheres
    for name in S.SCENES:
        precs = {r[1] for r in TABLE if r[0].partition("@")[0] == name}
        assert precs == ({F64} if name in ("mixed", "mixed_hbm") else {F32, F64}), name
    # the tags: with the lights table's, every tag the launch functions can select but the ones left out
    ours, theirs = {r[5] for r in TABLE}, {r[4] for r in lights.TABLE}
    every = all_tags()
    assert len(every) == 96 and ours <= every and theirs <= every and set(LEFT_OUT) <= every
    assert (ours | theirs) == every - set(LEFT_OUT), sorted(every - set(LEFT_OUT) - ours - theirs)
    # EVENTS_LEFT_OUT speaks of real events, and of none that REQUIRED asks of every form
    named = {e for _, evs in EVENTS_LEFT_OUT for e in re.findall(r"[a-z]+_[a-z_0-9]+", evs)}
    assert named <= set(oracle.EVENTS), named - set(oracle.EVENTS)
    assert not named & set.intersection(*REQUIRED.values()), named & set.intersection(*REQUIRED.values())
    assert not (ours | theirs) & set(LEFT_OUT)


# ------------------------------------------------------------------ renders
@pytest.fixture(scope="module")
def ctx():
    c = rt_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """(scene, camera) -> (desc, cam, oracle frame, oracle segments): rendered once, never changed."""
    cache = {}

    def get(name, cam_kind):
        key = (name, cam_kind or "perspective")
        if key not in cache:
            desc, cam = S.build(name, key[1])
            ref, segs = oracle.render(oracle.from_desc(desc), cam, SPP, DEPTH, seed=SEED, threads=8)
            ref.setflags(write=False)
            cache[key] = (desc, cam, ref, segs)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def measured():
    """What the rows measured, printed once at the end (DESIGN.md section 6 quotes the maxima)."""
    m = {}
    yield m
    for group, vals in sorted(m.items()):
        print(f"[materials] {group}: " + ", ".join(f"{k} max {max(v):.3g}" for k, v in sorted(vals.items())))


SPECULAR = {"metal_mirror", "metal_fuzz", "metal_below", "diel_cant", "diel_schlick", "diel_refract_front",
            "diel_refract_back", "gloss_specular"}


@pytest.mark.parametrize("row", TABLE, ids=row_id)
def test_material_matches_the_oracle(ctx, refs, measured, row):
    name, prec, trav, sched, cam_kind, tag = row
    desc, cam, ref, segs = refs(name, cam_kind)
    ctx.upload(desc)
    ctx.reset_counters()
    img = ctx.render(cam, SPP, DEPTH, seed=SEED, precision=prec, traversal=trav, segments_per_launch=sched)
    assert ctx.last_kernel() == tag
    events = cpu.EVENTS[(name, cam_kind or "perspective")]
    check_against_oracle(name, prec, img, ref, measured, row_id(row), bvh=name.partition("@")[0] in S.BVH_SCENES,
                         specular=bool(SPECULAR & set(events)), group=shade_form(tag).split(" ")[0])
    if prec == F64:
        # traced segments: the device stops a path whose throughput is exactly 0, the reference keeps recursing; without
        # light sampling nothing stops early
        st = ctx.stats()
        assert 0 < st.segments <= segs, (st.segments, segs)
        if desc.light < 0:
            assert st.segments == segs, (st.segments, segs)
