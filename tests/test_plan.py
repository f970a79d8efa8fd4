"""The host's render plan (csrc/rt_plan.h: pure C++, no HIP): the item layout and its passes, div_magic, the kernel
family a render takes and the path kernel within it. tests/native/plan_dump.cpp answers one question per input line; the
invariants, the pinned BASELINE layouts, the family table and every limit of the kernel choice are checked here."""
import os
import random
import subprocess

import pytest

import kernel_tags as T
from rt_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "csrc")
BUDGET = 2 << 30  # PlanKnobs::partial_budget
FLAT, LIN_QUAD, LIN_VOL, LIN_SPH, LIN_ALL, WIDE, STACK = range(7)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(REPO, "tests", "native", "plan_dump.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True,
                             text=True).stdout.split("\n")
        assert len(out) == len(lines) + 1 and out[-1] == ""
        return out[:-1]
    return run


def plans(ask, tuples):
    """tuples of (spp, samples_per_item, flat, full_pixels, npix, elem, budget or 0) -> dicts of the plan"""
    keys = ("chunk", "tail_chunk", "k_bulk", "nchunks", "cpp", "passes", "partial_bytes")
    out = ask(["P " + " ".join(str(int(v)) for v in t) for t in tuples])
    return [dict(zip(keys, (int(v) for v in ln.split()))) for ln in out]


def sweep():
    rng = random.Random(20260)
    ts = []
    for _ in range(3000):
        spp = rng.choice([1, 2, 3, rng.randint(1, 16), rng.randint(1, 300), rng.randint(1, 5000)])
        spi = rng.choice([0, 0, 0, 1, rng.randint(1, 2 * spp + 1)])  # 0: automatic; also samples_per_item > spp
        npix = min((1 << 31) - 1, int(2 ** rng.uniform(0, 31)))
        full = npix * rng.randint(1, 8)
        budget = rng.choice([0, 0, 1, int(2 ** rng.uniform(10, 36))])  # 1: the smallest (one chunk per pass)
        ts.append((spp, spi, rng.randint(0, 1), full, npix, rng.choice([4, 8]), budget))
    # spp below the automatic tail chunk, one pixel, the largest call
    ts += [(3, 0, 1, 16, 16, 4, 0), (1, 0, 0, 1, 1, 8, 1), (4096, 0, 0, (1 << 31) - 1, (1 << 31) - 1, 8, 0)]
    return ts


def test_item_plan_invariants(ask):
    ts = sweep()
    for t, p in zip(ts, plans(ask, ts)):
        spp, spi, flat, full, npix, elem, budget = t
        budget = budget or BUDGET
        # bulk items, then tail items, cover [0, spp) exactly once and in order (the kernels' item_range)
        at = 0
        for c in range(p["nchunks"]):
            bulk = c < p["k_bulk"]
            first = c * p["chunk"] if bulk else p["k_bulk"] * p["chunk"] + (c - p["k_bulk"]) * p["tail_chunk"]
            assert first == at and first < spp, (t, p, c)
            at = min(first + (p["chunk"] if bulk else p["tail_chunk"]), spp)
        assert at == spp, (t, p)
        assert 1 <= p["tail_chunk"] <= p["chunk"], (t, p)
        if spi <= 0:
            assert p["nchunks"] <= 256 or p["chunk"] >= spp, (t, p)
        else:
            assert p["chunk"] == p["tail_chunk"] == min(spi, spp), (t, p)
        assert p["cpp"] >= 1 and npix * p["cpp"] < 1 << 31, (t, p)
        assert p["passes"] * p["cpp"] >= p["nchunks"] > (p["passes"] - 1) * p["cpp"], (t, p)
        assert p["partial_bytes"] == 3 * elem * npix * p["cpp"] <= max(budget, 3 * elem * npix), (t, p)


def test_items_of_a_pass_stay_below_2_31(ask):
    # 64 uniform items per pixel, a budget that never binds: pixels x chunks at 2^31 - 64 and at 2^31
    lo, hi = plans(ask, [(64, 1, 0, 1 << 25, (1 << 25) - 1, 4, 1 << 40), (64, 1, 0, 1 << 25, 1 << 25, 4, 1 << 40)])
    assert (lo["nchunks"], lo["cpp"], lo["passes"]) == (64, 64, 1)
    assert (hi["nchunks"], hi["cpp"], hi["passes"]) == (64, 63, 2)


def test_div_magic(ask):
    rng = random.Random(7)
    top = (1 << 31) - 1
    q = []
    for d in (1, 2, 3, 7, 640000, 8294400, top):
        ns = {0, 1, top, top - 1, d - 1, d, d + 1, top // d * d, max(0, top // d * d - 1)}
        ns |= {rng.randint(0, top) for _ in range(400)} | {rng.randint(0, top // d) * d for _ in range(50)}
        q += [(d, n) for n in sorted(ns) if 0 <= n <= top]
    got = ask([f"D {d} {n}" for d, n in q])
    assert [int(g) for g in got] == [n // d for d, n in q]


def test_baseline_layouts(ask):
    # default knobs; (spp, samples_per_item, flat, full image, pixels of the call, element size)
    c1 = [(64, 0, 1, 400 * 400, 400 * 400, e, 0) for e in (4, 8)]
    c2 = [(1024, 0, 1, 800 * 800, 800 * 800, e, 0) for e in (4, 8)]
    c5 = [(4096, 0, 0, 3840 * 2160, 3840 * 2160, 8, 0)]
    explicit = [(2100, 1, 0, 1024 * 1024, 1024 * 1024, 4, 0)]
    ps = plans(ask, c1 + c2 + c5 + explicit)

    def layout(p):
        return p["chunk"], p["tail_chunk"], p["k_bulk"], p["nchunks"]
    for p in ps[0:2]:
        assert layout(p) == (2, 2, 28, 32) and p["passes"] == 1, p
    for p in ps[2:4]:
        assert layout(p) == (32, 8, 28, 44) and p["passes"] == 1, p
    assert layout(ps[4]) == (32, 16, 64, 192) and (ps[4]["cpp"], ps[4]["passes"]) == (10, 20), ps[4]
    assert layout(ps[5]) == (1, 1, 2100, 2100), ps[5]
    assert (ps[5]["cpp"], ps[5]["passes"], ps[5]["partial_bytes"]) == (170, 13, 2139095040), ps[5]


def test_kernel_family_table(ask):
    # header fields: has_flat, n_linear, n_spheres, n_tris, has_volumes, has_wide; then the family on the scene's
    # fast path and the one it falls back to
    kinds = {
        "cornell (C1, C2)": ((1, 14, 0, 0, 0, 0), FLAT, LIN_QUAD),
        "cornell + volumes (C5)": ((0, 16, 0, 0, 1, 0), LIN_VOL, LIN_VOL),
        "a few spheres": ((0, 4, 4, 0, 0, 0), LIN_SPH, LIN_SPH),
        "rtow (C3)": ((0, 0, 485, 0, 0, 1), WIDE, STACK),
        "mesh + quad light (C4)": ((0, 0, 0, 50000, 0, 1), WIDE, STACK),
    }
    cases, want = [], []
    for name, (hdr, fast, slow) in kinds.items():
        for cam in (abi.RT_CAM_PERSPECTIVE, abi.RT_CAM_FISHEYE):
            for persist in (1, 0):
                for ordered in (0, 1):
                    for texdata, cell in ((0, 0), (256, 0), (0, 1)):
                        ok = cam == abi.RT_CAM_PERSPECTIVE and not ordered and not texdata and not cell
                        if fast == WIDE:
                            ok = ok and persist
                        cases.append((name, hdr + (texdata, cell, cam, persist, ordered)))
                        want.append(fast if ok else slow)
    got = ask(["F " + " ".join(str(v) for v in c) for _, c in cases])
    names = ["flat program", "linear program (quads)", "linear program (quads + volumes)", "linear program (spheres)",
             "linear program (all kinds)", "wide BVH", "binary BVH"]
    for (name, c), w, g in zip(cases, want, got):
        assert g == f"{w} {names[w]}", (name, c, g)
    # spheres and triangles in one linear program: the program for every kind
    assert ask(["F 0 9 2 3 0 0 0 0 0 1 0"]) == [f"{LIN_ALL} {names[LIN_ALL]}"]


# ------------------------------------------------------------------ the path kernel (rt_plan.h path_kernel)
# The K line's arguments in order, with the values of a scene that reaches no limit. n_flat_quad is the three axes' sum.
K_FIELDS = ("has_flat", "n_linear", "n_spheres", "n_tris", "has_volumes", "has_wide", "n_texdata", "has_cell_noise",
            "n_flat_quad", "n_flat_box", "n_flat_room", "n_mats", "n_nodes", "n_wnodes", "n_wprim_words", "wide_stack",
            "wide_kinds", "mat_kinds", "tex_kinds", "light_kind", "light_aligned", "word_bytes", "cam_mode", "persist",
            "ordered", "stack_need")
K_DEFAULT = dict.fromkeys(K_FIELDS, 0)
K_DEFAULT.update(n_mats=4, n_nodes=100, stack_need=8, word_bytes=16, cam_mode=abi.RT_CAM_PERSPECTIVE, persist=1)
# scene classes (rt_scene.h M_*, T_*, L_* as bits and kinds; rt_plan.h lamb_light_scene, no_light_scene,
# lamb_iso_light_scene): the general one has a metal and a checker under an aligned quad light
M = {k: 1 << v for k, v in dict(lamb=abi.RT_MAT_LAMBERTIAN, metal=abi.RT_MAT_METAL, diel=abi.RT_MAT_DIELECTRIC,
                                iso=abi.RT_MAT_ISOTROPIC, light=abi.RT_MAT_DIFFUSE_LIGHT).items()}
SOLID, CHECKER = 1 << abi.RT_TEX_SOLID, 1 << abi.RT_TEX_CHECKER
L_NONE, L_QUAD = 0, 2
GENERAL = dict(mat_kinds=M["lamb"] | M["metal"] | M["light"], tex_kinds=SOLID | CHECKER, light_kind=L_QUAD, light_aligned=1)
LL = dict(mat_kinds=M["lamb"] | M["light"], tex_kinds=SOLID, light_kind=L_QUAD, light_aligned=3)
NL = dict(mat_kinds=M["lamb"] | M["metal"] | M["diel"], tex_kinds=SOLID | CHECKER, light_kind=L_NONE, light_aligned=0)
LLI = dict(mat_kinds=M["lamb"] | M["light"] | M["iso"], tex_kinds=SOLID, light_kind=L_QUAD, light_aligned=1)
# the programs a compiled scene can have
H_FLAT = dict(has_flat=1, n_linear=14, n_flat_quad=12)
H_QUADS = dict(n_linear=14)
H_VOLS = dict(n_linear=16, has_volumes=1)
H_SPHERES = dict(n_linear=4, n_spheres=4)
H_ALL_KINDS = dict(n_linear=9, n_spheres=2, n_tris=3)
H_WIDE = dict(has_wide=1, n_spheres=50, n_wnodes=10, n_wprim_words=100, wide_stack=8, wide_kinds=1)
H_BVH = dict(n_spheres=50)
PREC = {16: "f32", 32: "f64"}  # word_bytes -> the tag's precision


def tags(ask, cases):
    """dicts of K fields (K_DEFAULT for the rest) -> the tags"""
    return ask(["K " + " ".join(str(int({**K_DEFAULT, **c}[f])) for f in K_FIELDS) for c in cases])


def expect(ask, pairs):
    """[(dict of K fields, tag with "{p}" for the precision)]: asked at both word sizes"""
    cases = [({**c, "word_bytes": wb}, t.format(p=p)) for c, t in pairs for wb, p in PREC.items()]
    for (c, want), got in zip(cases, tags(ask, [c for c, _ in cases])):
        assert got == want, (c, got, want)


def test_path_kernel_flat_table_limits(ask):
    pairs = []
    # the general form's tables: 64 quads, 16 boxes, 2 rooms, 32 materials; one more and the records stay in global memory
    for field, cap in (("n_flat_quad", 64), ("n_flat_box", 16), ("n_flat_room", 2), ("n_mats", 32)):
        pairs += [({**H_FLAT, **GENERAL, field: cap}, T.FLAT_LDS + " persist"),
                  ({**H_FLAT, **GENERAL, field: cap + 1}, T.FLAT_GLOBAL + " persist"),
                  ({**H_FLAT, **LL, field: cap + 1}, T.FLAT_GLOBAL + " persist")]
    # the LL form's: 14 quads, 8 boxes, 1 room, 16 materials; a scene over one of them, within the general ones, takes
    # the general form in LDS, as does a scene within them that is not lambertian + light
    for field, cap in (("n_flat_quad", 14), ("n_flat_box", 8), ("n_flat_room", 1), ("n_mats", 16)):
        pairs += [({**H_FLAT, **LL, field: cap}, T.FLAT_LL + " persist"),
                  ({**H_FLAT, **LL, field: cap + 1}, T.FLAT_LDS + " persist"),
                  ({**H_FLAT, **GENERAL, field: cap}, T.FLAT_LDS + " persist")]
    # all four at their limit at once
    pairs += [({**H_FLAT, **GENERAL, "n_flat_quad": 64, "n_flat_box": 16, "n_flat_room": 2, "n_mats": 32}, T.FLAT_LDS + " persist"),
              ({**H_FLAT, **LL, "n_flat_quad": 14, "n_flat_box": 8, "n_flat_room": 1, "n_mats": 16}, T.FLAT_LL + " persist")]
    # an LL scene with a light off the axes, or a checker, is a general one
    pairs += [({**H_FLAT, **LL, "light_aligned": 0}, T.FLAT_LDS + " persist"),
              ({**H_FLAT, **LL, "tex_kinds": SOLID | CHECKER}, T.FLAT_LDS + " persist")]
    # the wavefront schedule reads the records in global memory
    pairs += [({**H_FLAT, **cls, "persist": 0}, T.FLAT_GLOBAL + " step") for cls in (GENERAL, LL)]
    expect(ask, pairs)


def test_path_kernel_lli_limits(ask):
    lli, vol = T.LIN_LLI, T.LIN_VOL
    expect(ask, [
        ({**H_VOLS, **LLI, "n_mats": 16}, lli + " persist"),
        ({**H_VOLS, **LLI, "n_mats": 17}, vol + " persist"),
        ({**H_VOLS, **LLI, "n_mats": 16, "persist": 0}, vol + " step"),  # step_body shades with the general program
        ({**H_VOLS, **LL, "n_mats": 16}, lli + " persist"),              # (no isotropic material: still the class)
        ({**H_VOLS, **GENERAL, "n_mats": 16}, vol + " persist"),
        ({**H_VOLS, **NL, "n_mats": 16}, vol + " persist"),
        ({**H_VOLS, **LLI, "light_aligned": 0}, vol + " persist"),
        ({**H_VOLS, **LLI, "n_mats": 16, "cam_mode": abi.RT_CAM_LENS}, lli + " camx persist"),
        ({**H_VOLS, **LLI, "n_mats": 17, "cam_mode": abi.RT_CAM_LENS}, vol + " camx persist"),
        # the class concerns the volume program alone
        ({**H_QUADS, **LLI}, T.LIN_QUAD + " persist"), ({**H_SPHERES, **LLI}, T.LIN_SPH + " persist"),
        ({**H_ALL_KINDS, **LLI, "has_volumes": 1}, T.LIN_ALL + " persist"),
    ])


def test_path_kernel_binary_bvh_limits(ask):
    def bvh(nodes, need, wb):
        return {**H_BVH, **GENERAL, "n_nodes": nodes, "stack_need": need, "word_bytes": wb}
    # fp32: the nodes in LDS up to 256 of them when the stack needs at most 16 entries (the kernel has 16)
    f32 = [(256, 1, "16,1"), (256, 8, "16,1"), (256, 16, "16,1"), (257, 16, "16,0"), (256, 17, "32,0"), (257, 17, "32,0"),
           (1, 16, "16,1"), (1, 17, "32,0"), (257, 8, "8,0"), (257, 9, "16,0"), (257, 32, "32,0")]
    # fp64: never; either precision: 8, 16 or kStackDepth = 32 entries by the need
    f64 = [(n, need, f"{8 if need <= 8 else 16 if need <= 16 else 32},0")
           for n in (1, 256, 257, 5000) for need in (1, 8, 9, 16, 17, 32)]
    for wb, rows in ((16, f32), (32, f64)):
        for sched, persist in ((" persist", 1), (" step", 0)):
            got = tags(ask, [{**bvh(n, need, wb), "persist": persist} for n, need, _ in rows])
            assert got == [f"StackTrav<{PREC[wb]},{a}>{sched}" for _, _, a in rows], (wb, sched, got)


def test_path_kernel_wide_kinds_and_classes(ask):
    # WK_SPHERE 1, WK_TRI 2, WK_QUAD 4, WK_MOVING 8: spheres alone, triangles alone and triangles + quads have kernels
    # of their own, every other combination takes the kernel of all kinds
    sets = {1: "1,0,0,0", 2: "0,1,0,0", 6: "0,1,1,0"}
    pairs = []
    for kinds in range(1, 16):
        k = sets.get(kinds, "1,1,1,1")
        for cls, name in ((GENERAL, "general"), (NL, "NL"), (LL, "LL"), (LLI, "LLI")):
            ll = int(name == "LL" and kinds == 6)  # LL: triangles + quads alone
            nl = int(name == "NL" and kinds == 1)  # NL: spheres alone
            pairs.append(({**H_WIDE, **cls, "wide_kinds": kinds}, f"WideTrav<{{p}},{k},1,{ll},{nl}> persist"))
    assert len({t for _, t in pairs}) == 6  # the six kind sets, each tree in LDS here
    # LL: at most 16 materials
    pairs += [({**H_WIDE, **LL, "wide_kinds": 6, "n_mats": 16}, T.W_TQ_LL + " persist"),
              ({**H_WIDE, **LL, "wide_kinds": 6, "n_mats": 17}, T.W_TQ + " persist"),
              ({**H_WIDE, **NL, "wide_kinds": 1, "n_mats": 17}, T.W_SPH_NL + " persist")]  # (NL has no table)
    expect(ask, pairs)


def test_path_kernel_wide_tree_in_lds(ask):
    # rt_plan.h wide_tree_in_lds: nodes at 144 bytes, the primitive words and every stack entry of 256 lanes as uint16
    # within 40 KiB; node offsets (index x 9) below 2^15; at most 2^12 words
    budget = 40 << 10

    def fits(nodes, words, stack, wb):
        return nodes * 144 + words * wb + stack * 256 * 2 <= budget and nodes * 9 < 0x8000 and words <= 0x1000
    cases = []
    for wb in (16, 32):
        # the budget, from both sides, by each of its three terms: the last word, node and stack entry that fit
        for nodes, stack in ((0, 0), (1, 8), (10, 22), (100, 8)):
            w = (budget - nodes * 144 - stack * 512) // wb
            cases += [(nodes, w, stack, wb), (nodes, w + 1, stack, wb)]
        for words, stack in ((16, 8), (1000, 1)):
            n = (budget - words * wb - stack * 512) // 144
            cases += [(n, words, stack, wb), (n + 1, words, stack, wb)]
        for nodes, words in ((10, 16), (100, 500)):
            st = (budget - nodes * 144 - words * wb) // 512
            cases += [(nodes, words, st, wb), (nodes, words, st + 1, wb)]
        # The two code limits lie past the budget at either word size (2^15 / 9 = 3,641 nodes are 524 KB, 2^12 + 1
        # words 65 KB or more), so only the budget can be met from both sides; their far sides are asked all the same.
        assert [fits(*c) for c in cases[-16:]] == [True, False] * 8
        far = [(3640, 0, 0, wb), (3641, 0, 0, wb), (0, 0x1000, 0, wb), (0, 0x1001, 0, wb)]
        assert not any(fits(*c) for c in far)
        cases += far
    want = [fits(*c) for c in cases]
    for kinds, cls, lds, hbm in ((1, NL, T.W_SPH_NL, T.W_SPH_NL_HBM), (6, LL, T.W_TQ_LL, T.W_TQ_LL_HBM),
                                 (15, GENERAL, T.W_ALL, T.W_ALL_HBM)):
        got = tags(ask, [{**H_WIDE, **cls, "wide_kinds": kinds, "n_wnodes": n, "n_wprim_words": w, "wide_stack": s,
                          "word_bytes": wb} for n, w, s, wb in cases])
        for c, fit, g in zip(cases, want, got):
            assert g == (lds if fit else hbm).format(p=PREC[c[3]]) + " persist", (c, fit, g)


def test_path_kernel_extended_form(ask):
    ext = [dict(cam_mode=abi.RT_CAM_ORTHONORMAL), dict(cam_mode=abi.RT_CAM_FISHEYE), dict(cam_mode=abi.RT_CAM_LENS),
           dict(n_texdata=256), dict(has_cell_noise=1)]
    pairs = []
    for sched, persist in ((" persist", 1), (" step", 0)):
        for e in ext:
            e = {**e, **GENERAL, "persist": persist}
            pairs += [({**H_QUADS, **e}, T.LIN_QUAD + " camx" + sched), ({**H_VOLS, **e}, T.LIN_VOL + " camx" + sched),
                      ({**H_SPHERES, **e}, T.LIN_SPH + " camx" + sched), ({**H_ALL_KINDS, **e}, T.LIN_ALL + " camx" + sched),
                      # the flat program and the wide tree have no extended form: the render leaves them
                      ({**H_FLAT, **e}, T.LIN_QUAD + " camx" + sched),
                      ({**H_BVH, **e, "n_nodes": 300}, "StackTrav<{p},8,0> camx" + sched),
                      ({**H_WIDE, **e, "n_nodes": 300}, "StackTrav<{p},8,0> camx" + sched)]
        base = {**GENERAL, "persist": persist}
        pairs += [({**H_QUADS, **base}, T.LIN_QUAD + sched), ({**H_BVH, **base, "n_nodes": 300}, "StackTrav<{p},8,0>" + sched)]
    expect(ask, pairs)


def test_path_kernel_sweep_reaches_every_kernel_and_no_other(ask):
    # every program x class x limit side x camera x schedule x order x precision: the tags are kernel_tags.all_tags(), the
    # instantiations launch_step lists, and a family never comes in a form it does not have
    cases = []
    for prog in (H_FLAT, H_QUADS, H_VOLS, H_SPHERES, H_ALL_KINDS, H_WIDE, H_BVH):
        for cls in (GENERAL, LL, NL, LLI):
            for kinds in (1, 2, 6, 15):
                for words, mats, quads, nodes in ((100, 4, 12, 100), (5000, 4, 12, 300), (100, 40, 12, 100), (100, 4, 70, 300)):
                    for need in (8, 12, 20):
                        for cam in (abi.RT_CAM_PERSPECTIVE, abi.RT_CAM_FISHEYE):
                            cases += [{**prog, **cls, "wide_kinds": kinds, "n_wprim_words": words, "n_mats": mats,
                                       "n_flat_quad": quads, "n_nodes": nodes, "stack_need": need, "cam_mode": cam,
                                       "persist": persist, "ordered": ordered, "word_bytes": wb}
                                      for persist in (1, 0) for ordered in (0, 1) for wb in (16, 32)]
    got = tags(ask, cases)
    assert set(got) == T.all_tags() and len(T.all_tags()) == 96, sorted(set(got) ^ T.all_tags())
    for c, g in zip(cases, got):
        if g.startswith(("FlatTrav", "WideTrav")):
            assert "camx" not in g and not c["ordered"] and c["cam_mode"] == abi.RT_CAM_PERSPECTIVE, (c, g)
        if g.startswith("WideTrav"):
            assert g.endswith(" persist"), (c, g)
        assert g.startswith(f"{g.split('<')[0]}<{PREC[c['word_bytes']]},"), (c, g)
        assert g.endswith(" persist" if c["persist"] else " step"), (c, g)
