"""The host's render plan (csrc/rt_plan.h: pure C++, no HIP): the item layout and its passes, div_magic, and the
kernel family a render takes. tests/native/plan_dump.cpp answers one question per input line; the invariants, the
pinned BASELINE layouts and the family table are checked here."""
import os
import random
import subprocess

import pytest

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
