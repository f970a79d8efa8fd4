"""Item runs without a GPU: what the wave queue of a kernel that takes runs hands out (csrc/rt_plan.h RunPlan,
plan_runs, unit_first_chunk, unit_first_item, run_goes_on, auto_run), walked by tests/native/item_runs.cpp as the
kernel walks it -- begin_item's unit -> first item, then shade's test on the sample index at every chunk end.

The item layout is left alone; the cases steer only how many bulk chunks a pixel has. With a large full image the flat
program's automatic layout has bulk chunks of 32 samples and tail items of 8; a caller-given item size of 32 has bulk
chunks alone, the last one short when spp is no multiple of 32."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "item_runs.cpp")
FULL = 1 << 22  # pixels of the full image: large, so the automatic item size is not cut for a small frame
ELEM = 8
NPIX = (1, 3, 64, 70 * 70)
RUNS = (1, 2, 4, 8)


def build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("item_runs"), "item_runs", ["-O2"])


def ask(exe, mode, *args):
    r = subprocess.run([exe, mode, *(str(int(a)) for a in args)], capture_output=True)
    assert r.returncode == 0, (mode, args, r.stderr.decode())
    return r.stdout


def plan(exe, spp, spi, npix, run, budget=0):
    """(item plan, [run plan per pass]) as dicts"""
    lines = ask(exe, "plan", spp, spi, 1, FULL, npix, ELEM, budget, run).decode().strip().split("\n")
    pl = dict(zip(("chunk", "tail_chunk", "k_bulk", "nchunks", "cpp", "passes"), map(int, lines[0].split())))
    keys = ("chunk0", "pc", "run_log2", "runs", "n_units", "run_samples", "run_mask", "cfg", "cfg_runs", "cfg_log2")
    rps = [dict(zip(keys, map(int, ln.split()))) for ln in lines[1:]]
    for rp in rps:  # the kernels' packed word gives back the plan it was made from
        assert (rp["cfg_runs"], rp["cfg_log2"]) == (rp["runs"], rp["run_log2"]), rp
        assert (rp["cfg"] == 0) == (rp["runs"] == 0)
    return pl, rps


def spp_with_bulk(k_bulk, tail):
    """an spp whose layout has k_bulk whole bulk chunks of 32: with tail items (automatic layout: the last eighth of
    the samples, rounded, in items of 8), or without (samples_per_item 32, plus a short last chunk)"""
    if not tail:
        return 32 * k_bulk + 5, 32
    for spp in range(1, 4096):
        if (spp - int(spp * 0.125 + 0.5)) // 32 == k_bulk and spp - 32 * k_bulk > 8:
            return spp, 0
    raise AssertionError(k_bulk)


def check_pass(exe, spp, spi, npix, run, pl, rp, pass_index=0, budget=0):
    walk = np.frombuffer(ask(exe, "walk", spp, spi, 1, FULL, npix, ELEM, budget, run, pass_index), dtype=np.uint32)
    walk = walk.reshape(-1, 3)
    first, walked, last_end = walk[:, 0].astype(np.int64), walk[:, 1].astype(np.int64), walk[:, 2].astype(np.int64)
    L, runs, pc, c0 = 1 << rp["run_log2"], rp["runs"], rp["pc"], rp["chunk0"]
    n_items = npix * pc
    assert len(walk) == rp["n_units"] == n_items - runs * (L - 1) * npix
    assert L <= max(run, 1) and (runs == 0) == (L == 1)
    # the expansion the plan describes: run units first, run-major, each L items npix apart; then the single items
    n_run_units = runs * npix
    u = np.arange(len(walk))
    want_first = np.where(u < n_run_units, (u // npix) * L * npix + u % npix, u + runs * (L - 1) * npix)
    assert np.array_equal(first, want_first)
    # the test on the sample index agrees with the expansion at every chunk end
    assert np.array_equal(walked, np.where(u < n_run_units, L, 1))
    # every item of the pass exactly once, and single items after every run
    seen = np.zeros(n_items, dtype=np.int32)
    for j in range(L):
        m = walked > j
        np.add.at(seen, first[m] + j * npix, 1)
    assert (seen == 1).all()
    if runs and n_run_units < len(walk):
        assert first[n_run_units:].min() > (first[:n_run_units] + (L - 1) * npix).max()
    # the sample range a lane ends on is the layout's range of the last item it walked
    chunk = (first + (walked - 1) * npix) // npix + c0
    bulk = chunk < pl["k_bulk"]
    end = np.where(bulk, (chunk + 1) * pl["chunk"],
                   pl["k_bulk"] * pl["chunk"] + (chunk - pl["k_bulk"] + 1) * pl["tail_chunk"])
    assert np.array_equal(last_end, np.minimum(end, spp))


@pytest.mark.parametrize("tail", [True, False], ids=["tail_items", "no_tail_items"])
@pytest.mark.parametrize("run", RUNS)
def test_units_visit_every_item_once(exe, run, tail):
    for k_bulk in sorted({0, 1, run, run + 1, 2 * run + 3}):
        if k_bulk == 0 and not tail:
            continue  # (a layout without tail items has a bulk chunk)
        spp, spi = spp_with_bulk(k_bulk, tail) if k_bulk else (20, 0)  # 20 spp: three tail items
        eff = run
        while eff > 1 and k_bulk // eff == 0:
            eff //= 2  # (a run is never longer than the pixel's bulk chunks)
        for npix in NPIX:
            pl, rps = plan(exe, spp, spi, npix, run)
            assert pl["passes"] == 1 and min(pl["k_bulk"], spp // pl["chunk"]) == k_bulk, (spp, spi, pl)
            assert (pl["nchunks"] > pl["k_bulk"]) == tail
            rp = rps[0]
            assert (1 << rp["run_log2"], rp["runs"]) == (eff, k_bulk // eff if eff > 1 else 0)
            check_pass(exe, spp, spi, npix, run, pl, rp)


def test_a_run_longer_than_the_bulk_chunks_is_shortened(exe):
    spp, spi = spp_with_bulk(3, True)
    _, (rp,) = plan(exe, spp, spi, 64, 8)
    assert (rp["run_log2"], rp["runs"]) == (1, 1)
    _, (rp,) = plan(exe, *spp_with_bulk(1, True), 64, 8)
    assert (rp["run_log2"], rp["runs"], rp["n_units"]) == (0, 0, 64 * plan(exe, *spp_with_bulk(1, True), 64, 1)[0]["nchunks"])


def test_a_multi_pass_call_has_runs_in_its_first_pass_alone_and_still_visits_every_item(exe):
    spp, spi = spp_with_bulk(11, True)
    npix, run = 64, 4
    budget = 3 * ELEM * npix * 6  # six chunks per pass
    pl, rps = plan(exe, spp, spi, npix, run, budget)
    assert pl["passes"] == len(rps) > 2 and pl["cpp"] == 6
    assert [rp["runs"] for rp in rps] == [1] + [0] * (len(rps) - 1)
    for k, rp in enumerate(rps):
        check_pass(exe, spp, spi, npix, run, pl, rp, k, budget)


def test_more_runs_a_pixel_than_the_packed_word_holds(exe):
    # a caller-given item size puts no limit on a pixel's chunks: 524,288 items of 1 sample would be 65,536 runs of
    # 8, one more than the packed word's 16 bits hold; a shorter run has more still, so the pass keeps items
    spp, npix = 524288, 169
    full = npix
    for run in (2, 4, 8):
        lines = ask(exe, "plan", spp, 1, 1, full, npix, ELEM, 0, run).decode().strip().split("\n")
        c0, pc, lg, runs, n_units, _, _, cfg, cfg_runs, cfg_log2 = map(int, lines[1].split())
        assert (c0, pc) == (0, spp) and (lg, runs, cfg) == (0, 0, 0) and n_units == npix * spp
        assert (cfg_runs, cfg_log2) == (runs, lg)
    assert int(ask(exe, "auto", spp, 1, 1, full, npix, ELEM, 0, 1, 2048, 1)) == 1
    # the largest layout the word does hold: 65,535 runs of 8 (and its walk visits every item)
    spp = 8 * 65535
    pl, (rp,) = plan(exe, spp, 1, 3, 8)
    assert (rp["run_log2"], rp["runs"]) == (3, 65535)
    check_pass(exe, spp, 1, 3, 8, pl, rp)


def auto(exe, spp, full, npix, takes, lanes, budget=0, overlapped=1):
    return int(ask(exe, "auto", spp, 0, 1, full, npix, ELEM, budget, takes, lanes, overlapped))


def test_the_automatic_run_length(exe):
    lanes = 256 * 2048  # 256 CUs
    c2 = 800 * 800
    whole = auto(exe, 1024, c2, c2, 1, lanes)
    assert whole == 8
    assert auto(exe, 1024, c2, c2, 0, lanes) == 1  # the wavefront schedule
    assert auto(exe, 1024, c2, c2, 1, lanes, overlapped=0) == 1  # no next launch to hide the launch's longer end
    assert auto(exe, 1024, c2, c2, 1, lanes, budget=3 * ELEM * c2 * 20) == 1  # a multi-pass call
    assert auto(exe, 64, 400 * 400, 400 * 400, 1, lanes) == 1  # a C1-sized frame: below the bound
    # it stays or falls as the call shrinks: the whole frame down to a rank of eight's share, and below
    prev = whole
    for div in (2, 4, 8, 64):
        cur = auto(exe, 1024, c2, c2 // div, 1, lanes)
        assert cur <= prev, (div, cur, prev)
        prev = cur
    assert auto(exe, 1024, c2, c2 // 8, 1, lanes) == 1  # one rank of eight keeps items
    # and as the chip grows under the same frame
    assert auto(exe, 1024, c2, c2, 1, 8 * lanes) <= whole


def test_under_the_sanitizers(tmp_path):
    try:
        san = build(tmp_path, "item_runs_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/native/item_runs.cpp failed")
    for run in RUNS:
        for tail in (True, False):
            spp, spi = spp_with_bulk(2 * run + 3, tail)
            pl, rps = plan(san, spp, spi, 70 * 70, run)
            check_pass(san, spp, spi, 70 * 70, run, pl, rps[0])
    assert auto(san, 1024, 640000, 640000, 1, 524288) == 8
