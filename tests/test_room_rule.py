"""csrc/rt_room.h, the open-box slab rule the flat program traces a room's walls with, against brute force.

tests/native/room_rule.cpp (plain C++, no HIP) draws seeded rays -- from inside, from outside toward the back of
the faces, toward the opening, with the origin exactly on a wall plane, with a direction component of exactly
zero -- for the closed box and for each of the six open faces, and compares the rule with one quad test per
existing face (the arithmetic of rt_device.h flat_quad_test): the same face and the same bits of t on every ray.
It is run once as built, and once built with the address and undefined-behaviour sanitizers, as a program of
its own."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cpu-ray-tracing-implementation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "room_rule.cpp")
MASKS = 7  # the closed box and six open faces


def build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def run(exe, per_mask):
    r = subprocess.run([exe, str(per_mask)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == MASKS + 1
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) == MASKS * per_mask
    # every class of ray hits something under every mask: none of the classes is empty
    for ln in lines[:-1]:
        counts = [int(v) for v in ln.split("class")[1].split()]
        assert len(counts) == 5 and min(counts) > per_mask // 200, ln
    return int(last[2])


def test_rule_matches_the_quad_tests_on_a_million_rays(tmp_path):
    hits = run(build(tmp_path, "room_rule", ["-O2"]), 150000)  # 1.05 M rays
    assert hits > 500000


def test_rule_under_the_sanitizers(tmp_path):
    try:
        exe = build(tmp_path, "room_rule_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.fail("the sanitizer build of tests/native/room_rule.cpp failed")
    run(exe, 20000)
