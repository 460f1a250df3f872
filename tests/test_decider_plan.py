"""The group plan of the exact batched decider (halo_amd/csrc/decider_plan.hpp).

A stand-alone program (tests/decider_plan_dump.cpp, built here by the host C++ compiler: the header is free of
HIP) sweeps n over 1 .. 2^24 (every power of two and its two neighbours) and k over 1 .. 4096 and counts the
plans that break a property:

  g >= 1, and g <= k;
  g n <= budget, or g = 1 (one instance alone may exceed the budget);
  the groups cover k exactly (ceil(k / g) groups, the last one not empty);
  g W n < 2^32, the entries the one-MSM batch path accepts (W windows per scalar).

W takes the window counts of the resident tables (15 at c = 17, 17 at c = 15) and the largest any window width
gives (43 at c = 6); the budget its default 2^25, a small one, and one so large that only the 2^32 bound holds.
A few plans are compared with literals worked out by hand.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("decider_plan") / "decider_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "decider_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


@pytest.mark.parametrize("budget", [1 << 25, 5 * 1024, 1 << 40])
@pytest.mark.parametrize("W", [15, 17, 43])
def test_every_plan_keeps_the_properties(dump, budget, W):
    got = dump(["sweep 0 24 4096 %d %d" % (budget, W)])[0]
    assert got.pop("checked") == (3 * 25 - 2) * 4096  # n = 0 and n = 2^24 + 1 are outside the range
    assert got == {"g_below_1": 0, "g_above_k": 0, "over_budget": 0, "cover": 0, "entries": 0}


def test_literal_plans(dump):
    cases = [
        # (n, k, budget, W) -> (g, groups)
        ((1 << 20, 4096, 1 << 25, 15), (32, 128)),   # the headline: 32 rows of 2^20 are 1 GiB
        ((1 << 20, 64, 1 << 25, 15), (32, 2)),
        ((1 << 20, 1, 1 << 25, 15), (1, 1)),
        ((1 << 16, 4096, 1 << 25, 17), (512, 8)),
        ((1 << 10, 5, 2 * 1024, 17), (2, 3)),        # tests/test_gpu_decider.py's three groups
        ((1 << 24, 7, 1 << 20, 15), (1, 7)),         # one instance alone exceeds the budget
        ((1 << 18, 4096, 1 << 40, 15), (1092, 4)),   # only the 2^32 entries bound: floor((2^32 - 1) / (15 2^18))
        ((1, 3, 1 << 25, 43), (3, 1)),
    ]
    got = dump(["plan %d %d %d %d" % c for c, _ in cases])
    assert [(g["g"], g["groups"]) for g in got] == [want for _, want in cases]
