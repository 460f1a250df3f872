"""The shape of the generator's fixed-base comb (halo_amd/csrc/fixed_base_plan.hpp): the recoding of a scalar into
signed digits, the table index of (window, digit) and the grid of a batch.

A stand-alone program (tests/fixed_base_plan_dump.cpp, built here by the host C++ compiler: the header is free of
HIP) recodes the edge scalars of tests/fixed_base_cases.py and 2000 seeded random scalars per field.  For each one:
every digit is in range, sum_w d_w 2^(c w) is the scalar exactly (the plan does not fold, so there is no sign rule),
no carry leaves the top window, and every table index is inside the table and is the slot of (window, |digit|).
The recoder under test is the one the kernel runs.  The grid covers k = 1, 63, 64, 65, 2^20 + 1.
"""
import json
import os
import random
import shutil
import subprocess

import pytest

import pasta as P
from fixed_base_cases import edge_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["pallas", "vesta"]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("fixed_base_plan") / "fixed_base_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fixed_base_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


@pytest.fixture(scope="module")
def plan(dump):
    return dump(["plan"])[0]


def words(x: int) -> str:
    return " ".join(str((x >> (32 * q)) & 0xFFFFFFFF) for q in range(8))


def test_plan_constants(plan):
    c, W = plan["c"], plan["windows"]
    assert c in (4, 8) and W * c == 256
    assert plan["half"] == 1 << (c - 1)
    assert plan["entries"] == W * plan["half"] and plan["entry_bytes"] == 64
    assert plan["table_bytes"] == plan["entries"] * 64
    assert plan["table_bytes"] <= 4 << 20  # an XCD's L2
    assert plan["threads"] % 64 == 0


def check_recoding(plan, got, scalars):
    c, W, half = plan["c"], plan["windows"], plan["half"]
    assert len(got) == len(scalars)
    for x, g in zip(scalars, got):
        d = g["digits"]
        assert len(d) == W and len(g["index"]) == W, hex(x)
        assert all(-half <= v <= half for v in d), hex(x)
        assert sum(v << (c * w) for w, v in enumerate(d)) == x, hex(x)
        assert g["carry"] == 0, hex(x)
        for w, (v, idx) in enumerate(zip(d, g["index"])):
            if v == 0:
                assert idx == -1, (hex(x), w)
            else:
                assert idx == w * half + abs(v) - 1 and 0 <= idx < plan["entries"], (hex(x), w)


@pytest.mark.parametrize("cname", CURVES)
def test_edge_scalars(dump, plan, cname):
    E = edge_scalars(cname)
    assert len(E) == 15 + 5 + 255 + 64
    check_recoding(plan, dump(["digits " + words(x) for x in E]), E)


@pytest.mark.parametrize("cname", CURVES)
def test_random_scalars(dump, plan, cname):
    r = P.CURVES[cname].scalar
    rng = random.Random(0xF1BA5E + CURVES.index(cname))
    xs = [rng.randrange(r) for _ in range(2000)]
    check_recoding(plan, dump(["digits " + words(x) for x in xs]), xs)


@pytest.mark.parametrize("cname", CURVES)
def test_the_doubling_case_is_what_the_comment_says(dump, plan, cname):
    """2^255 - r: the top digit is 2^254 / 2^(c (W - 1)) and the windows below it sum to 2^254 - r."""
    r = P.CURVES[cname].scalar
    c, W = plan["c"], plan["windows"]
    d = dump(["digits " + words((1 << 255) - r)])[0]["digits"]
    assert d[W - 1] == (1 << 254) >> (c * (W - 1))
    low = sum(v << (c * w) for w, v in enumerate(d[:-1]))
    assert low == (1 << 254) - r and low % r == (1 << 254) % r


def test_the_largest_integers_below_2_255_leave_no_carry(dump, plan):
    """The plan's static assertion, seen from outside: the bound holds for every integer below 2^255, not only below r."""
    xs = [(1 << 255) - 1, (1 << 255) - 2, int.from_bytes(b"\x80" * 31 + b"\x7f", "little"), (1 << 255) - (1 << 247)]
    check_recoding(plan, dump(["digits " + words(x) for x in xs]), xs)


def test_grid_covers_the_batch(dump, plan):
    ks = [1, 63, 64, 65, 127, 128, 129, (1 << 20) + 1]
    for k, g in zip(ks, dump(["grid %d" % k for k in ks])):
        t = g["threads"]
        assert t == plan["threads"]
        assert g["blocks"] * t >= k > (g["blocks"] - 1) * t, k
