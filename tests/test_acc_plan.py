"""The counts of an accumulation's ASDL transcript (halo_amd/csrc/acc_plan.hpp).

A stand-alone program (tests/acc_plan_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
prints, for m = 1 .. 64 instances, lg n = 0 .. 24 and both NS (base-field elements per absorbed scalar: 2 on Pallas,
1 on Vesta), the absorbed elements, the absorb permutations and the steps of the alpha^j ladder:

  elements = 1 + NS m (lg n + 1) + 2 m       the label, the challenges, the coordinates of the U
  permutations = ceil(elements / 2)          the rate-2 sponge
  steps = the bit length of m - 1, at most ceil(lg m) + 1, and 2^steps >= m (every j < m fits)
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("acc_plan") / "acc_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "acc_plan_dump.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], input="sweep 64 24\n", capture_output=True, text=True, check=True)
    return [tuple(int(x) for x in l.split()) for l in out.stdout.splitlines()]


def test_every_count_matches_the_formula(rows):
    assert len(rows) == 64 * 25 * 2
    seen = set()
    for m, lg, ns, elements, perms, steps in rows:
        seen.add((m, lg, ns))
        assert elements == 1 + ns * m * (lg + 1) + 2 * m
        assert perms == -(-elements // 2)
        assert steps == (m - 1).bit_length() and (1 << steps) >= m and steps <= (m - 1).bit_length() + 1
    assert len(seen) == len(rows)


def test_the_parities_the_gpu_tests_rely_on(rows):
    count = {(m, lg, ns): e for m, lg, ns, e, _, _ in rows}
    assert count[1, 4, 1] == 8 and count[2, 4, 1] == 15  # Vesta at n = 16: m = 1 even, m = 2 odd
    assert all(count[m, lg, 2] % 2 == 1 for m in range(1, 65) for lg in range(25))  # Pallas: always odd
    assert count[3, 16, 2] == 109 and count[3, 20, 2] == 133  # the Plonk verifier's m = 3 walks
