"""The host's plan of a sponge handle (halo_amd/csrc/sponge_plan.hpp): the mode it mirrors and the permutations it
counts.

A stand-alone program (tests/sponge_plan_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
runs the stepper from every start state -- Absorbed(0), Absorbed(1), Absorbed(2), Squeezed(1), Squeezed(2) -- over
e = 0 .. 33 absorbed elements (0 .. 5 cover every transition; 32 is a batch of 16 points) and then c = 0 .. 4
squeezes.  The resulting mode and the permutation count must be those of oracle/poseidon.InnerSponge driven the
same way (a subclass counts its _permute calls instead of running them).
The elements per absorbed item are 2 for a point, 1 for an fq, and 2 / 1 for an fr on Pallas / Vesta.

The launch plan of a batch of k sponges (the lane rule and the grid, which every sponge kernel's launcher reads) is
swept against its restatement here: three lanes per sponge (21 sponges a wave) while their waves number at most
eight per compute unit, else one lane (64 a wave), unless the tuning value pins 1 or 3; blocks of one wave up to
4096 waves and of four waves beyond.
"""
import os
import shutil
import subprocess

import pytest

import poseidon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STARTS = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)]
TUNES = (0, 1, 3)      # the free choice and both pinned layouts
CUS = (1, 8, 256, 304)


def plan_ks(cu):
    """Around a wave of either layout (20..22, 63..65), around the lane rule's switch at 21 * 8 * CU sponges and
    around the switch of waves per block at 4096 / 4097 waves of either layout."""
    edge = 21 * 8 * cu
    return sorted({1, 20, 21, 22, 63, 64, 65, edge - 1, edge, edge + 1, 21 * 4096, 21 * 4096 + 1, 64 * 4096, 64 * 4096 + 1,
                   1000003} - {0})


def plan_ref(tune, cu, k):
    waves3 = -(-k // 21)
    lanes = tune if tune in (1, 3) else (3 if waves3 <= 8 * cu else 1)
    waves = waves3 if lanes == 3 else -(-k // 64)
    wpb = 4 if waves > 4096 else 1
    return lanes, -(-waves // wpb), 64 * wpb


class CountingSponge(poseidon.InnerSponge):
    """The reference's state machine alone: _permute is counted, not run."""

    def __init__(self, squeezed, n):
        self.m, self.state, self.perms = 1 << 61, [0, 0, 0], 0
        self.mode, self.n = ("squeezed" if squeezed else "absorbed"), n

    def _permute(self):
        self.perms += 1


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sponge_plan") / "sponge_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sponge_plan_dump.cpp"), "-o", exe], check=True)
    plans = "".join(f"plan {t} {cu} {k}\n" for t in TUNES for cu in CUS for k in plan_ks(cu))
    out = subprocess.run([exe], input="steps 33 4\nitems 0 0\n" + plans, capture_output=True, text=True, check=True)
    rows = [l.split() for l in out.stdout.splitlines()]
    return ([tuple(int(x) for x in r[1:]) for r in rows if r[0] == "s"],
            [tuple(int(x) for x in r[1:]) for r in rows if r[0] == "i"],
            [tuple(int(x) for x in r[1:]) for r in rows if r[0] == "p"])


def test_every_step_matches_the_inner_sponge(dump):
    steps = dump[0]
    assert len(steps) == 5 * 34 * 5
    seen = set()
    for sq, n, e, c, sq2, n2, perms in steps:
        seen.add((sq, n, e, c))
        s = CountingSponge(sq, n)
        s.absorb([7] * e)
        for _ in range(c):
            s.squeeze()
        assert (sq2, n2, perms) == (int(s.mode == "squeezed"), s.n, s.perms), (sq, n, e, c)
    assert seen == {(sq, n, e, c) for sq, n in STARTS for e in range(34) for c in range(5)}


def test_the_cases_the_prover_transcript_takes(dump):
    """Sponge::new absorbs the label (Absorbed(1)); 32 elements of C_ws, two squeezes; 2 of C_z, one squeeze; 32 of
    C_ts, two squeezes: 34 permutations (DESIGN §4.8's count for the verifier's side of the same transcript)."""
    plan = {(sq, n, e, c): (sq2, n2, p) for sq, n, e, c, sq2, n2, p in dump[0]}
    assert plan[0, 0, 1, 0] == (0, 1, 0)
    assert plan[0, 1, 0, 1] == (1, 1, 1) and plan[1, 1, 0, 1] == (1, 2, 0) and plan[1, 2, 0, 1] == (1, 1, 1)
    assert plan[1, 1, 1, 0] == (0, 1, 0) and plan[1, 2, 1, 0] == (0, 1, 0)  # an absorb after a squeeze permutes nothing
    perms, mode = 0, (0, 0)
    for e, c in ((1, 0), (32, 2), (2, 1), (32, 2)):
        sq, n, p = plan[mode + (e, c)]
        perms, mode = perms + p, (sq, n)
    assert perms == 34 and mode == (1, 2)


def test_elements_per_item(dump):
    items = dump[1]
    assert sorted(items) == [(0, 0, 2), (0, 1, 2), (1, 0, 1), (1, 1, 2), (2, 0, 1), (2, 1, 1)]


def test_the_launch_plan_matches_its_restatement(dump):
    plans = dump[2]
    assert [(t, cu, k) for t, cu, k, *_ in plans] == [(t, cu, k) for t in TUNES for cu in CUS for k in plan_ks(cu)]
    for t, cu, k, lanes, blocks, threads in plans:
        assert (lanes, blocks, threads) == plan_ref(t, cu, k), (t, cu, k)


def test_the_grid_covers_every_sponge_and_wastes_less_than_a_block(dump):
    for t, cu, k, lanes, blocks, threads in dump[2]:
        per_block = (threads // 64) * (21 if lanes == 3 else 64)
        assert threads in (64, 256) and lanes in (1, 3)
        assert blocks * per_block >= k > (blocks - 1) * per_block, (t, cu, k)
        if t in (1, 3):
            assert lanes == t


def test_the_lane_rule_switches_at_eight_waves_per_compute_unit(dump):
    free = {(cu, k): lanes for t, cu, k, lanes, _, _ in dump[2] if t == 0}
    for cu in CUS:
        assert free[cu, 21 * 8 * cu] == 3 and free[cu, 21 * 8 * cu + 1] == 1
    grid = {(t, k): (blocks, threads) for t, cu, k, _, blocks, threads in dump[2] if cu == 256}
    assert grid[3, 21 * 4096] == (4096, 64) and grid[3, 21 * 4096 + 1] == (1025, 256)
    assert grid[1, 64 * 4096] == (4096, 64) and grid[1, 64 * 4096 + 1] == (1025, 256)
