"""CPU tests of the bisecting decider: the descent of halo_amd/csrc/decider_bisect.hpp against a toy group, and the
argument contract of halo_pcdl_decide_bisect_dev and the tuning key decide_bisect (include/halo_gpu.h).

A stand-alone program (tests/decider_bisect_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
runs the same bisect_descend loop as decider.hip with a stand-in for the device: D(S) = sum of rho_i delta_i over the
wrong instances of S in Z / (2^61 - 1), with weights under which no nonempty sum vanishes.  For every case it checks

  the verdicts are exactly the wrong instances;
  the rows asked for beyond the root pass number the failing internal nodes of the tree, counted independently, and
  are at most min(k - 1, b ceil(lg k)) for b wrong instances; the levels number at most ceil(lg k);
  every node obeys the split rule left = [lo, lo + floor((hi - lo) / 2)) and `src` names its own, nonzero, defect;
  each level's groups come in order without gaps, only the last one ragged, none above decider_group's g, within the
  budget unless it is one row, and below the 2^32 entries of the one-MSM path.

Every subset of k = 1 .. 10 instances is swept under both weightings and three group budgets; random subsets, from one
wrong instance to all of them, at k = 63, 64, 65, 4095, 4096.  A few traces are compared with literals worked out by
hand.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from halo_amd import _lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = {"bad_verdict": 0, "bad_rows": 0, "over_bound": 0, "bad_group": 0, "bad_defect": 0, "deep": 0}
OK, EINVAL, ENOTPOW2 = 0, 1, 4


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("decider_bisect") / "decider_bisect_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "decider_bisect_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


# n = 1024 coefficients, W = 17 windows; budgets: the default (one group per level), two rows, one row
@pytest.mark.parametrize("budget", [1 << 25, 2048, 1024])
@pytest.mark.parametrize("weights", ["inc", "signed"])
def test_every_subset_up_to_ten(dump, weights, budget):
    got = dump(["sweep %d 1024 %d 17 %s" % (k, budget, weights) for k in range(1, 11)])
    for k, g in zip(range(1, 11), got):
        assert g.pop("cases") == 1 << k
        assert g == CLEAN, k


@pytest.mark.parametrize("k", [63, 64, 65, 4095, 4096])
def test_random_subsets(dump, k):
    # n = 2^16, W = 17: the default budget holds 512 rows, so k = 4096 all wrong needs four groups at the widest level
    got = dump(["random %d 65536 %d 17 40 %d" % (k, 1 << 25, k), "random %d 1024 3072 17 40 %d" % (k, k + 1)])
    for g in got:
        assert g.pop("cases") == 40
        assert g == CLEAN


def test_literal_traces(dump):
    one, all8, last5, two_groups = dump(["trace 8 4096 %d 15 5" % (1 << 25), "trace 8 4096 %d 15 0 1 2 3 4 5 6 7" % (1 << 25),
                                         "trace 5 4096 %d 15 4" % (1 << 25), "trace 8 4096 8192 15 0 1 2 3 4 5 6 7"])
    assert all(t["clean"] for t in (one, all8, last5, two_groups))
    # k = 8, wrong {5}: three levels, one row each
    assert one["ok"] == [1, 1, 1, 1, 1, 0, 1, 1] and one["rows"] == 3
    assert [l["nodes"] for l in one["levels"]] == [[[0, 4, 8, 0]], [[4, 6, 8, 1]], [[4, 5, 6, 0]]]
    assert [l["groups"] for l in one["levels"]] == [[1], [1], [1]]
    # k = 8, all wrong: 1 + 2 + 4 rows, every level one group
    assert all8["ok"] == [0] * 8 and all8["rows"] == 7
    assert [l["nodes"] for l in all8["levels"]] == [
        [[0, 4, 8, 0]], [[0, 2, 4, 0], [4, 6, 8, 1]], [[0, 1, 2, 0], [2, 3, 4, 1], [4, 5, 6, 2], [6, 7, 8, 3]]]
    assert [l["groups"] for l in all8["levels"]] == [[1], [2], [4]]
    # ... and with a budget of two rows the last level takes two groups
    assert [l["groups"] for l in two_groups["levels"]] == [[1], [2], [2, 2]]
    # k = 5, wrong {4}: [0, 2) | [2, 5), then [2, 3) | [3, 5), then [3, 4) | [4, 5)
    assert last5["ok"] == [1, 1, 1, 1, 0] and last5["rows"] == 3
    assert [l["nodes"] for l in last5["levels"]] == [[[0, 2, 5, 0]], [[2, 3, 5, 1]], [[3, 4, 5, 1]]]


# ---------------------------------------------------------------------------------------------
# the ABI, before any device work
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(H.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(os.path.dirname(H.LIB_PATH), "..", "csrc")], check=True)
    return H.load()


def test_abi_version_106(L):
    assert L.halo_abi_version() >= 106


def test_the_symbol_exists_and_an_empty_batch_is_ok(L):
    assert hasattr(L, "halo_pcdl_decide_bisect_dev")
    assert L.halo_pcdl_decide_bisect_dev(0, 15, 0, None, None, None, None, None, None) == OK


def test_decide_bisect_tuning_key(L):
    assert H.get_tuning("decide_bisect") == 0
    H.set_tuning("decide_bisect", 1)
    assert H.get_tuning("decide_bisect") == 1
    H.set_tuning("decide_bisect", -1)
    assert H.get_tuning("decide_bisect") == 0
    with H.bisecting(True):
        assert H.get_tuning("decide_bisect") == 1
    assert H.get_tuning("decide_bisect") == 0
    with H.bisecting(False):
        assert H.get_tuning("decide_bisect") == 0


def test_decide_bisect_dev_argument_errors(L):
    k, lg = 3, 4
    xis = np.ones((k * (lg + 1), 4), dtype=np.uint64)
    U = np.zeros((k, 8), dtype=np.uint64)
    rho = np.ones((k, 4), dtype=np.uint64)
    ok = np.zeros(k, dtype=np.uint8)
    fn, name = L.halo_pcdl_decide_bisect_dev, "halo_pcdl_decide_bisect_dev"
    good = [H.ptr(xis), H.ptr(U), None, H.ptr(rho), H.ptr(ok)]
    assert fn(7, 15, k, *good, None) == EINVAL and name in H.last_error() and "unknown curve" in H.last_error()
    assert fn(0, 14, k, *good, None) == ENOTPOW2
    assert H.last_error() == "n (15) is not a power of two"
    for hole in (0, 1, 4):
        args = list(good)
        args[hole] = None
        assert fn(0, 15, k, *args, None) == EINVAL and H.last_error() == name + ": null pointer"
    args = list(good)
    args[3] = None
    assert fn(1, 15, k, *args, None) == EINVAL and H.last_error() == name + ": null d_rho"
