"""CPU tests of the bisecting Schnorr batch: the descent of halo_amd/csrc/schnorr_bisect.hpp against a toy group, and
the argument contract of halo_schnorr_verify_bisect_dev and the tuning keys schnorr_bisect, schnorr_bisect_leaf and
schnorr_bisect_pass_items (include/halo_gpu.h).

A stand-alone program (tests/schnorr_bisect_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
runs the same sig_bisect_descend loop as schnorr_bisect.hip with a stand-in for the device: D(S) = sum of rho_i over
the wrong items of S in Z / (2^61 - 1), under weights with which no nonempty sum vanishes, and an exact ladder.  For
every case it checks

  the verdicts are exactly the wrong items;
  passes c <= k (the budget rule's bound);
  the ladder slices are pairwise disjoint, inside [0, k), nodes of the tree, and failing;
  under (L, c) = (1, 1) no ladder runs and the passes number the failing internal nodes of the tree, counted
  independently: at most min(k - 1, b ceil(lg k)) for b wrong items, over at most ceil(lg k) levels;
  k < c or k <= L gives one ladder over [0, k) and no pass (a batch of one needs neither: its defect is its verdict);
  every node obeys the split rule and `src` names its own, nonzero, defect.

Every subset of k = 1 .. 10 items is swept under four settings of the rules; random subsets, from one wrong item to
all of them, at k = 63, 64, 65, 4095, 4096.  A few traces are compared with literals worked out by hand.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from halo_amd import _lib as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = {"bad_verdict": 0, "over_budget": 0, "bad_ladder": 0, "bad_full": 0, "bad_root": 0, "bad_defect": 0}
RULES = [(1, 1), (2, 1), (4, 2), (1, 4)]  # (L, c)
OK, EINVAL = 0, 1
GOLDEN = os.path.join(ROOT, "tests", "golden", "transcript.npz")
NAME = "halo_schnorr_verify_bisect_dev"


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("schnorr_bisect") / "schnorr_bisect_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "schnorr_bisect_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


@pytest.mark.parametrize("L,c", RULES)
def test_every_subset_up_to_ten(dump, L, c):
    got = dump(["sweep %d %d %d" % (k, L, c) for k in range(1, 11)])
    for k, g in zip(range(1, 11), got):
        assert g.pop("cases") == 1 << k
        assert g == CLEAN, k


@pytest.mark.parametrize("k", [63, 64, 65, 4095, 4096])
def test_random_subsets(dump, k):
    rules = RULES + [(64, 16), (1, 16), (32768, 16384)]
    got = dump(["random %d %d %d 40 %d" % (k, L, c, k + j) for j, (L, c) in enumerate(rules)])
    for g in got:
        assert g.pop("cases") == 40
        assert g == CLEAN


def test_literal_traces(dump):
    one, last5, budget, leaf, small, root_c = dump([
        "trace 8 1 1 5", "trace 5 1 1 4", "trace 64 1 16 3 20 40 63", "trace 17 4 1 2 9", "trace 4 4 1 1", "trace 8 1 16 1"])
    assert all(t["clean"] for t in (one, last5, budget, leaf, small, root_c))
    # k = 8, wrong {5}: three levels, one pass each, no ladder
    assert one["ok"] == [1, 1, 1, 1, 1, 0, 1, 1] and one["passes"] == 3 and one["ladders"] == []
    assert one["levels"] == [[[0, 4, 8, 0]], [[4, 6, 8, 1]], [[4, 5, 6, 0]]]
    # k = 5, wrong {4}: [0, 2) | [2, 5), then [2, 3) | [3, 5), then [3, 4) | [4, 5)
    assert last5["ok"] == [1, 1, 1, 1, 0] and last5["passes"] == 3
    assert last5["levels"] == [[[0, 2, 5, 0]], [[2, 3, 5, 1]], [[3, 4, 5, 1]]]
    # k = 64, c = 16, one wrong item per quarter: (0 + 1) 16 <= 64 and (1 + 2) 16 <= 64 admit levels 0 and 1, then
    # (3 + 4) 16 > 64 stops the descent at level 2 and the four quarters go to the ladder
    assert budget["passes"] == 3 and budget["levels"] == [[[0, 32, 64, 0]], [[0, 16, 32, 0], [32, 48, 64, 1]]]
    assert budget["ladders"] == [[0, 16], [16, 32], [32, 48], [48, 64]]
    assert [i for i, v in enumerate(budget["ok"]) if not v] == [3, 20, 40, 63]
    # k = 17, L = 4, wrong {2, 9}: [0, 8) | [8, 17); [0, 4) fails with four items: a leaf; [8, 12) likewise
    assert leaf["levels"] == [[[0, 8, 17, 0]], [[0, 4, 8, 0], [8, 12, 17, 1]]]
    assert leaf["ladders"] == [[0, 4], [8, 12]] and leaf["passes"] == 3
    assert [i for i, v in enumerate(leaf["ok"]) if not v] == [2, 9]
    # k <= L and k < c: the root goes straight to the ladder
    for t, k in ((small, 4), (root_c, 8)):
        assert t["passes"] == 0 and t["levels"] == [] and t["ladders"] == [[0, k]]
        assert t["ok"] == [1, 0] + [1] * (k - 2)


# ---------------------------------------------------------------------------------------------
# the ABI, before any device work
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(H.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(os.path.dirname(H.LIB_PATH), "..", "csrc")], check=True)
    lib = H.load()
    g = np.load(GOLDEN)
    for name, f in (("fp", H.FP), ("fq", H.FQ)):  # host-only call: no GPU needed
        mds, rc = H.fe_array(g[f"poseidon_{name}_mds"], 9), H.fe_array(g[f"poseidon_{name}_rc"], 165)
        assert lib.halo_poseidon_set_params(f, H.ptr(mds), H.ptr(rc)) == OK
    return lib


def test_abi_version_114_and_the_symbol(L):
    assert L.halo_abi_version() >= 114
    assert NAME in H.SIGNATURES and NAME not in H.missing_symbols()
    assert hasattr(L, NAME)


def test_an_empty_batch_is_ok_and_touches_nothing(L):
    assert getattr(L, NAME)(H.VESTA, None, None, None, None, 10, 0, None, None, None, None) == OK


def test_refusals_are_those_of_the_combined_dev_call(L):
    a = np.zeros((4, 8), dtype=np.uint64)
    one = np.ones((4, 4), dtype=np.uint64)
    p, r = H.ptr(a), H.ptr(one)
    for name in (NAME, "halo_schnorr_verify_combined_dev"):
        fn = getattr(L, name)
        seen = []
        for hole in range(4):  # pk, R, s; msgs may be NULL only when msg_len = 0
            ptrs = [p, p, p, p]
            ptrs[hole] = None
            seen.append((fn(H.VESTA, *ptrs, 1, 1, r, p, None, None), H.last_error()))
        seen.append((fn(H.VESTA, p, p, p, p, 1, 1, r, None, None, None), H.last_error()))  # d_ok
        seen.append((fn(2, p, p, p, p, 1, 1, r, p, None, None), H.last_error()))
        seen.append((fn(-1, p, p, p, p, 1, 1, r, p, None, None), H.last_error()))
        seen.append((fn(H.PALLAS, p, p, p, p, 1, 119304647, r, p, None, None), H.last_error()))
        assert [rc for rc, _ in seen] == [EINVAL] * 8
        assert all(name in msg for _, msg in seen)
        assert [msg.replace(name, "") for _, msg in seen] == [": null pointer"] * 5 + [": unknown curve"] * 2 + [
            ": 119304647 signatures in one call (at most 119304646)"]
        # a NULL d_rho means derived weights, a NULL msgs with msg_len = 0 is no hole: neither is refused here
        assert fn(H.VESTA, None, None, None, None, 0, 0, None, None, None, None) == OK


@pytest.mark.parametrize("key,default", [("schnorr_bisect", 0), ("schnorr_bisect_leaf", None), ("schnorr_bisect_pass_items", None)])
def test_the_keys_round_trip(L, key, default):
    d = H.get_tuning(key)
    if default is not None:
        assert d == default
    assert d >= 0
    try:
        H.set_tuning(key, 7)
        assert H.get_tuning(key) == 7
        H.set_tuning(key, -1)
        assert H.get_tuning(key) == d
        with H.tuning(**{key: 3}):
            assert H.get_tuning(key) == 3
        assert H.get_tuning(key) == d
    finally:
        H.set_tuning(key, -1)


def test_the_default_leaf_is_twice_the_pass_items(L):
    c, leaf = H.get_tuning("schnorr_bisect_pass_items"), H.get_tuning("schnorr_bisect_leaf")
    assert c >= 1 and c & (c - 1) == 0 and leaf == 2 * c


def test_bisect_without_weights_is_an_error():
    from halo_amd import schnorr
    z = np.zeros((1, 8), dtype=np.uint64)
    with pytest.raises(ValueError, match="bisect"):
        schnorr.verify_batch(z, z, np.ones((1, 4), dtype=np.uint64), np.zeros((1, 0, 4), dtype=np.uint64), bisect=True)
