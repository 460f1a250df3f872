"""The shape of the derived decider weights (halo_amd/csrc/rho_plan.hpp) and their CPU restatement (tests/rho_ref.py).

A stand-alone program (tests/rho_plan_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
reports, for k = 1 .. 4097, that the level counts halve with promotion of an odd element and end at 1 after
ceil(lg k) levels, that a derivation is 2 + ceil(lg k) launches, the leaf's element and permutation counts for
both curve directions at lg n = 0 .. 28, and the "zero becomes one" helper that the kernel shares with the host.
(The replacement cannot be reached on the device without a Poseidon preimage of zero: this is its only test.)

tests/rho_ref.py is compared with the committed fixture tests/golden/rho_fs.npz (tests/golden/make_rho_fs.py), which
guards the definition from drift, and checked for the properties the derivation is built for: weights below the
scalar modulus, nonzero and distinct; an instance that is not live influences nothing; one changed word of a live
instance changes every live weight, except in xi_0, which is not hashed.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pasta as P
import poseidon
import rho_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "rho_fs.npz"))
CURVES = ["pallas", "vesta"]
CASES = {"k1_lg0": (1, 0, False), "k2_lg1": (2, 1, False), "k3_lg3": (3, 3, False), "k5_lg3": (5, 3, False),
         "k5_lg3_live": (5, 3, True)}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("rho_plan") / "rho_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rho_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


# ---------------------------------------------------------------------------------------------
# rho_plan.hpp
# ---------------------------------------------------------------------------------------------
def test_levels_halve_with_promotion_and_end_at_one(dump):
    got = dump(["levels 4097"])[0]
    assert got == {"checked": 4097, "halving": 0, "end": 0, "levels": 0, "launches": 0, "launches_0": 0}


def test_literal_level_counts(dump):
    cases = {1: [1], 2: [2, 1], 3: [3, 2, 1], 5: [5, 3, 2, 1], 64: [64, 32, 16, 8, 4, 2, 1], 65: [65, 33, 17, 9, 5, 3, 2, 1],
             257: [257, 129, 65, 33, 17, 9, 5, 3, 2, 1], 4096: [4096 >> j for j in range(13)]}
    got = dump(["counts %d" % k for k in cases])
    for g, (k, want) in zip(got, cases.items()):
        assert g == {"counts": want, "levels": len(want) - 1, "launches": len(want) + 1}, k


def test_leaf_element_counts_for_both_directions(dump):
    got = dump(["leaf 28"])[0]
    # Vesta: the scalar field is the smaller one, a scalar is one element; Pallas: two
    assert got["below"] == [[3 + lg, (4 + lg) // 2] for lg in range(29)]
    assert got["above"] == [[3 + 2 * lg, lg + 2] for lg in range(29)]


@pytest.mark.parametrize("cname", CURVES)
def test_leaf_permutations_are_those_the_restated_sponge_runs(dump, cname, monkeypatch):
    got = dump(["leaf 5"])[0]["below" if cname == "vesta" else "above"]
    count = [0]
    permute = poseidon.InnerSponge._permute

    def counting(self):
        count[0] += 1
        permute(self)

    monkeypatch.setattr(poseidon.InnerSponge, "_permute", counting)
    for lg in range(6):
        count[0] = 0
        rho_ref.leaf(cname, np.zeros(8, dtype=np.uint64), np.ones((lg + 1, 4), dtype=np.uint64))
        assert count[0] == got[lg][1], lg


def test_zero_becomes_one(dump):
    got = dump(["zero 0 0 0 0 0 0 0 0", "zero 1 0 0 0 0 0 0 0", "zero 0 0 0 0 0 0 0 1", "zero 0 0 0 7 0 0 0 0",
                "zero 4294967295 4294967295 4294967295 4294967295 4294967295 4294967295 4294967295 4294967295"])
    assert [g["w"] for g in got] == [[1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1],
                                     [0, 0, 0, 7, 0, 0, 0, 0], [4294967295] * 8]
    assert rho_ref.zero_becomes_one(0) == 1 and rho_ref.zero_becomes_one(5) == 5


# ---------------------------------------------------------------------------------------------
# rho_ref.py
# ---------------------------------------------------------------------------------------------
def fixture_case(cname, case):
    k, lg, masked = CASES[case]
    live = G[f"{cname}_{case}_live"].tolist()
    assert (live != [1] * k) == masked
    return G[f"{cname}_{case}_xis"], G[f"{cname}_{case}_U"], (1 << lg) - 1, live if masked else None, G[f"{cname}_{case}_rho"]


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("cname", CURVES)
def test_rho_ref_against_the_committed_fixture(cname, case):
    xis, U, d, live, want = fixture_case(cname, case)
    assert xis.shape == (CASES[case][0], CASES[case][1] + 1, 4) and U.shape == (CASES[case][0], 8)
    got = rho_ref.weights(cname, xis, U, d, live)
    assert got.dtype == np.uint64 and np.array_equal(got, want)


def test_the_fixture_is_what_its_generator_makes():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_rho_fs
    finally:
        sys.path.pop(0)
    assert sorted(make_rho_fs.CASES) == sorted(CASES)
    for cname in CURVES:
        for case in CASES:
            xis, U, lv, d, _ = make_rho_fs.inputs(cname, case)
            assert np.array_equal(xis, G[f"{cname}_{case}_xis"]) and np.array_equal(U, G[f"{cname}_{case}_U"])
            assert np.array_equal(lv, G[f"{cname}_{case}_live"])


@pytest.mark.parametrize("cname", CURVES)
def test_weights_are_below_the_modulus_nonzero_and_distinct(cname):
    m = P.CURVES[cname].scalar
    for case in CASES:
        xis, U, d, live, _ = fixture_case(cname, case)
        w = rho_ref.weights_int(cname, xis, U, d, live)
        on = [True] * len(w) if live is None else [bool(b) for b in live]
        assert all(0 < x < m for x, o in zip(w, on) if o) and all(x == 0 for x, o in zip(w, on) if not o)
        assert len({x for x, o in zip(w, on) if o}) == sum(on)


@pytest.mark.parametrize("cname", CURVES)
def test_the_shape_of_the_batch_is_bound(cname):
    """The same instances under another k or another mask give other weights: a batch of 2 is no prefix of a batch
    of 3, and masking the third instance out is neither."""
    xis, U, d, _, _ = fixture_case(cname, "k3_lg3")
    w3 = rho_ref.weights_int(cname, xis, U, d)
    w2 = rho_ref.weights_int(cname, xis[:2], U[:2], d)
    assert not set(w3) & set(w2)
    masked = rho_ref.weights_int(cname, xis, U, d, [1, 1, 0])
    assert masked[2] == 0 and not set(masked[:2]) & set(w3) and not set(masked[:2]) & set(w2)


@pytest.mark.parametrize("cname", CURVES)
def test_an_instance_that_is_not_live_influences_nothing(cname):
    xis, U, d, live, _ = fixture_case(cname, "k5_lg3_live")
    base = rho_ref.weights_int(cname, xis, U, d, live)
    x2, U2 = xis.copy(), U.copy()
    for i in (1, 4):  # the two dead instances: every word of U and of the xi row
        U2[i] ^= np.uint64(0x5555)
        x2[i] ^= np.uint64(0x3333)
    assert rho_ref.weights_int(cname, x2, U2, d, live) == base


@pytest.mark.parametrize("cname", CURVES)
def test_one_changed_word_of_a_live_instance_changes_every_live_weight(cname):
    k, lg = 3, 2
    xis = np.ascontiguousarray(G[f"{cname}_k3_lg3_xis"][:, :lg + 1])
    U = G[f"{cname}_k3_lg3_U"]
    live = [1, 0, 1]
    base = rho_ref.weights_int(cname, xis, U, 3, live)
    for i in (0, 2):
        for word in range(8):
            U2 = U.copy()
            U2[i, word] ^= np.uint64(1)
            got = rho_ref.weights_int(cname, xis, U2, 3, live)
            assert got[1] == 0 and got[0] != base[0] and got[2] != base[2], (i, "U", word)
        for j in range(lg + 1):
            for word in range(4):
                x2 = xis.copy()
                x2[i, j, word] ^= np.uint64(1)
                got = rho_ref.weights_int(cname, x2, U, 3, live)
                if j == 0:  # xi_0 is not read by the decider and is not hashed
                    assert got == base, (i, word)
                else:
                    assert got[1] == 0 and got[0] != base[0] and got[2] != base[2], (i, j, word)
