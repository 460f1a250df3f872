"""GPU tests of the bisecting Schnorr batch (halo_amd/csrc/schnorr_bisect.hip behind halo_schnorr_verify_bisect_dev,
halo_schnorr_verify_combined under the tuning key schnorr_bisect = 1 and schnorr.verify_batch(bisect=True)): a rejected
combined batch resolved per item by halving its failing parts.  Expected verdicts always come from the CPU restatement
of the reference (tests/schnorr_ref.py, memoised); the exact call (verify_batch(rhos=None)) must agree as well.  Both
curves.  Items are drawn from the small pool of tests/schnorr_combined_ref.signature_pool, so a large k costs the
oracle nothing.  Unless a test says otherwise the keys are schnorr_bisect_leaf = 1, schnorr_bisect_pass_items = 1: the
full descent, down to single items, with no ladder."""
import ctypes
import os

import numpy as np
import pytest

import schnorr_bisect_cases as C

pytestmark = pytest.mark.gpu

CURVES = ["pallas", "vesta"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
# k_sig_t scans blocks of 256 items and k_sig_scan_totals, one block of 256 threads, scans their totals 256 at a time:
# 257 items make two totals, 65 537 make 257, so that the scan of the totals loops twice and carries.
SCAN_LOOPS_TWICE = 256 * 256 + 1


@pytest.fixture(scope="module")
def sch(hal):
    """halo_amd.schnorr with the reference's Poseidon constants installed for both fields."""
    from halo_amd import schnorr
    g = np.load(GOLDEN)
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    return schnorr


@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(cname):
        if cname not in cache:
            cache[cname] = C.variants(cname)
        return cache[cname]
    return get


def both_host_forms(hal, sch, cname, arrs, rhos):
    """The host form with the key set and verify_batch(bisect=True): the two must agree; -> (verdicts, combined)."""
    with hal.tuning(schnorr_bisect=1):
        a = sch.verify_batch(*arrs, cname, rhos=rhos, return_combined=True)
    b = sch.verify_batch(*arrs, cname, rhos=rhos, return_combined=True, bisect=True)
    assert hal.get_tuning("schnorr_bisect") == 0
    assert a[0].dtype == np.uint8 and a[1] == b[1] and np.array_equal(a[0], b[0])
    return a


@pytest.mark.parametrize("wrong", ["s_plus_1", "altered_msg", "other_pk", "other_R"])
@pytest.mark.parametrize("cname", CURVES)
def test_one_wrong_item_at_every_position(hal, sch, data, cname, wrong):
    it, at = data(cname)
    with hal.tuning(**C.FULL):
        for k in (2, 3, 5, 8, 17, 257):
            for pos in (range(k) if k < 257 else (0, 127, 128, 255, 256)):
                idx = np.arange(k) % 6
                idx[pos] = at[wrong]
                arrs, exp = it.take(idx)
                assert exp.sum() == k - 1 and exp[pos] == 0
                got, comb = both_host_forms(hal, sch, cname, arrs, C.rand_rho(k, 1000 * k + pos))
                assert comb == 0 and np.array_equal(got, exp), (k, pos)
                assert np.array_equal(sch.verify_batch(*arrs, cname), exp), (k, pos)


def test_every_subset_of_six(hal, sch, data):
    cname = "pallas"
    it, at = data(cname)
    kinds = [at[n] for n in ("s_plus_1", "altered_msg", "other_pk", "other_R")]
    with hal.tuning(**C.FULL):
        for mask in range(1, 64):
            idx = np.arange(6)
            for i in range(6):
                if (mask >> i) & 1:
                    idx[i] = kinds[(i + mask) % 4]
            arrs, exp = it.take(idx)
            assert [int(v) for v in exp] == [1 - ((mask >> i) & 1) for i in range(6)]
            got, comb = both_host_forms(hal, sch, cname, arrs, C.rand_rho(6, mask))
            assert comb == 0 and np.array_equal(got, exp), mask
            dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(6, 64 + mask))
            assert dcomb == 0 and np.array_equal(dok, exp), mask
        arrs, exp = it.take(np.arange(6))  # the empty subset: nothing to descend into
        got, comb = both_host_forms(hal, sch, cname, arrs, C.rand_rho(6, 0))
        assert comb == 1 and got.all()


def test_random_subsets_of_thirty_three(hal, sch, data):
    cname = "vesta"
    it, at = data(cname)
    kinds = np.array([at[n] for n in ("s_plus_1", "altered_msg", "other_pk", "other_R")])
    rng = np.random.default_rng(33)
    with hal.tuning(**C.FULL):
        for case, density in enumerate((0.03, 0.1, 0.25, 0.5, 0.5, 0.9)):
            idx = np.arange(33) % 6
            bad = rng.random(33) < density
            bad[rng.integers(33)] = True
            idx[bad] = kinds[rng.integers(4, size=int(bad.sum()))]
            arrs, exp = it.take(idx)
            assert np.array_equal(exp, (~bad).astype(np.uint8))
            got, comb = both_host_forms(hal, sch, cname, arrs, C.rand_rho(33, case))
            assert comb == 0 and np.array_equal(got, exp), case
            assert np.array_equal(sch.verify_batch(*arrs, cname), exp)


@pytest.mark.parametrize("cname", CURVES)
def test_all_sixteen_wrong(hal, sch, data, cname):
    it, at = data(cname)
    kinds = [at[n] for n in ("s_plus_1", "altered_msg", "other_pk", "other_R")]
    arrs, exp = it.take([kinds[i % 4] for i in range(16)])
    assert not exp.any()
    with hal.tuning(**C.FULL), C.Launches(hal) as n:
        dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(16, 16))
        seen = n()
    assert dcomb == 0 and not dok.any()
    assert seen["sig_split"] == 4 and seen["sig_bisect_msm"] == 4 and seen["sig_bisect_ladder"] == 0 and seen["sig_t"] == 1
    with hal.tuning(**C.FULL):
        got, comb = both_host_forms(hal, sch, cname, arrs, "fs")
    assert comb == 0 and not got.any()


@pytest.mark.parametrize("cname", CURVES)
def test_the_scan(hal, sch, data, cname):
    """A wrong prefix sum gives a wrong G part to some left half, which then fails with valid items in it: equality of
    the verdicts pins every P[mid] - P[lo] the descent reads."""
    it, at = data(cname)
    with hal.tuning(**C.FULL):
        for k, wrong in ((255, (254,)), (256, (255,)), (256, (0, 128)), (257, (256,)), (257, (255,)),
                         (SCAN_LOOPS_TWICE, (SCAN_LOOPS_TWICE - 1,)), (SCAN_LOOPS_TWICE, (256,))):
            idx = np.arange(k) % 6
            idx[list(wrong)] = at["s_plus_1"]
            arrs, exp = it.take(idx)
            assert exp.sum() == k - len(wrong)
            dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(k, k))
            assert dcomb == 0 and np.array_equal(dok, exp), (k, wrong)
            if k == SCAN_LOOPS_TWICE and wrong == (256,):
                got, comb = sch.verify_batch(*arrs, cname, rhos="fs", return_combined=True, bisect=True)
                assert comb == 0 and np.array_equal(got, exp)


@pytest.mark.parametrize("cname", CURVES)
def test_items_that_are_not_live_inside_failing_nodes(hal, sch, data, cname):
    it, at = data(cname)
    a = at
    batches = [
        # a left half all dead: an MSM of (0, 0) bases and zero scalars, a zero G part; that child passes
        [a["pk_off_curve"], a["R_off_curve"], 0, a["s_plus_1"]],
        [a["dead_and_wrong"], a["pk_off_curve"], a["R_off_curve"], a["dead_and_wrong"], 1, 2, a["other_R"], 3],
        # dead and wrong next to a wrong live item: the dead one weighs nothing, so its half fails on the live one alone
        [0, a["dead_and_wrong"], a["s_plus_1"], 1, 2],
        [a["dead_and_wrong"], a["altered_msg"]],
        # identities and R = pk among the terms of failing nodes
        [a["pk_identity"], a["R_identity"], a["R_equals_pk"], a["s_plus_1"], 0, a["pk_off_curve"], 1, a["R_identity"]],
        [a["pk_identity"], a["other_pk"], a["R_identity"], a["R_equals_pk"], a["R_equals_pk"], a["other_R"], a["pk_identity"]],
    ]
    with hal.tuning(**C.FULL):
        for idx in batches:
            arrs, exp = it.take(idx)
            dead = [j for j, i in enumerate(idx) if i in (a["pk_off_curve"], a["R_off_curve"], a["dead_and_wrong"])]
            live_wrong = [j for j in range(len(idx)) if not exp[j] and j not in dead]
            assert live_wrong and not exp[dead].any()
            for rhos in (C.rand_rho(len(idx), len(idx)), "fs"):
                got, comb = both_host_forms(hal, sch, cname, arrs, rhos)
                assert comb == 0 and np.array_equal(got, exp), idx
            dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(len(idx), 5))
            assert dcomb == 0 and np.array_equal(dok, exp), idx
            assert np.array_equal(sch.verify_batch(*arrs, cname), exp)


@pytest.mark.parametrize("cname", CURVES)
def test_right_defect_is_node_minus_left_under_the_callers_weights(hal, sch, data, cname):
    """s_0 + x, s_1 - x under weights (1, 1, ...) known in advance cancel inside the left half [0, 2): the root fails on
    item 3 alone, the left half passes and its two items are ACCEPTED -- the documented contract, and the proof that the
    right half's defect is the node's minus the left's under the weights given.  Under (1, 2, ...) all three are found."""
    it, at = data(cname)
    arrs, exp = it.take([at["plus_x"], at["minus_x"], 2, at["s_plus_1"]])
    assert exp.tolist() == [0, 0, 1, 0]
    r = C.rand_rho(2, 7)
    one_one = np.concatenate([C.small_rho(cname, [1, 1]), r])
    one_two = np.concatenate([C.small_rho(cname, [1, 2]), r])
    with hal.tuning(**C.FULL):
        for form in ("host", "dev"):
            run = (lambda rho: both_host_forms(hal, sch, cname, arrs, rho)) if form == "host" else \
                (lambda rho: C.bisect_dev(hal, cname, arrs, rho))
            got, comb = run(one_one)
            assert comb == 0 and got.tolist() == [1, 1, 1, 0], form
            got, comb = run(one_two)
            assert comb == 0 and got.tolist() == [0, 0, 1, 0], form
    assert sch.verify_batch(*arrs, cname).tolist() == [0, 0, 1, 0]
    got, comb = sch.verify_batch(*arrs, cname, rhos=one_one, return_combined=True)  # without the descent: every ladder
    assert comb == 0 and got.tolist() == [0, 0, 1, 0]


@pytest.mark.parametrize("cname", CURVES)
def test_leaf_and_budget_paths(hal, sch, data, cname):
    it, at = data(cname)
    # L = 4, c = 1 at k = 17: [0, 4) and [8, 12) are failing nodes of four items, each resolved by its own ladder
    idx = np.arange(17) % 6
    idx[[2, 9]] = at["s_plus_1"], at["other_pk"]
    arrs, exp = it.take(idx)
    with hal.tuning(schnorr_bisect_leaf=4, schnorr_bisect_pass_items=1), C.Launches(hal) as n:
        dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(17, 17))
        seen = n()
    assert dcomb == 0 and np.array_equal(dok, exp)
    assert seen["sig_split"] == 2 and seen["sig_bisect_ladder"] == 2
    # k = 64, c = 16, L = 1, a wrong item in every quarter: 1 + 2 passes, then (3 + 4) 16 > 64: four slice ladders
    idx = np.arange(64) % 6
    idx[[3, 20, 40, 63]] = at["s_plus_1"], at["altered_msg"], at["other_pk"], at["other_R"]
    idx[[5, 50]] = at["pk_off_curve"], at["dead_and_wrong"]
    arrs, exp = it.take(idx)
    assert exp.sum() == 64 - 6
    with hal.tuning(schnorr_bisect_leaf=1, schnorr_bisect_pass_items=16):
        with C.Launches(hal) as n:
            dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(64, 64))
            seen = n()
        assert dcomb == 0 and np.array_equal(dok, exp)
        assert seen["sig_split"] == 2 and seen["sig_bisect_ladder"] == 4
        got, comb = both_host_forms(hal, sch, cname, arrs, "fs")
        assert comb == 0 and np.array_equal(got, exp)
    # k < c: the root goes straight to the ladder, no pass and no scan
    with hal.tuning(schnorr_bisect_leaf=1, schnorr_bisect_pass_items=65), C.Launches(hal) as n:
        dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(64, 65))
        seen = n()
    assert dcomb == 0 and np.array_equal(dok, exp)
    assert seen["sig_split"] == 0 and seen["sig_t"] == 0 and seen["sig_bisect_ladder"] == 1


@pytest.mark.parametrize("cname", CURVES)
def test_default_keys_at_seventy_thousand(hal, sch, data, cname):
    it, at = data(cname)
    k = 70000
    idx = np.arange(k) % 6
    idx[41234] = at["s_plus_1"]
    arrs, exp = it.take(idx)
    assert exp.sum() == k - 1
    assert hal.get_tuning("schnorr_bisect_leaf") == 2 * hal.get_tuning("schnorr_bisect_pass_items")
    got, comb = both_host_forms(hal, sch, cname, arrs, C.rand_rho(k, k))
    assert comb == 0 and np.array_equal(got, exp)
    dok, dcomb = C.bisect_dev(hal, cname, arrs, None)
    assert dcomb == 0 and np.array_equal(dok, exp)


@pytest.mark.parametrize("cname", CURVES)
def test_derived_weights_twice(hal, sch, data, cname):
    it, at = data(cname)
    idx = np.arange(21) % 6
    idx[[4, 13, 20]] = at["s_plus_1"], at["R_off_curve"], at["other_R"]
    arrs, exp = it.take(idx)
    with hal.tuning(**C.FULL):
        a = sch.verify_batch(*arrs, cname, rhos="fs", return_combined=True, bisect=True)
        b = sch.verify_batch(*arrs, cname, rhos="fs", return_combined=True, bisect=True)
        assert a[1] == b[1] == 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[0], exp)
        dok, dcomb = C.bisect_dev(hal, cname, arrs, None)
        assert dcomb == 0 and np.array_equal(dok, exp)
    assert np.array_equal(sch.verify_batch(*arrs, cname, rhos="fs"), exp)  # and without the descent


@pytest.mark.parametrize("cname", CURVES)
def test_dev_form_bad_weights(hal, sch, data, cname):
    """The _dev form cannot refuse on the host: a live item whose rho is zero or not below the modulus gives combined = 0
    and all zeros, with no descent; the rho of an item that is not live is not read."""
    it, at = data(cname)
    arrs, exp = it.take([0, 1, at["pk_off_curve"], at["s_plus_1"], 2])
    rho = C.rand_rho(5, 6)
    rho[2] = 0  # not live: not read, neither by the pass nor by the prefix sums
    with hal.tuning(**C.FULL):
        dok, dcomb = C.bisect_dev(hal, cname, arrs, rho)
        assert dcomb == 0 and np.array_equal(dok, exp)
        for bad in (0, 0xFFFFFFFFFFFFFFFF):
            r = rho.copy()
            r[1] = bad
            with C.Launches(hal) as n:
                dok, dcomb = C.bisect_dev(hal, cname, arrs, r)
                seen = n()
            assert dcomb == 0 and not dok.any()
            assert not any(seen.values())


def test_dev_form_on_a_side_stream_then_the_exact_call(hal, sch, data):
    """Inputs resident, a non-default stream, and the exact _dev call right behind on the same stream: both use the
    challenges' buffer, the stream orders them."""
    import torch
    cname = "pallas"
    it, at = data(cname)
    k = 300
    idx = np.arange(k) % 6
    idx[::7] = at["s_plus_1"]
    arrs, exp = it.take(idx)
    idx2 = np.arange(k)[::-1] % 6
    idx2[5::11] = at["other_pk"]
    arrs2, exp2 = it.take(idx2)
    side = torch.cuda.Stream()
    d = [C.cuda(x) for x in arrs]
    d2 = [C.cuda(x) for x in arrs2]
    d_rho = C.cuda(C.rand_rho(k, 8))
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_ok2 = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_comb = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = hal.load()
    curve = hal.CURVES[cname]
    sp = ctypes.c_void_p(side.cuda_stream)
    with hal.tuning(**C.FULL):
        hal.check(L.halo_schnorr_verify_bisect_dev(curve, *[C.dev(t) for t in d], 10, k, C.dev(d_rho), C.dev(d_ok), C.dev(d_comb), sp))
    hal.check(L.halo_schnorr_verify_batch_dev(curve, *[C.dev(t) for t in d2], 10, k, C.dev(d_ok2), sp))
    torch.cuda.synchronize()
    assert int(d_comb.cpu()[0]) == 0 and np.array_equal(d_ok.cpu().numpy(), exp)
    assert np.array_equal(d_ok2.cpu().numpy(), exp2)


@pytest.mark.parametrize("cname", CURVES)
def test_an_accepted_batch(hal, sch, data, cname):
    it, at = data(cname)
    idx = list(np.arange(40) % 6)
    idx[7], idx[22], idx[30] = at["R_off_curve"], at["pk_identity"], at["R_equals_pk"]
    arrs, exp = it.take(idx)
    assert exp.sum() == 39
    for rhos in (C.rand_rho(40, 40), "fs"):
        plain = sch.verify_batch(*arrs, cname, rhos=rhos, return_combined=True)
        with C.Launches(hal) as n:
            got, comb = both_host_forms(hal, sch, cname, arrs, rhos)
            seen = n()
        assert comb == 1 and plain[1] == 1 and np.array_equal(got, plain[0]) and np.array_equal(got, exp)
        assert not any(seen.values())
    dok, dcomb = C.bisect_dev(hal, cname, arrs, None)
    assert dcomb == 1 and np.array_equal(dok, exp)
    arrs, exp = it.take([at["s_plus_1"]])  # a batch of one: its defect is its verdict
    got, comb = both_host_forms(hal, sch, cname, arrs, C.rand_rho(1, 1))
    assert comb == 0 and got.tolist() == [0]
    dok, dcomb = C.bisect_dev(hal, cname, arrs, C.rand_rho(1, 2))
    assert dcomb == 0 and dok.tolist() == [0]
