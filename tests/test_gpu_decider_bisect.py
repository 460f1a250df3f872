"""GPU tests of the bisecting decider (decide_bisect_device in halo_amd/csrc/decider.hip behind
halo_pcdl_decide_bisect_dev and, with the tuning key decide_bisect = 1, behind halo_pcdl_decide_batch,
halo_pcdl_check_fs_batch and halo_plonk_verify_batch; bisect=True in the Python layer).  All bit-exact.

Every expected verdict comes from the CPU oracle (pcdl_check.decider_commit_matches through test_gpu_decider's
oracle_verdict, the commitments through oracle_commit), never from the library's exact mode.

  * verdicts through decide_batch(..., rhos=..., bisect=True) and through the _dev entry point: both curves,
    lg n = 0, 1 (k = 2, 3) and 3, 10 (k = 2, 3, 5, 8, 65); wrong sets none, {0} (D(left) = D(node)), {k - 1} (D(left)
    the identity), {0, 1} (siblings), {k/2 - 1, k/2} (either side of the first split), all; damages U + G, one xi
    changed, U = (0, 0), U off the curve.  At lg n = 0 no xi is read (h = 1), so "xi" is no damage there and is left
    out; at lg n = 1 it changes xi_1, above that xi_3 (test_gpu_decider.damaged);
  * U_a + G and U_b - G in the same half: an unweighted descent would cancel them;
  * live masks; a rho that is zero or not below the modulus in the _dev form;
  * the groups of a level (decide_group_scalars) and the pipelined MSMs above msm_multi_max;
  * the structure by halo_profile_read: one MSM stage per group of failing nodes, no exact rows, no segments for an
    accepted batch, the exact rerun with the key off;
  * pcdl.check_batch(bisect=True) on the committed openings and halo_plonk_verify_batch with the key on over the
    committed chains, a forged U among them.
"""
import ctypes
import functools

import numpy as np
import pytest

import pasta as P
import plonk_ref as R
from halo_amd import pcdl, plonk
from test_gpu_decider import (PG, case_item, damaged, forged_next_u, forged_u, fs, launches, oracle_code,  # noqa: F401
                              oracle_commit, oracle_verdict, pv, random_rows, restated_verify, rhos, run_check, run_verify,
                              tampered_c, upload, _srs)
from test_gpu_pcdl_check import plus_one, unwrapped, wrapped

pytestmark = pytest.mark.gpu
CURVES = ["pallas", "vesta"]
KINDS = ["plus_g", "xi", "identity", "off_curve"]
KMAX = 65


@functools.lru_cache(maxsize=None)
def _batch(corc, cname, lg):
    """The recipe SRS of 2^lg points, 65 random xi rows and the oracle's commitments; computed once."""
    gs = _srs(corc, cname, 1 << lg)
    xis = random_rows(5000 + lg, KMAX, lg)
    return gs, xis, np.stack([oracle_commit(corc, cname, gs, row) for row in xis])


def damage(cname, gs, xis, Us, i, kind):
    lg = xis.shape[1] - 1
    if kind == "xi" and lg < 3:  # test_gpu_decider.damaged changes xi_3
        xis = xis.copy()
        xis[i, lg] = plus_one(xis[i, lg], P.CURVES[cname].scalar)
        return xis, Us.copy()
    return damaged(cname, gs, xis, Us, i, kind)


@functools.lru_cache(maxsize=None)
def _wrong_verdict(corc, cname, lg, i, kind) -> int:
    """The oracle's verdict of instance i of _batch after the damage (the damage of i does not depend on k)."""
    gs, xis, Us = _batch(corc, cname, lg)
    x, U = damage(cname, gs, xis, Us, i, kind)
    return oracle_verdict(corc, cname, gs, x[i], U[i])


def wrong_sets(k):
    sets = [(), (0,), (k - 1,), (0, 1), (k // 2 - 1, k // 2), tuple(range(k))]
    return sorted({tuple(sorted(set(s))) for s in sets if all(0 <= i < k for i in s)})


def bisect_dev(hal, cname, d, xis, Us, live=None, rho=None):
    """halo_pcdl_decide_bisect_dev over torch buffers on the current stream: the k verdicts."""
    import torch
    k = len(Us)

    def dev(a, dtype=np.int64):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()

    d_x, d_U, d_r = dev(xis), dev(Us), dev(rho)
    d_l = dev(np.asarray(live, dtype=np.uint8), np.uint8) if live is not None else None
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    hal.check(hal.load().halo_pcdl_decide_bisect_dev(
        hal.CURVES[cname], d, k, d_x.data_ptr(), d_U.data_ptr(), d_l.data_ptr() if live is not None else None,
        d_r.data_ptr(), d_ok.data_ptr(), ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().tolist()


# ---------------------------------------------------------------------------------------------
# 1. verdicts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg,kind", [(lg, kind) for lg in (0, 1, 3, 10) for kind in KINDS if (lg, kind) != (0, "xi")])
@pytest.mark.parametrize("cname", CURVES)
def test_bisect_gives_the_oracles_verdicts(hal, golden, corc, cname, lg, kind):
    n = 1 << lg
    upload(corc, golden, cname, n)
    gs, xis, Us = _batch(corc, cname, lg)
    for k in ((2, 3) if lg < 3 else (2, 3, 5, 8, 65)):
        r = rhos(100 + k, k)
        for wrong in wrong_sets(k):
            x, U = xis[:k], Us[:k]
            exp = [1] * k
            for i in wrong:
                x, U = damage(cname, gs, x, U, i, kind)
                exp[i] = _wrong_verdict(corc, cname, lg, i, kind)
                assert exp[i] == 0
            assert pcdl.decide_batch(x, U, n - 1, rhos=r, curve=cname, bisect=True).tolist() == exp, (k, wrong, "host")
            assert bisect_dev(hal, cname, n - 1, x, U, rho=r) == exp, (k, wrong, "dev")
    assert hal.get_tuning("decide_bisect") == 0


@pytest.mark.parametrize("lg", [3, 10])
@pytest.mark.parametrize("cname", CURVES)
def test_opposite_damages_in_one_half_do_not_cancel(hal, golden, corc, cname, lg):
    """U_a + G and U_b - G with a, b in the same half at every level until they part: the sum of the two unweighted
    defects is zero, the weighted one is not.  The oracle rejects both."""
    cv = P.CURVES[cname]
    n = 1 << lg
    upload(corc, golden, cname, n)
    gs, xis, Us = _batch(corc, cname, lg)
    G0 = unwrapped(cv, gs[0])
    for k, a, b in ((8, 0, 1), (8, 4, 7), (5, 2, 4), (65, 33, 64)):
        x, U = xis[:k], Us[:k].copy()
        U[a] = wrapped(cv, P.add(cv, unwrapped(cv, U[a]), G0))
        U[b] = wrapped(cv, P.add(cv, unwrapped(cv, U[b]), P.neg(cv, G0)))
        exp = [1] * k
        for i in (a, b):
            exp[i] = oracle_verdict(corc, cname, gs, x[i], U[i])
        assert exp[a] == 0 and exp[b] == 0
        r = rhos(200 + k, k)
        assert pcdl.decide_batch(x, U, n - 1, rhos=r, curve=cname, bisect=True).tolist() == exp, (k, a, b)
        assert bisect_dev(hal, cname, n - 1, x, U, rho=r) == exp, (k, a, b)


# ---------------------------------------------------------------------------------------------
# 2. live masks, weights the _dev form cannot refuse
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plus_g", "off_curve"])
@pytest.mark.parametrize("cname", CURVES)
def test_masked_out_instances_disturb_nothing(hal, golden, corc, cname, kind):
    lg, k = 10, 8
    upload(corc, golden, cname, 1 << lg)
    gs, xis, Us = _batch(corc, cname, lg)
    x, U = damage(cname, gs, xis[:k], Us[:k], 3, kind)  # 3 is wrong and masked out
    x, U = damage(cname, gs, x, U, 5, kind)             # 5 is wrong and live
    assert _wrong_verdict(corc, cname, lg, 5, kind) == 0
    live = [1, 1, 1, 0, 1, 1, 0, 1]                     # 6 is a good instance that is skipped
    exp = [1, 1, 1, 0, 1, 0, 0, 1]
    r = rhos(31, k)
    assert pcdl.decide_batch(x, U, 1023, rhos=r, live=live, curve=cname, bisect=True).tolist() == exp
    assert bisect_dev(hal, cname, 1023, x, U, live=live, rho=r) == exp
    # only masked-out instances are wrong: the root pass accepts
    x, U = damage(cname, gs, xis[:k], Us[:k], 3, kind)
    exp = [1, 1, 1, 0, 1, 1, 0, 1]
    assert pcdl.decide_batch(x, U, 1023, rhos=r, live=live, curve=cname, bisect=True).tolist() == exp
    assert bisect_dev(hal, cname, 1023, x, U, live=live, rho=r) == exp
    assert bisect_dev(hal, cname, 1023, x, U, live=[0] * k, rho=r) == [0] * k
    assert bisect_dev(hal, cname, 1023, x[3:4], U[3:4], rho=r[:1]) == [0]  # k = 1: the exact path
    assert bisect_dev(hal, cname, 1023, x[2:3], U[2:3], rho=r[:1]) == [1]


@pytest.mark.parametrize("cname", CURVES)
def test_dev_form_rejects_an_instance_with_an_unusable_weight(hal, golden, corc, cname):
    """The host forms refuse such a rho before any device work; the _dev form cannot look, so the instance is
    rejected up front, weighs nothing, and the others keep their verdicts."""
    lg, k = 10, 5
    upload(corc, golden, cname, 1 << lg)
    gs, xis, Us = _batch(corc, cname, lg)
    x, U = damage(cname, gs, xis[:k], Us[:k], 4, "plus_g")
    for bad_rho in (np.zeros(4, dtype=np.uint64), np.array(P.int_to_limbs(P.CURVES[cname].scalar), dtype=np.uint64)):
        r = rhos(41, k)
        r[1] = bad_rho
        assert bisect_dev(hal, cname, 1023, x, U, rho=r) == [1, 0, 1, 1, 0]
        assert bisect_dev(hal, cname, 1023, xis[:k], Us[:k], rho=r) == [1, 0, 1, 1, 1]


# ---------------------------------------------------------------------------------------------
# 3. the groups of a level, the pipelined MSMs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_a_level_in_two_groups(hal, golden, corc, cname):
    """decide_group_scalars = 2 n, k = 8, all wrong: the four rows of the last level take two groups."""
    lg, k = 10, 8
    upload(corc, golden, cname, 1 << lg)
    gs, xis, Us = _batch(corc, cname, lg)
    x, U = xis[:k], Us[:k]
    for i in range(k):
        x, U = damage(cname, gs, x, U, i, "plus_g")
        assert _wrong_verdict(corc, cname, lg, i, "plus_g") == 0
    one = damage(cname, gs, xis[:k], Us[:k], 6, "plus_g")
    with hal.tuning(decide_group_scalars=2 << lg):
        assert pcdl.decide_batch(x, U, 1023, rhos=rhos(51, k), curve=cname, bisect=True).tolist() == [0] * k
        assert bisect_dev(hal, cname, 1023, x, U, rho=rhos(51, k)) == [0] * k
        assert bisect_dev(hal, cname, 1023, *one, rho=rhos(51, k)) == [1, 1, 1, 1, 1, 1, 0, 1]


@pytest.mark.parametrize("cname", CURVES)
def test_pipelined_path_above_msm_multi_max(hal, golden, corc, cname):
    n = 1 << 11
    gs = upload(corc, golden, cname, n)
    xis = random_rows(3000, 3, 11)
    Us = np.stack([oracle_commit(corc, cname, gs, row) for row in xis])
    x, bad = damaged(cname, gs, xis, Us, 1, "plus_g")
    assert oracle_verdict(corc, cname, gs, x[1], bad[1]) == 0
    with hal.tuning(msm_multi_max=1 << 10):
        assert pcdl.decide_batch(xis, Us, n - 1, rhos=rhos(5, 3), curve=cname, bisect=True).tolist() == [1, 1, 1]
        assert pcdl.decide_batch(xis, bad, n - 1, rhos=rhos(5, 3), curve=cname, bisect=True).tolist() == [1, 0, 1]
        assert bisect_dev(hal, cname, n - 1, xis, bad, rho=rhos(5, 3)) == [1, 0, 1]


# ---------------------------------------------------------------------------------------------
# 4. structure
# ---------------------------------------------------------------------------------------------
def test_one_msm_stage_per_group_of_failing_nodes(hal, golden, corc):
    n, k = 1 << 12, 8
    gs = upload(corc, golden, "pallas", n)
    xis = random_rows(4000, k, 12)
    Us = np.stack([oracle_commit(corc, "pallas", gs, row) for row in xis])
    _, one = damaged("pallas", gs, xis, Us, 5, "plus_g")
    exp_one = [1, 1, 1, 1, 1, 0, 1, 1]
    every = Us
    for i in range(k):
        _, every = damaged("pallas", gs, xis, every, i, "plus_g")
    r = rhos(21, k)
    L = hal.load()
    hal.check(L.halo_profile_enable(1))

    def counts():
        return {name: launches(hal, name) for name in ("decide_msm", "hpoly_combine", "hpoly_rows", "hpoly_segments")}

    try:
        # one wrong instance: the root pass and one node per level
        hal.check(L.halo_profile_reset())
        assert pcdl.decide_batch(xis, one, n - 1, rhos=r, curve="pallas", bisect=True).tolist() == exp_one
        assert counts() == {"decide_msm": 1 + 3, "hpoly_combine": 1, "hpoly_rows": 0, "hpoly_segments": 3}
        hal.check(L.halo_profile_reset())
        assert bisect_dev(hal, "pallas", n - 1, xis, one, rho=r) == exp_one
        assert counts() == {"decide_msm": 1 + 3, "hpoly_combine": 1, "hpoly_rows": 0, "hpoly_segments": 3}
        # all wrong: 1 + 2 + 4 rows, still one group per level
        hal.check(L.halo_profile_reset())
        assert pcdl.decide_batch(xis, every, n - 1, rhos=r, curve="pallas", bisect=True).tolist() == [0] * k
        assert counts() == {"decide_msm": 1 + 3, "hpoly_combine": 1, "hpoly_rows": 0, "hpoly_segments": 3}
        # ... and two rows to a group: 1 + 1 + 1 + 2
        hal.check(L.halo_profile_reset())
        with hal.tuning(decide_group_scalars=2 * n):
            assert pcdl.decide_batch(xis, every, n - 1, rhos=r, curve="pallas", bisect=True).tolist() == [0] * k
        assert launches(hal, "decide_msm") == 1 + 1 + 1 + 2 and launches(hal, "hpoly_segments") == 4
        # an accepted batch runs nothing of the descent
        hal.check(L.halo_profile_reset())
        assert pcdl.decide_batch(xis, Us, n - 1, rhos=r, curve="pallas", bisect=True).tolist() == [1] * k
        assert counts() == {"decide_msm": 1, "hpoly_combine": 1, "hpoly_rows": 0, "hpoly_segments": 0}
        # the key off: the exact rerun, as before
        hal.check(L.halo_profile_reset())
        assert pcdl.decide_batch(xis, one, n - 1, rhos=r, curve="pallas").tolist() == exp_one
        assert counts() == {"decide_msm": 2, "hpoly_combine": 1, "hpoly_rows": 1, "hpoly_segments": 0}
    finally:
        hal.check(L.halo_profile_enable(0))
        hal.check(L.halo_profile_reset())


# ---------------------------------------------------------------------------------------------
# 5. pcdl::check and PlonkProof::verify with the key on
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_check_batch_bisect_on_the_committed_openings(fs, golden, corc, cname):
    """A mixed batch of plain and hiding openings of n = 4096 with one code 1 (c tampered) and one code 2 (the forged
    U* of test_gpu_decider's docstring): the oracle's codes, and those with the key off."""
    _, d, hiding = case_item(golden, corc, f"big_{cname}_n4096_hiding")
    _, _, plain = case_item(golden, corc, f"big_{cname}_n4096_plain")
    items = [plain, hiding, plain, hiding, plain]
    items[1] = tampered_c(cname, items[1])
    items[3] = forged_u(cname, golden, d, items[3])
    exp = [oracle_code(corc, cname, golden, d, q) for q in items]
    assert exp == [0, 1, 0, 2, 0]
    r = rhos(61, len(items))
    insts = [pcdl.Instance(C, d, z, v, pi) for C, z, v, pi in items]
    assert pcdl.check_batch(insts, rhos=r, curve=cname, verdicts=True, bisect=True).tolist() == exp
    assert pcdl.check_batch(insts, rhos=r, curve=cname, verdicts=True).tolist() == exp
    with fs.tuning(decide_bisect=1):
        assert run_check(cname, d, items, rho=r) == exp
        assert run_check(cname, d, [items[0], items[2]], rho=r[:2]) == [0, 0]
    with pytest.raises(pcdl.CheckFailed, match="instance 1") as e:
        pcdl.check_batch(insts, rhos=r, curve=cname, bisect=True)
    assert e.value.msg == pcdl.SUCCINCT_MSG


@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_plonk_verify_batch_bisect(pv, golden, key):
    """One proof with a forged acc_next.pi.U among good ones and one that fails its succinct check: 10 for the
    forgery, 0 for the good ones, equal to tests/plonk_ref.py's verify."""
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(PG, key)
    items = [recs[0], recs[1], forged_next_u(cname, rows, golden, recs[0]), recs[1], R.tamper(recs[0], "next_pi_c", m), recs[0],
             recs[1]]
    exp = [restated_verify(cname, rows, C_qs, golden, r) for r in items]
    assert exp == [0, 0, plonk.DECIDER, 0, plonk.DECIDER_SUCCINCT, 0, 0]
    r = rhos(95, len(items))
    with pv.tuning(decide_bisect=1):
        assert run_verify(pv, cname, rows, C_qs, items, rho=r) == exp
        assert run_verify(pv, cname, rows, C_qs, recs, rho=r[:2]) == [0, 0]
    assert run_verify(pv, cname, rows, C_qs, items, rho=r) == exp  # the key off
    from test_gpu_plonk_verify import as_proof, circuit_of
    trio = [as_proof(q, rows) for q in items]
    got = plonk.verify_batch(circuit_of(cname, rows, C_qs), [t[1] for t in trio], [t[2] for t in trio], [t[0] for t in trio],
                             rhos=r, curve=cname, bisect=True)
    assert got.tolist() == exp
