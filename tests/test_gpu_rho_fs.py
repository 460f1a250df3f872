"""GPU tests of the derived decider weights (halo_amd/csrc/decide_rho.hip behind halo_pcdl_decide_rho, its _dev form
and, with the tuning key decide_rho_fs = 1, a NULL rho of halo_pcdl_decide_batch, halo_pcdl_decide_bisect_dev,
halo_pcdl_check_fs_batch and halo_plonk_verify_batch; rhos="fs" in the Python layer).  All bit-exact.

The weights are compared with tests/rho_ref.py over the CPU oracle's Poseidon; every expected verdict comes from the
CPU oracle (test_gpu_decider's oracle_verdict / oracle_code, tests/plonk_ref.py), never from the library's exact mode.

  * halo_pcdl_decide_rho and _dev equal rho_ref: both curves, lg n = 0, 1, 3, 10, k = 1, 2, 3, 64, 65 (and 257 at
    lg n = 3): odd promotion at several levels, more than one block, both lane layouts (poseidon_lanes pinned to 1
    and to 3), with and without a live mask (the rows of the masked instances differ from what the reference was
    given), the _dev output pre-filled so that an unwritten entry shows;
  * with the key at 1, decide_batch(rhos="fs") gives the oracle's verdicts for valid batches and for the four damages
    of test_gpu_decider at the first and the last instance: both curves, lg n = 2, 10, k = 2, 3, 65, through the
    host form, the _dev form (and its `combined` byte), bisect=True and halo_pcdl_decide_bisect_dev with a NULL rho;
    the _dev form agrees with a call that passes decide_rho's output as the caller's rho;
  * the structure by halo_profile_read: a valid batch is one decide_msm stage and one decide_rho stage; with the
    key at 0 a NULL rho is exact mode, one decide_msm stage per group and no decide_rho stage;
  * pcdl.check_batch / check_fs_codes / check_bytes(rhos="fs") on the committed openings of tests/golden/transcript.npz
    and plonk.verify_batch(rhos="fs") on the chains of tests/golden/plonk_proofs.npz give the codes of rhos=None, a
    tampered c and a forged U among them.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import pasta as P
import plonk_ref as R
import rho_ref
from halo_amd import acc, pcdl, plonk, wire
from test_gpu_decider import (CASES, PG, case_item, decide_dev, forged_next_u, forged_u, fs, launches,  # noqa: F401
                              oracle_code, pv, random_rows, restated_verify, run_check, tampered_c, upload)
from test_gpu_decider_bisect import _batch, _wrong_verdict, damage
from test_gpu_pcdl_check import det_scalars
from test_gpu_plonk_verify import as_proof, circuit_of

pytestmark = pytest.mark.gpu
CURVES = ["pallas", "vesta"]
KINDS = ["none", "plus_g", "xi", "identity", "off_curve"]


# ---------------------------------------------------------------------------------------------
# 1. the weights
# ---------------------------------------------------------------------------------------------
def mask(k):
    """Every third instance from the second one, and the last one, are not live (k = 1: nothing is)."""
    live = [0 if i % 3 == 1 else 1 for i in range(k)]
    live[k - 1] = 0
    return live


@functools.lru_cache(maxsize=None)
def _leaves(cname, lg, kmax):
    """kmax instances (points that need not lie on the curve: they are only hashed; the third is the identity) and
    their leaves, computed once; the weights of every prefix and mask come from them."""
    xis = random_rows(7000 + lg, kmax, lg)
    Us = det_scalars(7100 + lg, 2 * kmax).reshape(kmax, 8)
    if kmax > 2:
        Us[2] = 0
    return xis, Us, [rho_ref.leaf(cname, Us[i], xis[i]) for i in range(kmax)]


def rho_dev(hal, cname, d, xis, Us, live=None):
    """halo_pcdl_decide_rho_dev over torch buffers on the current stream, the output pre-filled."""
    import torch
    k = len(Us)

    def dev(a, dtype=np.int64):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()

    d_x, d_U = dev(xis), dev(Us)
    d_l = dev(np.asarray(live, dtype=np.uint8), np.uint8) if live is not None else None
    d_out = torch.full((k, 4), 0x7777777777777777, dtype=torch.int64, device="cuda")
    hal.check(hal.load().halo_pcdl_decide_rho_dev(
        hal.CURVES[cname], d, k, d_x.data_ptr(), d_U.data_ptr(), d_l.data_ptr() if live is not None else None,
        d_out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("lg", [0, 1, 3, 10])
@pytest.mark.parametrize("cname", CURVES)
def test_decide_rho_equals_the_restated_derivation(fs, cname, lg):
    ks = [1, 2, 3, 21, 22, 64, 65] + ([257] if lg == 3 else [])
    xis, Us, leaves = _leaves(cname, lg, max(ks))
    d = (1 << lg) - 1
    for k in ks:
        for live in (None, mask(k)):
            on = [1] * k if live is None else live
            want = rho_ref.to_ark(cname, rho_ref.weights_from_leaves(cname, [x if o else None for x, o in zip(leaves[:k], on)], d))
            x, U = xis[:k].copy(), Us[:k].copy()
            for i in range(k):
                if not on[i]:  # the reference never saw these rows; they stay below the modulus for the host form
                    x[i, :, 0] ^= np.uint64(0x5555)
                    U[i, 0] ^= np.uint64(0x3333)
            for lanes in (1, 3):
                with fs.tuning(poseidon_lanes=lanes):
                    got = pcdl.decide_rho(x, U, d, live=live, curve=cname)
                    got_dev = rho_dev(fs, cname, d, x, U, live=live)
                assert np.array_equal(got, want), (k, live is not None, lanes, "host")
                assert np.array_equal(got_dev, want), (k, live is not None, lanes, "dev")


def test_decide_rho_at_the_fixture(fs):
    """The committed fixture, whose points lie on the curve, through the device."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rho_fs.npz"))
    for cname in CURVES:
        for case, lg in (("k1_lg0", 0), ("k2_lg1", 1), ("k3_lg3", 3), ("k5_lg3", 3), ("k5_lg3_live", 3)):
            live = G[f"{cname}_{case}_live"].tolist() if case.endswith("live") else None
            got = pcdl.decide_rho(G[f"{cname}_{case}_xis"], G[f"{cname}_{case}_U"], (1 << lg) - 1, live=live, curve=cname)
            assert np.array_equal(got, G[f"{cname}_{case}_rho"]), (cname, case)
    assert pcdl.decide_rho(np.zeros((0, 4, 4), dtype=np.uint64), np.zeros((0, 8), dtype=np.uint64), 7).shape == (0, 4)


# ---------------------------------------------------------------------------------------------
# 2. the decider under derived weights
# ---------------------------------------------------------------------------------------------
def bisect_dev_null(hal, cname, d, xis, Us):
    """halo_pcdl_decide_bisect_dev with a NULL d_rho over torch buffers on the current stream: the k verdicts."""
    import torch
    k = len(Us)
    d_x = torch.from_numpy(np.ascontiguousarray(xis).view(np.int64)).cuda()
    d_U = torch.from_numpy(np.ascontiguousarray(Us).view(np.int64)).cuda()
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    hal.check(hal.load().halo_pcdl_decide_bisect_dev(hal.CURVES[cname], d, k, d_x.data_ptr(), d_U.data_ptr(), None, None,
                                                     d_ok.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().tolist()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lg", [2, 10])
@pytest.mark.parametrize("cname", CURVES)
def test_derived_weights_give_the_oracles_verdicts(fs, golden, corc, cname, lg, kind):
    n = 1 << lg
    upload(corc, golden, cname, n)
    gs, xis, Us = _batch(corc, cname, lg)
    for k in (2, 3, 65):
        for i in ((None,) if kind == "none" else (0, k - 1)):
            x, U, exp = xis[:k], Us[:k], [1] * k
            if i is not None:
                x, U = damage(cname, gs, x, U, i, kind)
                exp[i] = _wrong_verdict(corc, cname, lg, i, kind)
                assert exp[i] == 0
            good = int(i is None)
            assert pcdl.decide_batch(x, U, n - 1, rhos="fs", curve=cname).tolist() == exp, (k, i, "host")
            assert pcdl.decide_batch(x, U, n - 1, rhos="fs", curve=cname, bisect=True).tolist() == exp, (k, i, "bisect")
            with fs.deriving(True):
                assert bisect_dev_null(fs, cname, n - 1, x, U) == exp, (k, i, "bisect_dev")
                got = decide_dev(fs, cname, n - 1, x, U)
            assert got == ([good] * k, good), (k, i, "dev")  # the _dev form never falls back
            own = pcdl.decide_rho(x, U, n - 1, curve=cname)
            assert decide_dev(fs, cname, n - 1, x, U, rho=own) == got, (k, i, "the caller's rho = decide_rho's")
    assert fs.get_tuning("decide_rho_fs") == 0 and fs.get_tuning("decide_bisect") == 0


def test_live_mask_and_k_1_under_the_key(fs, golden, corc):
    upload(corc, golden, "pallas", 1 << 10)
    gs, xis, Us = _batch(corc, "pallas", 10)
    x, U = damage("pallas", gs, xis[:8], Us[:8], 3, "plus_g")
    live = [1, 1, 1, 0, 1, 1, 0, 1]  # the damaged instance and a good one are skipped
    assert pcdl.decide_batch(x, U, 1023, rhos="fs", live=live, curve="pallas").tolist() == live
    with fs.deriving(True):
        assert decide_dev(fs, "pallas", 1023, x, U, live=live) == (live, 1)
        # k = 1 stays in exact mode: `combined` is not written
        assert decide_dev(fs, "pallas", 1023, x[3:4], U[3:4]) == ([0], 7)
        assert decide_dev(fs, "pallas", 1023, x[:1], U[:1]) == ([1], 7)
    own = pcdl.decide_rho(x, U, 1023, live=live, curve="pallas")
    assert [bool(r.any()) for r in own] == [bool(b) for b in live]
    assert decide_dev(fs, "pallas", 1023, x, U, live=live, rho=own) == (live, 1)


def test_structure_one_msm_stage_and_one_rho_stage(fs, golden, corc):
    upload(corc, golden, "pallas", 1 << 10)
    gs, xis, Us = _batch(corc, "pallas", 10)
    x, U = xis[:8], Us[:8]
    L = fs.load()
    fs.check(L.halo_profile_enable(1))
    try:
        fs.check(L.halo_profile_reset())
        assert pcdl.decide_batch(x, U, 1023, rhos="fs", curve="pallas").tolist() == [1] * 8
        assert launches(fs, "decide_msm") == 1 and launches(fs, "decide_rho") == 1 and launches(fs, "hpoly_rows") == 0
        assert launches(fs, "rho_leaves") == 1 and launches(fs, "rho_level") == 3 and launches(fs, "rho_weights") == 1
        fs.check(L.halo_profile_reset())
        with fs.deriving(True):
            assert decide_dev(fs, "pallas", 1023, x, U) == ([1] * 8, 1)
        assert launches(fs, "decide_msm") == 1 and launches(fs, "decide_rho") == 1
        # a damaged batch: the host form's exact rerun derives nothing again
        _, bad = damage("pallas", gs, x, U, 5, "plus_g")
        fs.check(L.halo_profile_reset())
        assert pcdl.decide_batch(x, bad, 1023, rhos="fs", curve="pallas").tolist() == [1, 1, 1, 1, 1, 0, 1, 1]
        assert launches(fs, "decide_msm") == 2 and launches(fs, "decide_rho") == 1 and launches(fs, "hpoly_rows") == 1
        # the key at 0: a NULL rho is exact mode, one stage per group and no derivation
        fs.check(L.halo_profile_reset())
        assert fs.get_tuning("decide_rho_fs") == 0
        with fs.tuning(decide_group_scalars=3 << 10):
            assert pcdl.decide_batch(x, U, 1023, curve="pallas").tolist() == [1] * 8
            assert launches(fs, "decide_msm") == 3 and launches(fs, "decide_rho") == 0 and launches(fs, "hpoly_rows") == 3
            fs.check(L.halo_profile_reset())
            assert decide_dev(fs, "pallas", 1023, x, U) == ([1] * 8, 7)
        assert launches(fs, "decide_msm") == 3 and launches(fs, "decide_rho") == 0
    finally:
        fs.check(L.halo_profile_enable(0))
        fs.check(L.halo_profile_reset())


# ---------------------------------------------------------------------------------------------
# 3. pcdl::check and PlonkProof::verify
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES)
def test_check_fs_codes_on_the_committed_openings_under_derived_weights(fs, golden, corc, key):
    cname, d, item = case_item(golden, corc, key)
    bad_c, forged = tampered_c(cname, item), forged_u(cname, golden, d, item)
    assert [oracle_code(corc, cname, golden, d, q) for q in (item, bad_c, forged)] == [0, 1, 2]
    for batch, exp in (([item, item, item], [0, 0, 0]), ([item, bad_c, item], [0, 1, 0]), ([forged, item, item], [2, 0, 0]),
                       ([item, forged, bad_c], [0, 2, 1])):
        assert run_check(cname, d, batch) == exp
        assert run_check(cname, d, batch, rho="fs") == exp


def test_python_layer(fs, golden, corc):
    """pcdl.check_batch, acc.decider_batch and pcdl.check_bytes over two degree bounds: each d derives its own weights."""
    insts = []
    for key in ("open_pallas_n16_plain", "open_pallas_n64_hiding"):  # the longer SRS is uploaded last
        cname, d, item = case_item(golden, corc, key)
        insts += [pcdl.Instance(item[0], d, item[1], item[2], item[3])]
    good = [insts[0], insts[1], insts[0], insts[1]]
    with_c, with_u = list(good), list(good)
    q = tampered_c("pallas", (good[2].C, good[2].z, good[2].v, good[2].pi))
    with_c[2] = good[2]._replace(pi=q[3])
    q = forged_u("pallas", golden, 63, (good[1].C, good[1].z, good[1].v, good[1].pi))
    with_u[1] = good[1]._replace(pi=q[3])
    for batch, exp in ((good, [0, 0, 0, 0]), (with_c, [0, 0, 1, 0]), (with_u, [0, 2, 0, 0])):
        assert pcdl.check_batch(batch, curve="pallas", verdicts=True).tolist() == exp
        assert pcdl.check_batch(batch, rhos="fs", curve="pallas", verdicts=True).tolist() == exp
        assert pcdl.check_batch(batch, rhos="fs", curve="pallas", verdicts=True, bisect=True).tolist() == exp
        buf = wire.encode_instances(batch, curve="pallas")
        assert pcdl.check_bytes(buf, curve="pallas", verdicts=True).tolist() == exp
        assert pcdl.check_bytes(buf, rhos="fs", curve="pallas", verdicts=True).tolist() == exp
        assert pcdl.check_bytes(buf, rhos="fs", curve="pallas", verdicts=True, bisect=True).tolist() == exp
    acc.decider_batch(good, rhos="fs", curve="pallas")
    with pytest.raises(pcdl.CheckFailed, match="instance 1") as e:
        acc.decider_batch(with_u, rhos="fs", curve="pallas")
    assert e.value.index == 1 and e.value.msg == pcdl.DECIDER_MSG
    with pytest.raises(ValueError, match="'fs'"):
        pcdl.check_batch(good, rhos="random", curve="pallas")
    assert fs.get_tuning("decide_rho_fs") == 0


@pytest.mark.parametrize("key", sorted(R.CHAINS))
def test_plonk_verify_batch_on_the_committed_chains(pv, golden, key):
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(PG, key)
    circuit = circuit_of(cname, rows, C_qs)
    bad_c, forged = R.tamper(recs[0], "next_pi_c", m), forged_next_u(cname, rows, golden, recs[1])
    for batch in ([recs[0], recs[1]], [recs[0], recs[1], bad_c], [recs[0], forged, recs[1]], [forged, bad_c, recs[0], recs[1]]):
        exp = [restated_verify(cname, rows, C_qs, golden, r) for r in batch]
        trio = [as_proof(r, rows) for r in batch]
        args = (circuit, [t[1] for t in trio], [t[2] for t in trio], [t[0] for t in trio])
        assert plonk.verify_batch(*args, curve=cname).tolist() == exp
        assert plonk.verify_batch(*args, rhos="fs", curve=cname).tolist() == exp
        assert plonk.verify_batch(*args, rhos="fs", curve=cname, bisect=True).tolist() == exp
    assert {plonk.DECIDER_SUCCINCT, plonk.DECIDER, plonk.ACCEPT} == set(exp)
    assert pv.get_tuning("decide_rho_fs") == 0
