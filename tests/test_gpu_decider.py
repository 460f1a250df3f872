"""GPU tests of the batched decider (halo_amd/csrc/decider.hip behind halo_pcdl_decide_batch, halo_pcdl_check_fs_batch
and their _dev forms; halo_amd.pcdl.decide_batch / check_batch, halo_amd.acc.decider_batch).  All bit-exact.

Expected values come from the CPU oracle alone: the commitment of an instance is corc.msm over pcdl_check.h_coeffs,
a verdict is pcdl_check.decider_commit_matches, a succinct verdict pcdl_check.succinct_check under the oracle's
Poseidon transcript.  The exact mode compares canonical affine words on the device, so "U' equals the oracle's"
is tested by handing the oracle's commitment in as U and asking for verdict 1, and by verdict 0 for U + G.

  * both curves, lg n = 0 (h = 1), 1 (empty low table), 2, 3 (odd split), 10, 12; k = 1, 2, 3, 65; random xi rows
    and one with a zero xi; exact and combined mode;
  * four damages (U + G, one xi changed, U = (0, 0), U off the curve) at the first and last instance and on both
    sides of a group boundary (three groups of k = 5 at n = 2^10): both modes give the oracle's verdicts;
  * the pipelined path above msm_multi_max at a small size;
  * combined mode launches one MSM; a damaged batch falls back in the host form and does not in the _dev form;
  * live masks; the errors that come before any device work;
  * pcdl::check of the committed openings (tests/golden/transcript.npz): accepted, code 1 for a tampered c, code 2
    for a U that only the decider can tell from the prover's, mixed batches of 22 and 65, the _dev form, and the
    Python layer against pcdl.check_device;
  * PlonkProof::verify of the chains of tests/golden/plonk_proofs.npz (halo_plonk_verify_batch): accepted; for
    every tampering tests/plonk_ref.py knows the verify_succinct code of the same batch; code 9 for a tampered
    acc_next.pi.c, 10 for a forged acc_next.pi.U, the earlier code for a proof that fails both; mixed batches
    of 22 and 65 in both modes and the _dev form, against tests/plonk_ref.py's verify.

A U that is simply swapped for another point already fails the succinct check (its term -c U), so code 2 needs a
forgery that the succinct check accepts: no challenge depends on U or c, so for c' = 2 c the point
U* = U / 2 - (h(z) xi_0 / 2) H satisfies C_(lg n) == c' U* + c' h(z) xi_0 H.  The oracle's succinct check confirms
it before the device sees it.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import pasta as P
import pcdl_check
from halo_amd import acc, group, pcdl
from test_gpu_pcdl_check import det_scalars, fe, load_case, plus_one, unwrapped, wrapped

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "transcript.npz"))
CASES = sorted({k[:-2] for k in G.files if (k.startswith("open_") or k.startswith("big_")) and k.endswith("_C")})
CURVES = ["pallas", "vesta"]


@pytest.fixture(scope="module")
def fs(hal):
    """The reference's Poseidon constants installed for both fields."""
    from halo_amd import schnorr
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, G[f"poseidon_{f}_mds"], G[f"poseidon_{f}_rc"])
    return hal


def to_int(x, m: int) -> int:
    return P.from_mont(P.limbs_to_int(x), m)


@functools.lru_cache(maxsize=None)
def _srs(corc, cname, n):
    return corc.srs_generate(cname, n)


def upload(corc, golden, cname, n):
    """The recipe SRS of length n with the reference's (S, H) and the window-shifted copies; returns the points."""
    S, Hh = golden[f"ref_sh_{cname}"]
    gs = _srs(corc, cname, n)
    group.PublicParams.upload(cname, gs, S, Hh, precompute_windows=True)
    return gs


def oracle_commit(corc, cname, gs, xi_row):
    """Commit(Gs[0..n), h.coeffs) of one xi row (ark) on the CPU."""
    m = P.CURVES[cname].scalar
    hc = pcdl_check.h_coeffs([to_int(x, m) for x in xi_row], m)
    sc = np.array([P.int_to_limbs(P.to_mont(x, m)) for x in hc], dtype=np.uint64).reshape(-1, 4)
    return corc.msm(cname, np.ascontiguousarray(gs[: len(hc)]), np.ascontiguousarray(sc))


def oracle_verdict(corc, cname, gs, xi_row, U) -> int:
    cv = P.CURVES[cname]
    try:
        unwrapped(cv, U)  # a point the reference's Affine type cannot hold has no commitment to equal
    except Exception:
        return 0
    m = cv.scalar
    return int(pcdl_check.decider_commit_matches(cname, U, [to_int(x, m) for x in xi_row], gs, corc.msm))


def random_rows(seed, k, lg):
    return det_scalars(seed, k * (lg + 1)).reshape(k, lg + 1, 4)


def rhos(seed, k):
    r = det_scalars(seed, k)
    r[:, 0] |= np.uint64(1)  # never zero
    return r


def decide_dev(hal, cname, d, xis, Us, live=None, rho=None):
    """halo_pcdl_decide_batch_dev over torch buffers on the current stream: (ok, combined)."""
    import torch
    k = len(Us)

    def dev(a, dtype=np.int64):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()

    d_x, d_U = dev(xis), dev(Us)
    d_l = dev(np.asarray(live, dtype=np.uint8), np.uint8) if live is not None else None
    d_r = dev(rho) if rho is not None else None
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_c = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    hal.check(hal.load().halo_pcdl_decide_batch_dev(
        hal.CURVES[cname], d, k, d_x.data_ptr(), d_U.data_ptr(), d_l.data_ptr() if live is not None else None,
        d_r.data_ptr() if rho is not None else None, d_ok.data_ptr(), d_c.data_ptr(), ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().tolist(), int(d_c.cpu().numpy()[0])


def launches(hal, name) -> int:
    n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
    hal.check(hal.load().halo_profile_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
    return n.value


# ---------------------------------------------------------------------------------------------
# 1. the commitments, both modes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg", [0, 1, 2, 3, 10, 12])
@pytest.mark.parametrize("cname", CURVES)
def test_decide_batch_accepts_the_oracles_commitments(hal, golden, corc, cname, lg):
    n, kmax = 1 << lg, 65
    gs = upload(corc, golden, cname, n)
    xis = random_rows(1000 + lg, kmax, lg)
    if lg:
        xis[1, lg] = 0  # a zero xi: every odd coefficient of h is zero
        xis[2, 1] = 0   # ... and the upper half
    Us = np.stack([oracle_commit(corc, cname, gs, row) for row in xis])
    G0 = unwrapped(P.CURVES[cname], gs[0])
    for k in (1, 2, 3, 65):
        assert pcdl.decide_batch(xis[:k], Us[:k], n - 1, curve=cname).tolist() == [1] * k, k
        assert pcdl.decide_batch(xis[:k], Us[:k], n - 1, rhos=rhos(7 + k, k), curve=cname).tolist() == [1] * k, k
        # the same U moved by G is no commitment of h: the comparison is of U' itself
        bad = Us[:k].copy()
        bad[k - 1] = wrapped(P.CURVES[cname], P.add(P.CURVES[cname], unwrapped(P.CURVES[cname], bad[k - 1]), G0))
        exp = [1] * (k - 1) + [0]
        assert pcdl.decide_batch(xis[:k], bad, n - 1, curve=cname).tolist() == exp, k
        assert pcdl.decide_batch(xis[:k], bad, n - 1, rhos=rhos(7 + k, k), curve=cname).tolist() == exp, k
    if lg:  # the rows with a zero xi on their own (k = 1 is always exact mode)
        assert pcdl.decide_batch(xis[1:3], Us[1:3], n - 1, curve=cname).tolist() == [1, 1]
        assert pcdl.decide_batch(xis[1:2], Us[1:2], n - 1, rhos=rhos(3, 1), curve=cname).tolist() == [1]


# ---------------------------------------------------------------------------------------------
# 2. damaged batches: both modes give the oracle's verdicts
# ---------------------------------------------------------------------------------------------
def damaged(cname, gs, xis, Us, i, kind):
    cv = P.CURVES[cname]
    xis, Us = xis.copy(), Us.copy()
    if kind == "plus_g":
        Us[i] = wrapped(cv, P.add(cv, unwrapped(cv, Us[i]), unwrapped(cv, gs[0])))
    elif kind == "xi":
        xis[i, 3] = plus_one(xis[i, 3], cv.scalar)
    elif kind == "identity":
        Us[i] = 0
    else:
        Us[i, 0] ^= np.uint64(1)  # off the curve
    return xis, Us


@pytest.fixture(scope="module")
def five(hal, golden, corc):
    """Per curve: the recipe SRS of 2^10 points, five random xi rows and the oracle's commitments."""
    out = {}
    for cname in CURVES:
        gs = _srs(corc, cname, 1 << 10)
        xis = random_rows(2000, 5, 10)
        out[cname] = (gs, xis, np.stack([oracle_commit(corc, cname, gs, row) for row in xis]))
    return out


@pytest.mark.parametrize("kind", ["plus_g", "xi", "identity", "off_curve"])
@pytest.mark.parametrize("cname", CURVES)
def test_damaged_batch_both_modes_give_the_oracles_verdicts(hal, golden, corc, five, cname, kind):
    """decide_group_scalars = 2 n: k = 5 makes the groups (0, 1), (2, 3), (4); the damaged instance is the first,
    the last, and on either side of the first boundary."""
    gs, xis, Us = five[cname]
    upload(corc, golden, cname, 1 << 10)
    with hal.tuning(decide_group_scalars=2 << 10):
        for i in (0, 1, 2, 4):
            x, U = damaged(cname, gs, xis, Us, i, kind)
            exp = [1] * 5
            exp[i] = oracle_verdict(corc, cname, gs, x[i], U[i])
            assert exp[i] == 0
            assert pcdl.decide_batch(x, U, 1023, curve=cname).tolist() == exp, (i, "exact")
            assert pcdl.decide_batch(x, U, 1023, rhos=rhos(11 + i, 5), curve=cname).tolist() == exp, (i, "combined")


# ---------------------------------------------------------------------------------------------
# 3. above msm_multi_max: pipelined MSMs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_pipelined_path_above_msm_multi_max(hal, golden, corc, cname):
    n = 1 << 11
    gs = upload(corc, golden, cname, n)
    xis = random_rows(3000, 3, 11)
    Us = np.stack([oracle_commit(corc, cname, gs, row) for row in xis])
    _, bad = damaged(cname, gs, xis, Us, 1, "plus_g")
    before = hal.get_tuning("msm_multi_max")
    with hal.tuning(msm_multi_max=1 << 10):
        assert pcdl.decide_batch(xis, Us, n - 1, curve=cname).tolist() == [1, 1, 1]
        assert pcdl.decide_batch(xis, bad, n - 1, curve=cname).tolist() == [1, 0, 1]
        assert pcdl.decide_batch(xis, bad, n - 1, rhos=rhos(5, 3), curve=cname).tolist() == [1, 0, 1]
    assert hal.get_tuning("msm_multi_max") == before


# ---------------------------------------------------------------------------------------------
# 4. combined mode is one MSM
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eight(hal, golden, corc):
    gs = _srs(corc, "pallas", 1 << 12)
    xis = random_rows(4000, 8, 12)
    return gs, xis, np.stack([oracle_commit(corc, "pallas", gs, row) for row in xis])


def test_combined_mode_launches_one_msm(hal, golden, corc, eight):
    gs, xis, Us = eight
    upload(corc, golden, "pallas", 1 << 12)
    _, bad = damaged("pallas", gs, xis, Us, 5, "plus_g")
    exp_bad = [1, 1, 1, 1, 1, 0, 1, 1]
    L = hal.load()
    hal.check(L.halo_profile_enable(1))
    try:
        hal.check(L.halo_profile_reset())
        assert pcdl.decide_batch(xis, Us, 4095, rhos=rhos(21, 8), curve="pallas").tolist() == [1] * 8
        assert launches(hal, "decide_msm") == 1 and launches(hal, "hpoly_combine") == 1 and launches(hal, "hpoly_rows") == 0
        hal.check(L.halo_profile_reset())
        assert decide_dev(hal, "pallas", 4095, xis, Us, rho=rhos(21, 8)) == ([1] * 8, 1)
        assert launches(hal, "decide_msm") == 1
        # one damaged instance: the host form reruns the batch in exact mode (one group, so one more MSM stage)
        hal.check(L.halo_profile_reset())
        assert pcdl.decide_batch(xis, bad, 4095, rhos=rhos(21, 8), curve="pallas").tolist() == exp_bad
        assert launches(hal, "decide_msm") == 2 and launches(hal, "hpoly_rows") == 1
        # the _dev form reports combined = 0 and does not fall back
        hal.check(L.halo_profile_reset())
        assert decide_dev(hal, "pallas", 4095, xis, bad, rho=rhos(21, 8)) == ([0] * 8, 0)
        assert launches(hal, "decide_msm") == 1 and launches(hal, "hpoly_rows") == 0
        assert decide_dev(hal, "pallas", 4095, xis, bad) == (exp_bad, 7)  # exact: combined is not written
        # exact mode: one stage per group
        hal.check(L.halo_profile_reset())
        with hal.tuning(decide_group_scalars=3 << 12):
            assert pcdl.decide_batch(xis, bad, 4095, curve="pallas").tolist() == exp_bad
        assert launches(hal, "decide_msm") == 3 and launches(hal, "hpoly_rows") == 3
    finally:
        hal.check(L.halo_profile_enable(0))
        hal.check(L.halo_profile_reset())


# ---------------------------------------------------------------------------------------------
# 5. live masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plus_g", "off_curve"])
def test_masked_out_instance_disturbs_nothing(hal, golden, corc, eight, kind):
    gs, xis, Us = eight
    upload(corc, golden, "pallas", 1 << 12)
    x, bad = damaged("pallas", gs, xis, Us, 3, kind)
    live = [1, 1, 1, 0, 1, 1, 0, 1]  # 6 is a good instance that is skipped
    exp = [1, 1, 1, 0, 1, 1, 0, 1]
    assert pcdl.decide_batch(x, bad, 4095, live=live, curve="pallas").tolist() == exp
    assert pcdl.decide_batch(x, bad, 4095, rhos=rhos(31, 8), live=live, curve="pallas").tolist() == exp
    assert decide_dev(hal, "pallas", 4095, x, bad, live=live, rho=rhos(31, 8)) == (exp, 1)
    assert decide_dev(hal, "pallas", 4095, x, bad, live=live)[0] == exp
    assert pcdl.decide_batch(x, bad, 4095, live=[0] * 8, curve="pallas").tolist() == [0] * 8
    assert decide_dev(hal, "pallas", 4095, x[3:4], bad[3:4], live=[0], rho=rhos(31, 1)) == ([0], 1)


# ---------------------------------------------------------------------------------------------
# 6. errors before any device work
# ---------------------------------------------------------------------------------------------
def test_errors(hal, golden, corc, eight):
    gs, xis, Us = eight
    upload(corc, golden, "pallas", 1 << 12)
    r = rhos(41, 8)
    zero = r.copy()
    zero[4] = 0
    with pytest.raises(hal.HaloError, match=r"rho\[4\] is zero") as e:
        pcdl.decide_batch(xis, Us, 4095, rhos=zero, curve="pallas")
    assert e.value.code == 1
    big = r.copy()
    big[7] = np.array(P.int_to_limbs(P.CURVES["pallas"].scalar), dtype=np.uint64)  # the modulus itself
    with pytest.raises(hal.HaloError, match=r"rho\[7\] is not below the modulus") as e:
        pcdl.decide_batch(xis, Us, 4095, rhos=big, curve="pallas")
    assert e.value.code == 1
    x13 = random_rows(42, 2, 13)
    with pytest.raises(hal.HaloAssertion, match="d was larger than D!") as e:
        pcdl.decide_batch(x13, Us[:2], (1 << 13) - 1, curve="pallas")
    assert e.value.code == 5
    with pytest.raises(hal.HaloAssertion, match=r"n \(4095\) is not a power of two"):
        pcdl.decide_batch(xis[:, :12], Us, 4094, curve="pallas")
    L = hal.load()
    assert L.halo_pcdl_decide_batch(0, 4095, 0, None, None, None, None, None) == 0
    assert L.halo_pcdl_decide_batch_dev(0, 4095, 0, None, None, None, None, None, None, None) == 0
    assert L.halo_pcdl_check_fs_batch(0, 4095, 0, *[None] * 12) == 0
    assert L.halo_pcdl_check_fs_batch_dev(0, 4095, 0, *[None] * 14) == 0


# ---------------------------------------------------------------------------------------------
# 7. pcdl::check from raw instances
# ---------------------------------------------------------------------------------------------
def case_item(golden, corc, key):
    """(cname, d, (C, z, v, pi)) of a committed opening; its SRS is uploaded."""
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    return cname, d, (C, z, v, pi)


@functools.lru_cache(maxsize=None)
def _oracle_xis(cname, d, C, z, v, Ls, Rs, C_bar, w_prime, S):
    """The challenges of one instance as canonical ints, from its bytes (the transcript reads neither U nor c)."""
    cv = P.CURVES[cname]
    m = cv.scalar
    import poseidon
    pt = lambda b: unwrapped(cv, np.frombuffer(b, dtype=np.uint64))  # noqa: E731
    sc = lambda b: to_int(np.frombuffer(b, dtype=np.uint64), m)  # noqa: E731
    t = poseidon.Sponge(cname, poseidon.PCDL)
    Cp = pt(C)
    alpha = None
    if C_bar is not None:
        t.absorb_g([Cp, pt(C_bar)])
        t.absorb_fr([sc(z), sc(v)])
        alpha = t.challenge()
        Cp = P.add(cv, P.add(cv, Cp, P.mul_fast(cv, alpha, pt(C_bar))), P.neg(cv, P.mul_fast(cv, sc(w_prime), pt(S))))
    t.absorb_g([Cp])
    t.absorb_fr([sc(z), sc(v)])
    xis = [t.challenge()]
    for j in range(len(Ls) // 64):
        t.absorb_fr([xis[j]])
        t.absorb_g([pt(Ls[64 * j: 64 * j + 64]), pt(Rs[64 * j: 64 * j + 64])])
        xis.append(t.challenge())
    return alpha, tuple(xis)


def oracle_xis(cname, golden, d, item):
    C, z, v, pi = item
    b = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()  # noqa: E731
    hid = pi.get("C_bar") is not None
    return _oracle_xis(cname, d, b(C), b(z), b(v), b(pi["Ls"]), b(pi["Rs"]), b(pi["C_bar"]) if hid else None,
                       b(pi["w_prime"]) if hid else None, b(golden[f"ref_sh_{cname}"][0]))


def oracle_code(corc, cname, golden, d, item) -> int:
    """pcdl::check on the CPU: 0, 1 (the succinct check raises) or 2 (U is not the commitment of h)."""
    C, z, v, pi = item
    m = P.CURVES[cname].scalar
    S, Hh = golden[f"ref_sh_{cname}"]
    alpha, xis = oracle_xis(cname, golden, d, item)
    hid = pi.get("C_bar") is not None
    try:
        pcdl_check.succinct_check(cname, C, d, to_int(z, m), to_int(v, m), pi["Ls"], pi["Rs"], pi["U"], to_int(pi["c"], m),
                                  list(xis), Hh, S=S, C_bar=pi["C_bar"], w_prime=to_int(pi["w_prime"], m) if hid else None,
                                  alpha=alpha)
    except AssertionError:
        return 1
    return 0 if pcdl_check.decider_commit_matches(cname, pi["U"], list(xis), _srs(corc, cname, d + 1), corc.msm) else 2


def tampered_c(cname, item):
    C, z, v, pi = item
    return C, z, v, dict(pi, c=plus_one(pi["c"], P.CURVES[cname].scalar))


def forged_u(cname, golden, d, item):
    """c' = 2 c and U* = U / 2 - (h(z) xi_0 / 2) H: the succinct check holds, U* is not the commitment of h."""
    C, z, v, pi = item
    cv = P.CURVES[cname]
    m = cv.scalar
    _, xis = oracle_xis(cname, golden, d, item)
    half = pow(2, -1, m)
    hz = pcdl_check.h_eval(list(xis), to_int(z, m), m)
    Hh = unwrapped(cv, golden[f"ref_sh_{cname}"][1])
    U = P.add(cv, P.mul_fast(cv, half, unwrapped(cv, pi["U"])), P.neg(cv, P.mul_fast(cv, hz * xis[0] % m * half % m, Hh)))
    return C, z, v, dict(pi, c=fe(2 * to_int(pi["c"], m), m), U=wrapped(cv, U))


def run_check(cname, d, items, rho=None):
    hid = [pi.get("C_bar") is not None for *_, pi in items]
    zero_pt, zero_fe = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    return pcdl.check_fs_codes(
        np.stack([C for C, *_ in items]), d, np.stack([z for _, z, _, _ in items]), np.stack([v for _, _, v, _ in items]),
        np.concatenate([pi["Ls"] for *_, pi in items]) if d else None,
        np.concatenate([pi["Rs"] for *_, pi in items]) if d else None, np.stack([pi["U"] for *_, pi in items]),
        np.stack([pi["c"] for *_, pi in items]), hiding=hid if any(hid) else None,
        C_bars=np.stack([pi["C_bar"] if h else zero_pt for (*_, pi), h in zip(items, hid)]),
        w_primes=np.stack([pi["w_prime"] if h else zero_fe for (*_, pi), h in zip(items, hid)]), rhos=rho,
        curve=cname).tolist()


def run_check_dev(hal, cname, d, items, rho=None):
    """halo_pcdl_check_fs_batch_dev over torch buffers on the current stream: (codes, combined)."""
    import torch
    k = len(items)

    def dev(a, dtype=np.int64):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()

    hid = np.array([pi.get("C_bar") is not None for *_, pi in items], dtype=np.uint8)
    zero_pt, zero_fe = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    bufs = [dev(np.stack([C for C, *_ in items])), dev(np.stack([z for _, z, _, _ in items])),
            dev(np.stack([v for _, _, v, _ in items])), dev(np.concatenate([pi["Ls"] for *_, pi in items])),
            dev(np.concatenate([pi["Rs"] for *_, pi in items])), dev(np.stack([pi["U"] for *_, pi in items])),
            dev(np.stack([pi["c"] for *_, pi in items])), dev(hid, np.uint8),
            dev(np.stack([pi["C_bar"] if h else zero_pt for (*_, pi), h in zip(items, hid)])),
            dev(np.stack([pi["w_prime"] if h else zero_fe for (*_, pi), h in zip(items, hid)]))]
    d_rho = dev(rho) if rho is not None else None
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_c = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    hal.check(hal.load().halo_pcdl_check_fs_batch_dev(
        hal.CURVES[cname], d, k, *[b.data_ptr() for b in bufs], d_rho.data_ptr() if rho is not None else None,
        d_ok.data_ptr(), d_c.data_ptr(), ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().tolist(), int(d_c.cpu().numpy()[0])


@pytest.mark.parametrize("key", CASES)
def test_check_fs_batch_on_the_committed_openings(fs, golden, corc, key):
    cname, d, item = case_item(golden, corc, key)
    bad_c, forged = tampered_c(cname, item), forged_u(cname, golden, d, item)
    assert [oracle_code(corc, cname, golden, d, q) for q in (item, bad_c, forged)] == [0, 1, 2]
    assert run_check(cname, d, [item]) == [0]
    assert run_check(cname, d, [bad_c]) == [1]
    assert run_check(cname, d, [forged]) == [2]
    for rho in (None, rhos(51, 3)):
        assert run_check(cname, d, [forged, item, bad_c], rho=rho) == [2, 0, 1]
        assert run_check(cname, d, [item, bad_c, item], rho=rho) == [0, 1, 0]  # a failed succinct check is masked out


@pytest.mark.parametrize("k", [22, 65])
@pytest.mark.parametrize("cname", CURVES)
def test_check_fs_batch_mixed(fs, golden, corc, cname, k):
    """Plain and hiding openings of n = 4096 alternate; c tampered at 0 and k - 1, U forged at 20 and 21 (the lane
    layouts' wave boundaries: 21 three-lane sponges, 64 one-lane ones)."""
    _, d, hiding = case_item(golden, corc, f"big_{cname}_n4096_hiding")
    _, _, plain = case_item(golden, corc, f"big_{cname}_n4096_plain")
    pair = [plain, hiding]
    items = [pair[i % 2] for i in range(k)]
    kinds = {0: "c", 20: "U", 21: "U"}
    kinds.setdefault(k - 1, "c")  # the last instance: 21 itself at k = 22
    for i, kind in kinds.items():
        items[i] = tampered_c(cname, items[i]) if kind == "c" else forged_u(cname, golden, d, items[i])
    exp = [oracle_code(corc, cname, golden, d, q) for q in items]
    assert exp == [{"c": 1, "U": 2}.get(kinds.get(i), 0) for i in range(k)]
    r = rhos(61, k)
    assert run_check(cname, d, items) == exp
    assert run_check(cname, d, items, rho=r) == exp
    assert run_check_dev(fs, cname, d, items) == (exp, 7)
    # combined mode in the _dev form: the batch holds forgeries, so combined = 0 and no decider verdict is given
    codes, combined = run_check_dev(fs, cname, d, items, rho=r)
    assert combined == 0 and codes == [1 if e == 1 else 2 for e in exp]
    good = [q if e != 2 else pair[i % 2] for i, (q, e) in enumerate(zip(items, exp))]
    exp_good = [e if e != 2 else 0 for e in exp]
    assert run_check_dev(fs, cname, d, good, rho=r) == (exp_good, 1)
    assert run_check(cname, d, good, rho=r) == exp_good


def test_python_layer_against_check_device(fs, golden, corc):
    """pcdl.check_batch / acc.decider_batch over two degree bounds against pcdl.check_device one by one."""
    insts = []
    for key in ("open_pallas_n16_plain", "open_pallas_n64_hiding"):  # the longer SRS is uploaded last
        cname, d, item = case_item(golden, corc, key)
        insts += [pcdl.Instance(item[0], d, item[1], item[2], item[3])]
    good = [insts[0], insts[1], insts[0], insts[1]]
    bad = list(good)
    q = forged_u("pallas", golden, 63, (good[1].C, good[1].z, good[1].v, good[1].pi))
    bad[1] = good[1]._replace(pi=q[3])
    q = tampered_c("pallas", (good[2].C, good[2].z, good[2].v, good[2].pi))
    bad[2] = good[2]._replace(pi=q[3])

    def one_by_one(batch):
        out = []
        for q in batch:
            try:
                pcdl.check_device(q.C, q.d, q.z, q.v, q.pi, curve="pallas")
                out.append(0)
            except pcdl.CheckFailed as e:
                out.append({pcdl.SUCCINCT_MSG: 1, pcdl.DECIDER_MSG: 2}[e.msg])
        return out

    assert one_by_one(good) == [0, 0, 0, 0] and one_by_one(bad) == [0, 2, 1, 0]
    for rho in (None, rhos(71, 4)):
        assert pcdl.check_batch(good, rhos=rho, curve="pallas") is None
        acc.decider_batch(good, rhos=rho, curve="pallas")
        assert pcdl.check_batch(bad, rhos=rho, curve="pallas", verdicts=True).tolist() == one_by_one(bad)
        with pytest.raises(pcdl.CheckFailed, match="^U ≠ CM.Commit\\(ck, h_vec\\) \\(instance 1\\)$") as e:
            pcdl.check_batch(bad, rhos=rho, curve="pallas")
        assert e.value.index == 1 and e.value.msg == pcdl.DECIDER_MSG
        with pytest.raises(pcdl.CheckFailed, match="instance 0") as e:
            acc.decider_batch(bad[2:], rhos=rho[2:] if rho is not None else None, curve="pallas")
        assert e.value.index == 0 and e.value.msg == pcdl.SUCCINCT_MSG
    with pytest.raises(pcdl.CheckFailed, match="d was larger than D!"):
        pcdl.check_batch([good[0]._replace(d=127)], curve="pallas")


# ---------------------------------------------------------------------------------------------
# 8. PlonkProof::verify for k proofs
# ---------------------------------------------------------------------------------------------
import plonk_ref as R  # noqa: E402
from halo_amd import plonk  # noqa: E402
from test_gpu_plonk_verify import G as PG, arrays, mds_ark, run_batch as run_succinct  # noqa: E402
from test_gpu_plonk_verify import FIELDS as PFIELDS  # noqa: E402

WHY = {"": plonk.ACCEPT, "succinct": plonk.DECIDER_SUCCINCT, "decider": plonk.DECIDER}


@pytest.fixture
def pv(fs, golden):
    """The SRS recipe's first 64 points for both curves (the fixtures' SRS; uploaded per test, as the tests above
    upload theirs), Poseidon constants installed."""
    for cname in CURVES:
        S, Hh = golden[f"ref_sh_{cname}"]
        group.PublicParams.upload(cname, np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"]), S, Hh,
                                  precompute_windows=True)
    return fs


def restated_verify(cname, rows, C_qs, golden, rec) -> int:
    """PlonkProof::verify on the CPU (tests/plonk_ref.py): the verify_succinct code, else what pcdl::check of
    acc_next rejected."""
    code, why = R.verify(cname, rows, C_qs, golden[f"ref_sh_{cname}"][1], rec, golden[f"ref_srs_{cname}_b00_first64"])
    return code if code else WHY[why]


def forged_next_u(cname, rows, golden, rec):
    """acc_next.pi with c' = 2 c and the U* that its succinct check accepts (forged_u)."""
    Ls, Rs, U, c = rec.next_pi
    item = (rec.next[:8], rec.next[8:12], rec.next[12:], {"Ls": Ls, "Rs": Rs, "U": U, "c": c, "C_bar": None, "w_prime": None})
    pi = forged_u(cname, golden, rows - 1, item)[3]
    return rec._replace(next_pi=(Ls, Rs, pi["U"], pi["c"]))


def run_verify(hal, cname, rows, C_qs, recs, rho=None, dev=False):
    """halo_plonk_verify_batch (or its _dev form) over k Recs: the verdicts (and `combined`)."""
    k = len(recs)
    a = arrays(recs)
    npi = a["pub"].shape[1]
    nxt = [np.ascontiguousarray(np.stack([r.next_pi[j] for r in recs])) for j in range(4)]
    ins = [np.ascontiguousarray(C_qs), a["pub"] if npi else None] + [a[f] for f in PFIELDS] + \
        [a["prev_C"], a["prev_z"], a["prev_v"], a["next_C"], a["next_z"], a["next_v"]] + nxt + [mds_ark(cname), rho]
    verdict = np.full(k, 77, dtype=np.uint8)
    L = hal.load()
    if not dev:
        p = [hal.ptr(x) for x in ins]
        hal.check(L.halo_plonk_verify_batch(hal.CURVES[cname], rows, k, p[0], p[1], npi, *p[2:], hal.ptr(verdict)))
        return verdict.tolist()
    import torch
    d_in = [None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda() for x in ins]
    d_v = torch.full((k,), 77, dtype=torch.uint8, device="cuda")
    d_c = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    p = [None if t is None else t.data_ptr() for t in d_in]
    hal.check(L.halo_plonk_verify_batch_dev(hal.CURVES[cname], rows, k, p[0], p[1], npi, *p[2:], d_v.data_ptr(),
                                            d_c.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return d_v.cpu().numpy().tolist(), int(d_c.cpu().numpy()[0])


@pytest.mark.parametrize("key", sorted(R.CHAINS))
def test_plonk_verify_batch_accepts_the_fixtures(pv, golden, key):
    cname, rows = R.CHAINS[key]
    C_qs, recs = R.load_chain(PG, key)
    assert [restated_verify(cname, rows, C_qs, golden, r) for r in recs] == [0, 0]
    assert run_verify(pv, cname, rows, C_qs, recs) == [0, 0]
    assert run_verify(pv, cname, rows, C_qs, recs, rho=rhos(81, 2)) == [0, 0]
    assert run_verify(pv, cname, rows, C_qs, recs[:1], rho=rhos(81, 1)) == [0]
    assert run_verify(pv, cname, rows, C_qs, recs, rho=rhos(81, 2), dev=True) == ([0, 0], 1)
    assert run_verify(pv, cname, rows, C_qs, recs, dev=True) == ([0, 0], 7)


@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_plonk_verify_batch_tampered(pv, golden, key):
    """Every tampering of tests/plonk_ref.py: the code of halo_plonk_verify_succinct_batch on the same batch where
    that is nonzero; a tampered acc_next.pi.c is 9; a forged acc_next.pi.U is 10; failing both reports the
    earlier code."""
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(PG, key)
    kinds = sorted(R.TAMPERINGS)
    items = [R.tamper(recs[i % 2], kind, m) for i, kind in enumerate(kinds)]
    items.append(forged_next_u(cname, rows, golden, recs[0]))                                  # 10
    items.append(R.tamper(R.tamper(recs[1], "r_c", m), "next_pi_c", m))                         # both: INSTANCE_1
    items.append(forged_next_u(cname, rows, golden, R.tamper(recs[0], "next_z", m)))           # both: Z
    Ls, Rs, U, c = recs[1].next_pi
    items.append(recs[1]._replace(next_pi=(Ls, Rs, recs[1].U[0].copy(), c)))                    # U swapped: 9 already
    items.append(recs[0])
    exp = [restated_verify(cname, rows, C_qs, golden, r) for r in items]
    succinct = run_succinct(pv, cname, rows, C_qs, items)[0].tolist()
    assert exp[-5:] == [plonk.DECIDER, plonk.INSTANCE_1, plonk.Z, plonk.DECIDER_SUCCINCT, plonk.ACCEPT]
    assert exp[kinds.index("next_pi_c")] == plonk.DECIDER_SUCCINCT
    assert [e if s else 0 for e, s in zip(exp, succinct)] == succinct  # a nonzero succinct code is the verdict
    assert [s for s, kind in zip(succinct, kinds)] == [R.TAMPERINGS[kind] for kind in kinds]
    assert run_verify(pv, cname, rows, C_qs, items) == exp
    assert run_verify(pv, cname, rows, C_qs, items, rho=rhos(91, len(items))) == exp
    assert run_verify(pv, cname, rows, C_qs, items, dev=True) == (exp, 7)
    codes, combined = run_verify(pv, cname, rows, C_qs, items, rho=rhos(91, len(items)), dev=True)
    assert combined == 0 and codes == [plonk.DECIDER if e in (0, plonk.DECIDER) else e for e in exp]
    # the Python layer
    from test_gpu_plonk_verify import as_proof, circuit_of
    trio = [as_proof(r, rows) for r in items]
    got = plonk.verify_batch(circuit_of(cname, rows, C_qs), [t[1] for t in trio], [t[2] for t in trio], [t[0] for t in trio],
                             rhos=rhos(92, len(items)), curve=cname)
    assert got.tolist() == exp


@pytest.mark.parametrize("k", [22, 65])
@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_plonk_verify_batch_mixed(pv, golden, key, k):
    """Accepts, every reject kind of verify_succinct and both decider rejects inside one batch that crosses a
    three-lane wave (22) and a one-lane wave (65)."""
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(PG, key)
    kinds = sorted(R.TAMPERINGS)
    items = []
    for i in range(k):
        rec = recs[(i // 2) % 2]
        if i % 4 == 1 or i == k - 1:
            rec = R.tamper(rec, kinds[(i // 4) % len(kinds)], m)
        elif i % 4 == 3:
            rec = forged_next_u(cname, rows, golden, rec)
        items.append(rec)
    exp = [restated_verify(cname, rows, C_qs, golden, r) for r in items]
    assert {0, plonk.DECIDER_SUCCINCT, plonk.DECIDER} <= set(exp) and len(set(exp)) >= 6
    assert run_verify(pv, cname, rows, C_qs, items) == exp
    assert run_verify(pv, cname, rows, C_qs, items, rho=rhos(95, k)) == exp
    assert run_verify(pv, cname, rows, C_qs, items, dev=True)[0] == exp
    good = [r if e != plonk.DECIDER else recs[0] for r, e in zip(items, exp)]
    exp_good = [e if e != plonk.DECIDER else 0 for e in exp]
    assert run_verify(pv, cname, rows, C_qs, good, rho=rhos(95, k), dev=True) == (exp_good, 1)


def test_plonk_verify_batch_errors(pv, golden):
    C_qs, recs = R.load_chain(PG, "pallas_n8")
    zero = rhos(97, 2)
    zero[1] = 0
    with pytest.raises(pv.HaloError, match=r"rho\[1\] is zero"):
        run_verify(pv, "pallas", 8, C_qs, recs, rho=zero)
    Ls, Rs, U, c = recs[1].next_pi
    big = recs[1]._replace(next_pi=(Ls, Rs, U, np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)))
    with pytest.raises(pv.HaloError, match="proof 1 is not below the modulus"):
        run_verify(pv, "pallas", 8, C_qs, [recs[0], big])
    with pytest.raises(AssertionError, match=r"n \(12\) is not a power of two"):
        run_verify(pv, "pallas", 12, C_qs, recs)
    L = pv.load()
    assert L.halo_plonk_verify_batch(0, 8, 0, *([None] * 2), 0, *([None] * 21)) == 0
    assert L.halo_plonk_verify_batch_dev(0, 8, 0, *([None] * 2), 0, *([None] * 23)) == 0
    assert plonk.verify_batch(plonk.PlonkCircuit(8, C_qs, 2, mds_ark("pallas")), [], [], []).tolist() == []
