"""GPU tests of the accumulation scheme in one call each (halo_amd/csrc/acc_fs.hip behind halo_acc_verifier_batch,
its _dev form and halo_acc_prover; halo_amd.acc.common_subroutine_device / prover_device / verifier_device /
verifier_batch): the ASDL transcript on the device, bit for bit against today's acc.prover / acc.verifier /
acc.common_subroutine under the restated Poseidon sponge (SpongeAdapter, pinned to the reference by
tests/golden/transcript.npz).  No tolerance is involved.

  * prover parity on both curves and both lane layouts, m = 1, 2, 3, 5 at n = 16 and m = 2 at n = 2 (both parities
    of the absorbed element count; m = 5 is no power of two, m = 1 a single alpha^0 term), hiding and plain mixed;
  * the verdicts in the reference's order and their isolation in batches that cross a three-lane wave (21 sponges),
    a three-lane block (84) and a one-lane block (256);
  * points off the curve, the identity as acc.C, lg n = 0, the device-pointer form, a failing prover call, the backend."""
import ctypes

import numpy as np
import pytest

import pasta as P
from halo_amd import acc, group, pcdl
from test_gpu_pcdl_check import SpongeAdapter, det_scalars, fe, plus_one
from test_gpu_pcdl_fs import fresh_opening, fs, oracle_transcript  # noqa: F401  (fs: the fixture)

pytestmark = pytest.mark.gpu
LANES = [1, 3]
CURVES = ["pallas", "vesta"]
ACCEPT, INSTANCE, C_BAR, Z, V = range(5)


def transcripts(cname):
    return lambda label: SpongeAdapter(cname, label)


def use_srs(corc, golden, cname, n):
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, corc.srs_generate(cname, n), S, Hh, precompute_windows=True)


@pytest.fixture(scope="module")
def inst(fs, golden, corc):
    """Per curve: five plain n = 16 instances and one hiding one (index 5), two plain n = 2 instances ("n2"), made once
    under the oracle sponge.  The n = 16 SRS is uploaded last and stays."""
    out = {}
    for cname in CURVES:
        two = [pcdl.Instance(C, 1, z, v, pi) for C, z, v, pi in (fresh_opening(corc, golden, cname, 2, False, 1200 + i) for i in range(2))]
        qs = [pcdl.Instance(C, 15, z, v, pi)
              for C, z, v, pi in (fresh_opening(corc, golden, cname, 16, i == 5, 1100 + i) for i in range(6))]
        out[cname] = qs
        out[cname + "_n2"] = two
    return out


_ORACLE = {}


def oracle_prover(cname, key, qs):
    """acc.prover and acc.common_subroutine under SpongeAdapter, once per (curve, shape)."""
    if (cname, key) not in _ORACLE:
        nt = transcripts(cname)
        _ORACLE[cname, key] = (acc.prover(qs, nt, curve=cname), acc.common_subroutine(qs, nt, curve=cname))
    return _ORACLE[cname, key]


def same_accumulator(a, e):
    assert np.array_equal(a.C, e.C) and a.d == e.d and np.array_equal(a.z, e.z) and np.array_equal(a.v, e.v)
    assert len(a.pi["Ls"]) == len(e.pi["Ls"]) and len(a.pi["Rs"]) == len(e.pi["Rs"])
    assert all(np.array_equal(x, y) for x, y in zip(a.pi["Ls"], e.pi["Ls"]))
    assert all(np.array_equal(x, y) for x, y in zip(a.pi["Rs"], e.pi["Rs"]))
    assert np.array_equal(a.pi["U"], e.pi["U"]) and np.array_equal(a.pi["c"], e.pi["c"])
    assert np.array_equal(a.pi["v"], e.pi["v"])  # the oracle route's opener evaluated its own h at z


def opened_polynomial_at_z(qs, a, cname):
    """h(z) by a route that shares nothing with k_acc_finish's product forms: the coefficients of sum alpha^j h_j from
    the host route's challenges (HPoly.combine), evaluated at the accumulator's z (pcdl.evaluate)."""
    _, _, _, hs, alphas = acc.common_subroutine(qs, transcripts(cname), curve=cname, device_transcripts=True)
    return pcdl.evaluate(pcdl.HPoly.combine(hs, alphas), a.z, curve=cname)


# ---------------------------------------------------------------------------------------------
# 1, 2. prover parity
# ---------------------------------------------------------------------------------------------
SHAPES = [("n16_m1", 16, [0]), ("n16_m2", 16, [0, 1]), ("n16_m3", 16, [0, 1, 2]), ("n16_m5", 16, [0, 1, 2, 3, 4]),
          ("n2_m2", 2, [0, 1]), ("n16_mixed", 16, [0, 5, 1])]


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("key,n,idx", SHAPES)
@pytest.mark.parametrize("cname", CURVES)
def test_prover_parity(fs, golden, corc, inst, cname, key, n, idx, lanes):
    use_srs(corc, golden, cname, n)
    qs = [inst[cname if n == 16 else cname + "_n2"][i] for i in idx]
    exp, _ = oracle_prover(cname, key, qs)
    with fs.tuning(poseidon_lanes=lanes):
        a = acc.prover_device(qs, curve=cname)
        same_accumulator(a, exp)
        acc.verifier_device(qs, a, curve=cname)
    # the opener's own v = h(z) equals the accumulator's v: halo_acc_prover compares the two on its side (a
    # mismatch is an error of the call), and here the accumulator's v meets h(z) evaluated from coefficients
    assert np.array_equal(opened_polynomial_at_z(qs, a, cname), a.v)
    acc.verifier(qs, a, transcripts(cname), curve=cname)
    acc.decider(a, transcripts(cname), curve=cname)


# ---------------------------------------------------------------------------------------------
# 3. common_subroutine_device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", CURVES)
def test_common_subroutine_device(fs, golden, corc, inst, cname, lanes):
    use_srs(corc, golden, cname, 16)
    qs = [inst[cname][i] for i in (0, 1, 2)]
    _, exp = oracle_prover(cname, "n16_m3", qs)
    with fs.tuning(poseidon_lanes=lanes):
        got = acc.common_subroutine_device(qs, curve=cname)
    assert np.array_equal(got[0], exp[0]) and got[1] == exp[1] and np.array_equal(got[2], exp[2])
    assert len(got[3]) == 3 and all(np.array_equal(a.xis, b.xis) for a, b in zip(got[3], exp[3]))
    assert np.array_equal(got[4], exp[4])
    m = P.CURVES[cname].scalar
    bad = list(qs)
    bad[1] = qs[1]._replace(v=plus_one(qs[1].v, m))
    with pytest.raises(pcdl.CheckFailed, match="instance 1") as e:
        acc.common_subroutine_device(bad, curve=cname)
    assert e.value.msg == pcdl.SUCCINCT_MSG and e.value.index == 1
    with pytest.raises(pcdl.CheckFailed, match="^No instances given$"):
        acc.common_subroutine_device([], curve=cname)
    with pytest.raises(pcdl.CheckFailed, match="d_i ≠ d") as e:
        acc.prover_device([qs[0], inst[cname + "_n2"][0]], curve=cname)
    assert e.value.index == 1


# ---------------------------------------------------------------------------------------------
# 4. verdict order and isolation
# ---------------------------------------------------------------------------------------------
def oracle_code(cname, qs, a):
    """acc.verifier under SpongeAdapter as (verdict, first_bad)."""
    try:
        acc.verifier(qs, a, transcripts(cname), curve=cname)
    except pcdl.CheckFailed as e:
        if e.msg == pcdl.SUCCINCT_MSG:
            return INSTANCE, e.index
        return {"C_bar' ≠ C_bar": C_BAR, "z' = z": Z, "h(z) = v": V}[e.msg], len(qs)
    return ACCEPT, len(qs)


@pytest.fixture(scope="module")
def cases(fs, golden, corc, inst):
    """Per curve: the distinct (qs, acc) cases of the verdict tests and their oracle codes, the oracle run once each."""
    out = {}
    for cname in CURVES:
        use_srs(corc, golden, cname, 16)
        m = P.CURVES[cname].scalar
        qs = [inst[cname][0], inst[cname][1]]
        a, _ = oracle_prover(cname, "n16_m2", qs)
        bad_c = qs[1]._replace(pi=dict(qs[1].pi, c=plus_one(qs[1].pi["c"], m)))
        bad_u = qs[0]._replace(pi=dict(qs[0].pi, U=qs[0].pi["Ls"][1].copy()))
        table = {"good": (qs, a), "c1": ([qs[0], bad_c], a), "u0": ([bad_u, qs[1]], a),
                 "C": (qs, a._replace(C=qs[0].pi["U"].copy())), "z": (qs, a._replace(z=plus_one(a.z, m))),
                 "v": (qs, a._replace(v=plus_one(a.v, m))), "both": ([bad_u, bad_c], a),
                 "c1_z": ([qs[0], bad_c], a._replace(z=plus_one(a.z, m)))}
        out[cname] = {name: (q, ac, oracle_code(cname, q, ac)) for name, (q, ac) in table.items()}
    return out


def test_oracle_codes_are_the_ones_the_cases_are_named_for(cases):
    for cname in CURVES:
        got = {name: code for name, (_, _, code) in cases[cname].items()}
        assert got == {"good": (ACCEPT, 2), "c1": (INSTANCE, 1), "u0": (INSTANCE, 0), "C": (C_BAR, 2), "z": (Z, 2),
                       "v": (V, 2), "both": (INSTANCE, 0), "c1_z": (INSTANCE, 1)}


def tampered_batch(cs, k):
    """k pairs, the good one replicated and the tamper kinds cycled over positions 0, 20, 21, 22 and k - 1; the two
    combined tampers at 10 and 11.  At k = 22, where 22 is past the batch and k - 1 is 21, the kinds of 21 and 22
    go to 12 and 13."""
    names = ["good"] * k
    names[10], names[11] = "both", "c1_z"
    for pos, name in zip((0, 20, 21, 22, k - 1), ("c1", "u0", "C", "z", "v")):
        if pos < k:
            names[pos] = name
    if k == 22:
        names[12], names[13] = "C", "z"
    return names


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("k", [22, 85, 257])
@pytest.mark.parametrize("cname", CURVES)
def test_verdict_order_and_isolation(fs, golden, corc, cases, cname, k, lanes):
    use_srs(corc, golden, cname, 16)
    cs = cases[cname]
    names = tampered_batch(cs, k)
    with fs.tuning(poseidon_lanes=lanes):
        verdict, first_bad, asdl, C_bar, v = acc.verifier_codes([cs[n][0] for n in names], [cs[n][1] for n in names], 15, cname)
    assert verdict.tolist() == [cs[n][2][0] for n in names]
    assert first_bad.tolist() == [cs[n][2][1] for n in names]
    good = cs["good"][1]
    for i, n in enumerate(names):
        if n in ("good", "C", "z", "v"):  # the instances are the good ones: alpha, z', C_bar', v' are the accumulator's
            assert np.array_equal(asdl[i, 1], good.z) and np.array_equal(v[i], good.v), i
            assert np.array_equal(C_bar[i], good.C), i  # "C": the sum is not the identity there, acc.C is added back
    if k == 22:
        with fs.tuning(poseidon_lanes=lanes):
            codes = acc.verifier_batch([(cs[n][0], cs[n][1]) for n in names[1:10]], curve=cname, verdicts=True)
            assert codes.tolist() == [ACCEPT] * 9
            with pytest.raises(pcdl.CheckFailed, match="^z' = z \\(instance 2\\)$"):
                acc.verifier_batch([(cs[n][0], cs[n][1]) for n in ("good", "good", "z", "v")], curve=cname)
            for name, text in (("c1", "instance 1"), ("C", "^C_bar' ≠ C_bar$"), ("z", "^z' = z$"), ("v", "^h\\(z\\) = v$")):
                with pytest.raises(pcdl.CheckFailed, match=text):
                    acc.verifier_device(cs[name][0], cs[name][1], curve=cname)


# ---------------------------------------------------------------------------------------------
# 5. points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", CURVES)
def test_points(fs, golden, corc, cases, cname, lanes):
    use_srs(corc, golden, cname, 16)
    qs, a, _ = cases[cname]["good"]
    off_u = qs[1].pi["U"].copy()
    off_u[0] ^= np.uint64(1)
    off_l = qs[0].pi["Ls"].copy()
    off_l[2, 4] ^= np.uint64(1)
    off_c = a.C.copy()
    off_c[0] ^= np.uint64(1)
    pairs = [(qs, a), ([qs[0], qs[1]._replace(pi=dict(qs[1].pi, U=off_u))], a), (qs, a),
             ([qs[0]._replace(pi=dict(qs[0].pi, Ls=off_l)), qs[1]], a), (qs, a._replace(C=off_c)),
             (qs, a._replace(C=np.zeros(8, dtype=np.uint64))), (qs, a)]
    with fs.tuning(poseidon_lanes=lanes):
        verdict, first_bad, *_ = acc.verifier_codes([p[0] for p in pairs], [p[1] for p in pairs], 15, cname)
    assert verdict.tolist() == [ACCEPT, INSTANCE, ACCEPT, INSTANCE, C_BAR, C_BAR, ACCEPT]
    assert first_bad.tolist() == [2, 1, 2, 0, 2, 2, 2]


# ---------------------------------------------------------------------------------------------
# 6. lg n = 0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", CURVES)
def test_no_round(fs, golden, corc, cname, lanes):
    """d = 0: C = (0, 0) with v = c = 0 passes the succinct check (C + e H - c U with e = xi_0 (v - c h(z)) = 0) whatever
    U is.  alpha, z' against the oracle's ASDL walk over the oracle's xi_0, C_bar' against the host lincomb,
    v' = 1 + alpha (the accumulation's h_j of no round is 1)."""
    use_srs(corc, golden, cname, 2)
    m = P.CURVES[cname].scalar
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    empty = np.zeros((0, 8), dtype=np.uint64)
    zs, zero = det_scalars(1300, 2), np.zeros(4, dtype=np.uint64)
    qs = [pcdl.Instance(np.zeros(8, dtype=np.uint64), 0, zs[j], zero,
                        {"Ls": empty, "Rs": empty, "U": srs[2 + j].copy(), "c": zero, "C_bar": None, "w_prime": None})
          for j in range(2)]
    t = SpongeAdapter(cname, "ASDL")
    t.absorb_fr([x for q in qs for x in oracle_transcript(cname, golden, q.C, q.z, q.v, q.pi)[1]])
    t.absorb_g([q.pi["U"] for q in qs])
    alpha, z_prime = t.challenge(), t.challenge()
    with fs.tuning(poseidon_lanes=lanes):
        verdict, first_bad, asdl, C_bar, v = acc.verifier_codes([qs], None, 0, cname)
        assert verdict.tolist() == [ACCEPT] and first_bad.tolist() == [2]
        assert np.array_equal(asdl[0, 0], alpha) and np.array_equal(asdl[0, 1], z_prime)
        one = fe(1, m)
        assert np.array_equal(C_bar[0], pcdl.point_lincomb(np.stack([q.pi["U"] for q in qs])[None], np.stack([one, alpha])[None],
                                                           curve=cname)[0])
        assert np.array_equal(v[0], fe(1 + P.from_mont(P.limbs_to_int(alpha), m), m))
        a = pcdl.Instance(C_bar[0], 0, z_prime, v[0], None)
        bad = [qs[0], qs[1]._replace(v=plus_one(qs[1].v, m))]
        verdict, first_bad, asdl2, *_ = acc.verifier_codes([qs, bad, qs], [a, a, a._replace(v=plus_one(a.v, m))], 0, cname)
    assert verdict.tolist() == [ACCEPT, INSTANCE, V] and first_bad.tolist() == [2, 1, 2]
    assert np.array_equal(asdl2[0], asdl[0]) and np.array_equal(asdl2[2], asdl[0])


# ---------------------------------------------------------------------------------------------
# 7. the device-pointer form
# ---------------------------------------------------------------------------------------------
def run_dev(fs, cname, d, groups, accs):
    """halo_acc_verifier_batch_dev over torch buffers on the current stream."""
    import torch
    k, m = len(groups), len(groups[0])

    def dev(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.uint8 if a.dtype == np.uint8 else np.int64)).cuda()

    bufs = [dev(a) for a in pcdl.instance_rows([q for g in groups for q in g], d)]
    bufs += [dev(np.stack([a.C for a in accs])), dev(np.stack([a.z for a in accs])), dev(np.stack([a.v for a in accs]))]
    d_verdict = torch.full((k,), 9, dtype=torch.uint8, device="cuda")
    d_fb = torch.full((k,), 9, dtype=torch.int32, device="cuda")
    d_asdl = torch.zeros(k * 8, dtype=torch.int64, device="cuda")
    d_cb = torch.zeros(k * 8, dtype=torch.int64, device="cuda")
    d_v = torch.zeros(k * 4, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fs.check(fs.load().halo_acc_verifier_batch_dev(
        fs.CURVES[cname], d, k, m, *[b.data_ptr() if b is not None else None for b in bufs], d_verdict.data_ptr(),
        d_fb.data_ptr(), d_asdl.data_ptr(), d_cb.data_ptr(), d_v.data_ptr(), ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    return (d_verdict.cpu().numpy(), d_fb.cpu().numpy().view(np.uint32), d_asdl.cpu().numpy().view(np.uint64).reshape(k, 2, 4),
            d_cb.cpu().numpy().view(np.uint64).reshape(k, 8), d_v.cpu().numpy().view(np.uint64).reshape(k, 4))


@pytest.mark.parametrize("cname", CURVES)
def test_dev_form_equals_the_host_form(fs, golden, corc, cases, cname):
    use_srs(corc, golden, cname, 16)
    cs = cases[cname]
    names = tampered_batch(cs, 67)
    groups, accs = [cs[n][0] for n in names], [cs[n][1] for n in names]
    host = acc.verifier_codes(groups, accs, 15, cname)
    dev = run_dev(fs, cname, 15, groups, accs)
    assert dev[0].tolist() == host[0].tolist() == [cs[n][2][0] for n in names]
    for h, g in zip(host[1:], dev[1:]):
        assert np.array_equal(h, g)


@pytest.mark.parametrize("cname,which,code", [("pallas", "c", INSTANCE), ("vesta", "z", INSTANCE), ("pallas", "acc_z", Z),
                                              ("vesta", "acc_v", V)])
def test_dev_form_scalar_not_below_the_modulus(fs, golden, corc, cases, cname, which, code):
    use_srs(corc, golden, cname, 16)
    qs, a, _ = cases[cname]["good"]
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    bq, ba = list(qs), a
    if which == "c":
        bq[1] = qs[1]._replace(pi=dict(qs[1].pi, c=big))
    elif which == "z":
        bq[1] = qs[1]._replace(z=big)
    else:
        ba = a._replace(**{which[4:]: big})
    verdict, first_bad, asdl, _, v = run_dev(fs, cname, 15, [qs, bq, qs], [a, ba, a])
    assert verdict.tolist() == [ACCEPT, code, ACCEPT]
    assert first_bad.tolist() == [2, 1 if code == INSTANCE else 2, 2]
    for i in (0, 2):
        assert np.array_equal(asdl[i, 1], a.z) and np.array_equal(v[i], a.v)


# ---------------------------------------------------------------------------------------------
# 8. halo_acc_prover with one failing instance
# ---------------------------------------------------------------------------------------------
def test_prover_with_a_failing_instance(fs, golden, corc, inst, cases):
    cname = "pallas"
    use_srs(corc, golden, cname, 16)
    qs = [inst[cname][0], cases[cname]["c1"][0][1], inst[cname][2]]
    rows = pcdl.instance_rows(qs, 15)
    outs = [np.full(s, 0x77, dtype=np.uint64) for s in ((8,), (4,), (4,), (4, 8), (4, 8), (8,), (4,))]
    verdict, first_bad = np.full(1, 9, dtype=np.uint8), np.full(1, 9, dtype=np.uint32)
    rc = fs.load().halo_acc_prover(fs.CURVES[cname], 15, 3, *[fs.ptr(a) for a in rows], *[fs.ptr(o) for o in outs],
                                   fs.ptr(verdict), fs.ptr(first_bad))
    assert rc == 0 and verdict.tolist() == [INSTANCE] and first_bad.tolist() == [1]
    assert all((o == 0x77).all() for o in outs)
    with pytest.raises(pcdl.CheckFailed, match="instance 1"):
        acc.prover_device(qs, curve=cname)
    # the session pool stays usable
    good = [inst[cname][i] for i in (0, 1, 2)]
    same_accumulator(acc.prover_device(good, curve=cname), oracle_prover(cname, "n16_m3", good)[0])
    ins = det_scalars(1400, 17)
    C = pcdl.commit(ins[:16], 15, curve=cname)
    pi = pcdl.open(ins[:16], C, 15, ins[16], transcript=SpongeAdapter(cname), curve=cname)
    pcdl.check(C, 15, ins[16], pi["v"], pi, SpongeAdapter(cname), curve=cname)


# ---------------------------------------------------------------------------------------------
# 9. the backend
# ---------------------------------------------------------------------------------------------
def test_backend_parity(fs, golden, corc, inst):
    from halo_amd.prover import DeviceBackend
    cname = "pallas"
    use_srs(corc, golden, cname, 16)
    B1 = DeviceBackend(cname, device_transcripts=True, device_acc=True)
    B0 = DeviceBackend(cname, device_transcripts=True, device_acc=False)
    qs = [{"C": q.C, "z": B0.to_int(q.z), "v": B0.to_int(q.v), "Ls": list(q.pi["Ls"]), "Rs": list(q.pi["Rs"]), "U": q.pi["U"],
           "c": B0.to_int(q.pi["c"])} for q in inst[cname][:3]]
    a1, a0 = B1.acc_prove(qs, 15, transcripts(cname)), B0.acc_prove(qs, 15, transcripts(cname))
    assert a1["z"] == a0["z"] and a1["v"] == a0["v"] and a1["c"] == a0["c"]
    assert np.array_equal(a1["C"], a0["C"]) and np.array_equal(a1["U"], a0["U"])
    assert all(np.array_equal(x, y) for x, y in zip(a1["Ls"], a0["Ls"]))
    assert all(np.array_equal(x, y) for x, y in zip(a1["Rs"], a0["Rs"])) and len(a1["Ls"]) == len(a0["Ls"]) == 4


# ---------------------------------------------------------------------------------------------
# 10. HALO_ESRSRANGE: d above the resident SRS, and an SRS without (S, H)
# ---------------------------------------------------------------------------------------------
ESRSRANGE = 5
ENTRY_POINTS = ("halo_acc_verifier_batch", "halo_acc_verifier_batch_dev", "halo_acc_prover")


def raw_calls(H, cid, d):
    """The three entry points called directly with k = 1, m = 2 and arrays of well-formed values (the identity for
    every point, 1 for every scalar): [(name, status, halo_last_error(), the outputs are as they were)]."""
    import torch
    lg = (d + 1).bit_length() - 1
    pts, fes = np.zeros((2 * max(lg, 1), 8), dtype=np.uint64), np.ones((2 * max(lg, 1), 4), dtype=np.uint64)
    d_pts, d_fes = torch.from_numpy(pts.view(np.int64)).cuda(), torch.from_numpy(fes.view(np.int64)).cuda()
    L, out = H.load(), []

    def host_args(p, f):
        return [p, f, f, p, p, p, f, None, None, None]

    # verifier, host arrays
    verdict, fb = np.full(1, 9, dtype=np.uint8), np.full(1, 9, dtype=np.uint32)
    rc = L.halo_acc_verifier_batch(cid, d, 1, 2, *host_args(H.ptr(pts), H.ptr(fes)), H.ptr(pts), H.ptr(fes), H.ptr(fes),
                                   H.ptr(verdict), H.ptr(fb), None, None, None)
    out.append((ENTRY_POINTS[0], rc, H.last_error(), verdict.tolist() == [9] and fb.tolist() == [9]))
    # verifier, device pointers
    d_verdict = torch.full((1,), 9, dtype=torch.uint8, device="cuda")
    p, f = d_pts.data_ptr(), d_fes.data_ptr()
    rc = L.halo_acc_verifier_batch_dev(cid, d, 1, 2, *host_args(p, f), p, f, f, d_verdict.data_ptr(), None, None, None, None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = H.last_error()
    torch.cuda.synchronize()
    out.append((ENTRY_POINTS[1], rc, msg, d_verdict.cpu().tolist() == [9]))
    # prover
    outs = [np.full(s, 0x77, dtype=np.uint64) for s in ((8,), (4,), (4,), (max(lg, 1), 8), (max(lg, 1), 8), (8,), (4,))]
    verdict, fb = np.full(1, 9, dtype=np.uint8), np.full(1, 9, dtype=np.uint32)
    rc = L.halo_acc_prover(cid, d, 2, *host_args(H.ptr(pts), H.ptr(fes)), *[H.ptr(o) for o in outs], H.ptr(verdict), H.ptr(fb))
    out.append((ENTRY_POINTS[2], rc, H.last_error(),
                all((o == 0x77).all() for o in outs) and verdict.tolist() == [9] and fb.tolist() == [9]))
    return out


@pytest.mark.parametrize("cname", CURVES)
def test_d_above_the_srs(fs, golden, corc, cname):
    """D = 15 resident, d = 2 D + 1 = 31: every entry point answers with the reference's text and writes nothing."""
    use_srs(corc, golden, cname, 16)
    for name, rc, msg, untouched in raw_calls(fs, fs.CURVES[cname], 31):
        assert rc == ESRSRANGE and "d was larger than D!" in msg and untouched, (name, rc, msg)
    for name, rc, msg, _ in raw_calls(fs, fs.CURVES[cname], 15):  # and the same calls within D go through
        assert rc == 0, (name, rc, msg)


_NO_SH_CHILD = r"""
import json, os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, "oracle"), {tests!r}]
import numpy as np
from halo_amd import _lib as H
from halo_amd import schnorr
import test_gpu_acc_fs as T
H.ensure_device()
g = np.load(os.path.join({tests!r}, "golden", "transcript.npz"))
for f in ("fp", "fq"):
    schnorr.set_poseidon_params(f, g["poseidon_" + f + "_mds"], g["poseidon_" + f + "_rc"])
out = {{}}
for cname, cid in H.CURVES.items():
    H.check(H.load().halo_srs_synthesize(cid, 16, 7))  # a resident SRS, and no (S, H) in this process
    out[cname] = [[name, rc, msg, bool(ok)] for name, rc, msg, ok in T.raw_calls(H, cid, 15)]
print("RESULT " + json.dumps(out))
"""


def test_refused_without_s_and_h(fs):
    """(S, H) stay resident for the life of a process once any test has uploaded them, so the refusal is taken in a
    fresh process that only synthesizes an SRS (as tests/test_gpu_hiding.py does for the hiding commitment)."""
    import json
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    r = subprocess.run([sys.executable, "-c", _NO_SH_CHILD.format(root=root, tests=tests)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    for cname, calls in json.loads(line[7:]).items():
        assert [c[0] for c in calls] == list(ENTRY_POINTS)
        for name, rc, msg, untouched in calls:
            assert rc == ESRSRANGE and "(S, H)" in msg and name in msg and untouched, (cname, name, rc, msg)
