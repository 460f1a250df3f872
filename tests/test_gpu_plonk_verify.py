"""GPU tests of PlonkProof::verify_succinct / verify on the device (halo_amd/csrc/plonk_verify.hip behind
halo_plonk_verify_succinct_batch and its _dev form; halo_amd.plonk), against the big-integer restatement of
tests/plonk_ref.py:

  * the committed two-step chains of tests/golden/plonk_proofs.npz (Pallas n = 8 and 64, Vesta n = 16): accepted by
    verify_succinct and verify, every challenge and both sides of the identity bit for bit;
  * one field tampered at a time: the restatement's verdict code and the reference's message;
  * batches of 1, 3, 22 and 65 proofs (22 crosses a three-lane wave of 21 sponges, 65 a one-lane wave) mixing
    accepts and every reject kind, both lane layouts, the host and the device-pointer entry;
  * the gate algebra alone on random, all-zero and all r - 1 evaluations with 0, 2 and 5 public inputs (the
    affine-mul and range-check terms, which the fixture circuit leaves at q = 0);
  * the error codes and the empty batch;
  * a round trip: naive_prover on the device under the reference's transcripts at n = 2^10, then plonk.verify."""
import ctypes
import os

import numpy as np
import pytest

import pasta as P
import plonk_ref as R
from halo_amd import group, pcdl, plonk

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
G = np.load(os.path.join(HERE, "golden", "plonk_proofs.npz"))
T = np.load(os.path.join(HERE, "golden", "transcript.npz"))
LANES = [1, 3]
FIELDS = ("C_ws", "C_z", "C_ts", "vs", "Ls", "Rs", "U", "c")


@pytest.fixture(scope="module")
def pv(hal, golden):
    """The reference's Poseidon constants for both fields and the SRS recipe's first 64 points for both curves."""
    from halo_amd import schnorr
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, T[f"poseidon_{f}_mds"], T[f"poseidon_{f}_rc"])
    for cname in ("pallas", "vesta"):
        S, Hh = golden[f"ref_sh_{cname}"]
        group.PublicParams.upload(cname, np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"]), S, Hh,
                                  precompute_windows=True)
    return hal


def mds_ark(cname):
    m = P.CURVES[cname].scalar
    return np.stack([R.fe(x, m) for row in R.scalar_mds(cname) for x in row])


def arrays(recs):
    """The per-proof arguments of the call, stacked."""
    a = {f: np.ascontiguousarray(np.stack([getattr(r, f) for r in recs])) for f in FIELDS}
    a["pub"] = np.ascontiguousarray(np.stack([r.pub for r in recs]))
    for name, src in (("prev", "prev"), ("next", "next")):
        s = np.stack([getattr(r, src) for r in recs])
        a[name + "_C"], a[name + "_z"], a[name + "_v"] = (np.ascontiguousarray(s[:, :8]), np.ascontiguousarray(s[:, 8:12]),
                                                          np.ascontiguousarray(s[:, 12:]))
    return a


def run_batch(hal, cname, rows, C_qs, recs, dev=False):
    """One call over k Recs: (verdict (k,), challenges (k, 5, 4), sides (k, 2, 4), asdl (k, 2, 4))."""
    k = len(recs)
    a = arrays(recs)
    npi = a["pub"].shape[1]
    ins = [np.ascontiguousarray(C_qs), a["pub"] if npi else None] + [a[f] for f in FIELDS] + \
        [a["prev_C"], a["prev_z"], a["prev_v"], a["next_C"], a["next_z"], a["next_v"], mds_ark(cname)]
    outs = [np.full(k, 77, dtype=np.uint8), np.zeros((k, 5, 4), dtype=np.uint64), np.zeros((k, 2, 4), dtype=np.uint64),
            np.zeros((k, 2, 4), dtype=np.uint64)]
    L = hal.load()
    if not dev:
        p = [hal.ptr(x) for x in ins]
        hal.check(L.halo_plonk_verify_succinct_batch(hal.CURVES[cname], rows, k, p[0], p[1], npi, *p[2:],
                                                     *[hal.ptr(x) for x in outs]))
        return outs
    import torch
    d_in = [None if x is None else torch.from_numpy(x.view(np.int64)).cuda() for x in ins]
    d_out = [torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in outs]
    p = [None if t is None else t.data_ptr() for t in d_in]
    hal.check(L.halo_plonk_verify_succinct_batch_dev(hal.CURVES[cname], rows, k, p[0], p[1], npi, *p[2:],
                                                     *[t.data_ptr() for t in d_out],
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return [t.cpu().numpy().view(o.dtype).reshape(o.shape) for t, o in zip(d_out, outs)]


def restated(cname, rows, C_qs, golden, rec):
    m = P.CURVES[cname].scalar
    code, rb = R.verify_succinct(cname, rows, C_qs, golden[f"ref_sh_{cname}"][1], rec)
    return code, {k: None if v is None else np.stack([R.fe(x, m) for x in v]) for k, v in rb.items()}


def as_proof(rec, rows):
    """(PlonkProof, public inputs, acc_prev) of halo_amd.plonk from a Rec."""
    def pi(j):
        return {"Ls": rec.Ls[j], "Rs": rec.Rs[j], "U": rec.U[j], "c": rec.c[j], "C_bar": None, "w_prime": None}
    Ls, Rs, U, c = rec.next_pi
    vs = plonk.PlonkProofEvals(rec.vs[0:16], rec.vs[16:31], rec.vs[31:41], rec.vs[41:57], rec.vs[57:65], rec.vs[65:73],
                               rec.vs[73], rec.vs[74], rec.vs[75:78])
    acc_next = pcdl.Instance(rec.next[:8], rows - 1, rec.next[8:12], rec.next[12:],
                             {"Ls": Ls, "Rs": Rs, "U": U, "c": c, "C_bar": None, "w_prime": None})
    proof = plonk.PlonkProof(vs, plonk.PlonkProofCommitments(rec.C_ws, rec.C_ts, rec.C_z),
                             plonk.PlonkProofEvalProofs(pi(1), pi(2)), acc_next)
    return proof, rec.pub, pcdl.Instance(rec.prev[:8], rows - 1, rec.prev[8:12], rec.prev[12:], pi(0))


def circuit_of(cname, rows, C_qs, npi=2):
    return plonk.PlonkCircuit(rows, C_qs, npi, mds_ark(cname))


# ---------------------------------------------------------------------------------------------
# 1. the committed chains
# ---------------------------------------------------------------------------------------------
def test_fixtures_contain_an_identity_commitment():
    for key in R.CHAINS:
        _, recs = R.load_chain(G, key)
        assert all(any(not w.any() for w in rec.C_ts) for rec in recs), key


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("key", sorted(R.CHAINS))
def test_fixtures_accepted_bit_exact(pv, key, lanes):
    cname, rows = R.CHAINS[key]
    C_qs, recs = R.load_chain(G, key)
    with pv.tuning(poseidon_lanes=lanes):
        verdict, chal, sides, asdl = run_batch(pv, cname, rows, C_qs, recs)
        assert verdict.tolist() == [0, 0]
        for step in range(2):
            assert np.array_equal(chal[step], G[f"{key}_{step}_challenges"]), (key, step)
            assert np.array_equal(sides[step], G[f"{key}_{step}_sides"]), (key, step)
            assert np.array_equal(asdl[step], G[f"{key}_{step}_asdl"]), (key, step)
            assert np.array_equal(sides[step][0], sides[step][1])
            proof, pub, prev = as_proof(recs[step], rows)
            plonk.verify_succinct(proof, circuit_of(cname, rows, C_qs), pub, prev, curve=cname)
            plonk.verify(proof, circuit_of(cname, rows, C_qs), pub, prev, curve=cname)


# ---------------------------------------------------------------------------------------------
# 2. tampering
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(R.TAMPERINGS))
@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_tampered_field(pv, golden, key, kind):
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(G, key)
    bad = R.tamper(recs[1], kind, m)
    want = R.TAMPERINGS[kind]
    code, _ = restated(cname, rows, C_qs, golden, bad)
    assert code == want
    verdict = run_batch(pv, cname, rows, C_qs, [recs[1], bad, recs[0]])[0]
    assert verdict.tolist() == [0, want, 0]  # its neighbours are left alone
    proof, pub, prev = as_proof(bad, rows)
    circuit = circuit_of(cname, rows, C_qs)
    if kind == "next_pi_c":
        plonk.verify_succinct(proof, circuit, pub, prev, curve=cname)
        with pytest.raises(pcdl.CheckFailed) as e:
            plonk.verify(proof, circuit, pub, prev, curve=cname)
        assert e.value.msg == pcdl.SUCCINCT_MSG
        return
    with pytest.raises(pcdl.CheckFailed) as e:
        plonk.verify_succinct(proof, circuit, pub, prev, curve=cname)
    assert e.value.msg == plonk.MESSAGES[want]
    if plonk.INSTANCE_0 <= want <= plonk.INSTANCE_2:
        assert e.value.index == want - plonk.INSTANCE_0 and e.value.msg == pcdl.SUCCINCT_MSG
    if want == plonk.IDENTITY:
        assert e.value.msg.startswith("T(𝔷) ≠ (F_GC(𝔷) + α F_CC1(𝔷)")


@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_swapped_selector_commitment(pv, golden, key):
    """C_qs[0] and C_qs[1] swapped: the transcript is the same, C_r is another point -> instance 1."""
    cname, rows = R.CHAINS[key]
    C_qs, recs = R.load_chain(G, key)
    C_bad = C_qs.copy()
    C_bad[0], C_bad[1] = C_qs[1], C_qs[0]
    assert restated(cname, rows, C_bad, golden, recs[0])[0] == R.INSTANCE_1
    assert run_batch(pv, cname, rows, C_bad, recs)[0].tolist() == [R.INSTANCE_1] * 2
    proof, pub, prev = as_proof(recs[0], rows)
    with pytest.raises(pcdl.CheckFailed) as e:
        plonk.verify(proof, circuit_of(cname, rows, C_bad), pub, prev, curve=cname)
    assert e.value.msg == pcdl.SUCCINCT_MSG and e.value.index == 1


def test_public_input_count_is_checked_before_the_device(pv):
    C_qs, recs = R.load_chain(G, "pallas_n8")
    proof, pub, prev = as_proof(recs[0], 8)
    with pytest.raises(pcdl.CheckFailed, match="public_input_count"):
        plonk.verify_succinct(proof, circuit_of("pallas", 8, C_qs, npi=3), pub, prev)


# ---------------------------------------------------------------------------------------------
# 3. batches
# ---------------------------------------------------------------------------------------------
def mixed_batch(key, k):
    """k proofs, every other one tampered with the next kind of TAMPERINGS (so that accepts and the reject
    kinds meet inside one wave), and the last one."""
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(G, key)
    kinds = sorted(R.TAMPERINGS)
    items = []
    for i in range(k):
        rec = recs[(i // 2) % 2]
        if i % 2 == 1 or i == k - 1:
            rec = R.tamper(rec, kinds[(i // 2) % len(kinds)], m)
        items.append(rec)
    return cname, rows, C_qs, items


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("k", [1, 3, 22, 65])
@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_batches(pv, golden, key, k, lanes):
    cname, rows, C_qs, items = mixed_batch(key, k)
    exp = [restated(cname, rows, C_qs, golden, rec)[0] for rec in items]
    if k >= 22:
        assert {0, 1, 2, 3, 4, 5, 6, 7, 8} <= set(exp)
    with pv.tuning(poseidon_lanes=lanes):
        host = run_batch(pv, cname, rows, C_qs, items)
        dev = run_batch(pv, cname, rows, C_qs, items, dev=True)
    assert host[0].tolist() == exp
    assert dev[0].tolist() == exp
    for i, rec in enumerate(items):
        if exp[i] == R.MALFORMED:
            continue
        rb = restated(cname, rows, C_qs, golden, rec)[1]
        for got in (host, dev):
            assert np.array_equal(got[1][i], rb["challenges"]) and np.array_equal(got[2][i], rb["sides"]), i
            assert np.array_equal(got[3][i], rb["asdl"]), i


# ---------------------------------------------------------------------------------------------
# 4. the gate algebra
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npi", [0, 2, 5])
@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_gate_algebra(pv, golden, key, npi):
    """Evaluations that satisfy nothing: every q is nonzero, so all five custom gates count."""
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(G, key)
    rng = np.random.default_rng(40 + npi)
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    rnd = lambda n: np.stack([R.fe(int.from_bytes(rng.bytes(32), "little"), m) for _ in range(n)]).reshape(n, 4)  # noqa: E731
    items = []
    for j, vs in enumerate((rnd(78), rnd(78), np.zeros((78, 4), dtype=np.uint64), np.tile(R.fe(m - 1, m), (78, 1)))):
        pts = srs[rng.permutation(64)]
        items.append(recs[j % 2]._replace(vs=vs, pub=rnd(npi) if npi else np.zeros((0, 4), dtype=np.uint64),
                                          C_ws=pts[:16].copy(), C_z=pts[16].copy(), C_ts=pts[17:33].copy()))
    verdict, chal, sides, _ = run_batch(pv, cname, rows, C_qs, items)
    for i, rec in enumerate(items):
        code, rb = restated(cname, rows, C_qs, golden, rec)
        assert verdict[i] == code != 0
        assert np.array_equal(chal[i], rb["challenges"]), i
        assert np.array_equal(sides[i], rb["sides"]), i


# ---------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------
def test_error_codes(pv, golden):
    cname, rows = "pallas", 8
    C_qs, recs = R.load_chain(G, "pallas_n8")
    assert run_batch(pv, cname, rows, C_qs, recs)[0].tolist() == [0, 0]
    with pytest.raises(AssertionError, match=r"n \(12\) is not a power of two"):
        run_batch(pv, cname, 12, C_qs, recs)
    wide = [r._replace(Ls=np.zeros((3, 7, 8), dtype=np.uint64), Rs=np.zeros((3, 7, 8), dtype=np.uint64)) for r in recs]
    for dev in (False, True):
        with pytest.raises(AssertionError, match="d was larger than D!"):
            run_batch(pv, cname, 128, C_qs, wide, dev=dev)
    with pytest.raises(pv.HaloError, match="2 rows"):
        run_batch(pv, cname, 2, C_qs, recs)
    big = recs[1].vs.copy()
    big[5] = 0xFFFFFFFFFFFFFFFF
    with pytest.raises(pv.HaloError, match="proof 1 is not below the modulus"):
        run_batch(pv, cname, rows, C_qs, [recs[0], recs[1]._replace(vs=big)])
    assert run_batch(pv, cname, rows, C_qs, [recs[0], recs[1]._replace(vs=big), recs[0]], dev=True)[0].tolist() == \
        [0, R.MALFORMED, 0]
    L = pv.load()
    assert L.halo_plonk_verify_succinct_batch(0, 8, 0, *([None] * 2), 0, *([None] * 19)) == 0
    assert L.halo_plonk_verify_succinct_batch_dev(0, 12, 0, *([None] * 2), 0, *([None] * 20)) == 0
    assert plonk.verify_succinct_batch(circuit_of(cname, rows, C_qs), [], [], []).tolist() == []


# ---------------------------------------------------------------------------------------------
# 6. prove on the device, verify on the device
# ---------------------------------------------------------------------------------------------
def test_round_trip_from_the_device_prover(pv, golden, corc):
    from halo_amd.prover import DeviceBackend, naive_prover
    cname, n = "pallas", 1 << 10
    m = P.CURVES[cname].scalar
    S, Hh = golden[f"ref_sh_{cname}"]
    srs = corc.srs_generate(cname, n)
    group.PublicParams.upload(cname, srs, S, Hh, precompute_windows=True)
    try:
        B = DeviceBackend(cname)
        host = R.satisfiable_circuit(R.CpuBackend(cname, srs[:1], S, Hh), n, seed=5, cname=cname)
        wit = {k: [B.from_ints(p) for p in host[k]] for k in ("qs", "ws", "rs", "ids", "sigmas")}
        wit["w_evals"] = [B.ntt(p, n) for p in wit["ws"]]
        wit["public_inputs"], wit["mds"] = host["public_inputs"], host["mds"]
        nt = R.new_transcript(cname)
        rng = np.random.default_rng(6)
        p0 = B.from_ints([int.from_bytes(rng.bytes(32), "little") % m for _ in range(n)])
        acc_prev = B.acc_prove([B.instance_open(p0, n - 1, 12345, nt)], n - 1, nt)
        out = naive_prover(B, wit, n, None, acc_prev=acc_prev, transcript=nt)
        C_qs = np.stack(B.commit_many(wit["qs"]))
        proof = plonk.PlonkProof.from_prover(out, cname)
        circuit = circuit_of(cname, n, C_qs)
        pub = np.stack([R.fe(x, m) for x in host["public_inputs"]])
        prev = pcdl.Instance(acc_prev["C"], n - 1, R.fe(acc_prev["z"], m), R.fe(acc_prev["v"], m),
                             {"Ls": np.stack(acc_prev["Ls"]), "Rs": np.stack(acc_prev["Rs"]), "U": acc_prev["U"],
                              "c": R.fe(acc_prev["c"], m), "C_bar": None, "w_prime": None})
        plonk.verify(proof, circuit, pub, prev, curve=cname)
        verdict, chal, _, _ = plonk.verify_succinct_batch(circuit, [pub], [prev], [proof], cname, readbacks=True)
        rec = R.rec_from_prover(B, out, acc_prev, host["public_inputs"])
        code, rb = restated(cname, n, C_qs, golden, rec)
        assert code == 0 and verdict.tolist() == [0]
        assert np.array_equal(chal[0], rb["challenges"])
        flipped = proof._replace(vs=proof.vs._replace(z=R.plus_one(proof.vs.z, m)))
        with pytest.raises(pcdl.CheckFailed) as e:
            plonk.verify(flipped, circuit, pub, prev, curve=cname)
        assert e.value.msg == plonk.IDENTITY_MSG
    finally:
        group.PublicParams.upload(cname, np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"]), S, Hh,
                                  precompute_windows=True)
