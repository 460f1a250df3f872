"""GPU tests of the Fiat-Shamir sponge as an object (halo_amd/csrc/sponge.hip behind halo_sponge_*; halo_amd.sponge)
and of the prover's PLONK transcript on it (``DeviceBackend(device_plonk=True)``), bit for bit against
oracle/poseidon.Sponge (pinned to the reference's vectors by tests/test_oracle.py).  No tolerance is involved.

  1. every mode transition, both curves, both lane layouts, the four labels; a seeded walk of 40 operations;
  2. one absorb call against three, and against three that change the lane layout between calls;
  3. the committed PLONK and PCDL transcripts and halo_amd.schnorr's batched hash;
  4. lockstep batches of 1, 3, 22 and 65 sponges (22 crosses a three-lane wave of 21 sponges, 65 a one-lane wave), the
     host and the device-pointer forms;
  5. reset() and handle reuse;
  6. the sponge dropped into pcdl.open and halo_amd.acc;
  7. naive_prover with its PLONK sponge on the device: bit identity with the host sponge, and a round trip;
  8. the errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pasta as P
import plonk_ref as R
import poseidon
from halo_amd import acc, group, pcdl, plonk, schnorr, sponge

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T = np.load(os.path.join(HERE, "golden", "transcript.npz"))
PROOFS = np.load(os.path.join(HERE, "golden", "plonk_proofs.npz"))
CURVES = ["pallas", "vesta"]
LANES = [1, 3]
LABELS = {"PCDL": poseidon.PCDL, "ASDL": poseidon.ASDL, "PLONK": poseidon.PLONK, "SIGNATURE": poseidon.SIGNATURE}
EINVAL = 1


@pytest.fixture(scope="module")
def sp(hal):
    """The reference's Poseidon constants installed for both fields."""
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, T[f"poseidon_{f}_mds"], T[f"poseidon_{f}_rc"])
    return hal


def use_srs(corc, golden, cname, n):
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, corc.srs_generate(cname, n), S, Hh, precompute_windows=True)


class Oracle:
    """oracle/poseidon.Sponge behind halo_amd.sponge.Sponge's interface (R.SpongeAdapter's conversions, any label,
    absorb_fq and reset as outer_sponge.rs has them); ``squeezed`` keeps what the inner sponge gave each challenge."""

    def __init__(self, cname, label):
        self.cname, self.c = cname, P.CURVES[cname]
        self.a = R.SpongeAdapter(cname, "PCDL")
        self.a.s = poseidon.Sponge(cname, LABELS[label])
        self.squeezed = []
        self._tap()

    def _tap(self):
        inner, log = self.a.s.inner, self.squeezed
        plain = inner.squeeze

        def squeeze():
            log.append(plain())
            return log[-1]
        inner.squeeze = squeeze

    def absorb_g(self, pts):
        self.a.absorb_g(np.asarray(pts, dtype=np.uint64).reshape(-1, 8))

    def absorb_fr(self, xs):
        self.a.absorb_fr(np.asarray(xs, dtype=np.uint64).reshape(-1, 4))

    def absorb_fq(self, xs):
        self.a.s.inner.absorb([R.to_int(x, self.c.base) for x in np.asarray(xs, dtype=np.uint64).reshape(-1, 4)])

    def challenge(self):
        return self.a.challenge()

    def reset(self):  # outer_sponge.rs:97-99: a fresh inner sponge, no label
        self.a.s.inner = poseidon.InnerSponge("fq" if self.cname == "pallas" else "fp")
        self._tap()


def base_fe(cname, xs):
    return np.stack([R.fe(x, P.CURVES[cname].base) for x in xs])


def scalar_fe(cname, xs):
    return np.stack([R.fe(x, P.CURVES[cname].scalar) for x in xs])


def rand_ints(rng, m, k):
    return [int.from_bytes(rng.bytes(32), "little") % m for _ in range(k)]


def both(cname, label):
    return sponge.Sponge(cname, label), Oracle(cname, label)


def same_challenge(dev, ora, what=None):
    got, exp = dev.challenge(), ora.challenge()
    assert got.shape == (4,) and got.dtype == np.uint64 and np.array_equal(got, exp), what


# ---------------------------------------------------------------------------------------------
# 1. mode transitions
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("label", sorted(LABELS))
@pytest.mark.parametrize("cname", CURVES)
def test_mode_transitions(sp, cname, label, lanes):
    xs = base_fe(cname, [3, 1 << 200, 5, 7, 11, 13, 17])
    with sp.tuning(poseidon_lanes=lanes):
        d, o = both(cname, label)
        same_challenge(d, o, "straight after new")
        for count in (1, 2, 3, 4):  # Absorbed(1) + count: below, at and past the rate
            d, o = both(cname, label)
            d.absorb_fq(xs[:count])
            o.absorb_fq(xs[:count])
            same_challenge(d, o, count)
        d, o = both(cname, label)
        for j in range(3):  # Squeezed(1), Squeezed(2), then a permutation again
            same_challenge(d, o, ("in a row", j))
        for squeezes in (1, 2):  # an absorb after one squeeze and after two
            d, o = both(cname, label)
            for _ in range(squeezes):
                same_challenge(d, o)
            d.absorb_fq(xs[4:6])
            o.absorb_fq(xs[4:6])
            same_challenge(d, o, ("absorb after", squeezes))
            same_challenge(d, o)
        d.close()


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", CURVES)
def test_edge_values(sp, golden, cname, lanes):
    c = P.CURVES[cname]
    odd_top = c.scalar - 2 if (c.scalar - 2) & 1 else c.scalar - 3  # an odd scalar with its top bits set
    assert odd_top & 1 and odd_top >> 253
    gen = golden[f"ref_srs_{cname}_b00_first64"][0]
    assert gen.any()
    with sp.tuning(poseidon_lanes=lanes):
        d, o = both(cname, "PCDL")
        for s in (0, 1, c.scalar - 1, odd_top):
            d.absorb_fr(scalar_fe(cname, [s]))
            o.absorb_fr(scalar_fe(cname, [s]))
            same_challenge(d, o, ("fr", s))
        for pts in (np.zeros((1, 8), dtype=np.uint64), gen[None], np.stack([gen, np.zeros(8, dtype=np.uint64)])):
            d.absorb_g(pts)
            o.absorb_g(pts)
            same_challenge(d, o, "g")
        d.absorb_g_affine([gen])
        o.absorb_g([gen])
        for x in (0, c.base - 1):
            d.absorb_fq(base_fe(cname, [x]))
            o.absorb_fq(base_fe(cname, [x]))
            same_challenge(d, o, ("fq", x))
        d.absorb_fr(np.zeros((0, 4), dtype=np.uint64))  # n = 0: nothing happens
        same_challenge(d, o, "after an empty absorb")


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", CURVES)
def test_random_walk(sp, golden, cname, lanes):
    c = P.CURVES[cname]
    rng = np.random.default_rng(2024)
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    challenges = 0
    with sp.tuning(poseidon_lanes=lanes):
        d, o = both(cname, "ASDL")
        for step in range(40):
            op, count = int(rng.integers(0, 4)), int(rng.integers(1, 4))
            if op == 0:
                pts = srs[rng.integers(0, 64, size=count)]
                d.absorb_g(pts), o.absorb_g(pts)
            elif op == 1:
                xs = scalar_fe(cname, rand_ints(rng, c.scalar, count))
                d.absorb_fr(xs), o.absorb_fr(xs)
            elif op == 2:
                xs = base_fe(cname, rand_ints(rng, c.base, count))
                d.absorb_fq(xs), o.absorb_fq(xs)
            else:
                for _ in range(count):
                    same_challenge(d, o, step)
                    challenges += 1
        same_challenge(d, o, "last")
    assert challenges >= 5
    if cname == "vesta":  # the shift by one bit dropped a set bit at least once
        assert any(v & 1 for v in o.squeezed)


# ---------------------------------------------------------------------------------------------
# 2. splitting
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["g", "fr", "fq"])
@pytest.mark.parametrize("cname", CURVES)
def test_one_call_or_three(sp, golden, cname, kind):
    c = P.CURVES[cname]
    rng = np.random.default_rng(7)
    items = {"g": golden[f"ref_srs_{cname}_b00_first64"][3:6], "fr": scalar_fe(cname, rand_ints(rng, c.scalar, 3)),
             "fq": base_fe(cname, rand_ints(rng, c.base, 3))}[kind]
    outs = []
    for plan in ([(items, 1)], [(items[j:j + 1], 1) for j in range(3)], [(items[j:j + 1], (1, 3, 1)[j]) for j in range(3)],
                 [(items[j:j + 1], (3, 1, 3)[j]) for j in range(3)]):
        s = sponge.Sponge(cname, "PLONK")
        for part, lanes in plan:
            with sp.tuning(poseidon_lanes=lanes):
                getattr(s, "absorb_" + kind)(part)
        with sp.tuning(poseidon_lanes=plan[-1][1] ^ 2):  # 1 <-> 3
            outs.append(np.stack([s.challenge(), s.challenge(), s.challenge()]))
    o = Oracle(cname, "PLONK")
    getattr(o, "absorb_" + kind)(items)
    exp = np.stack([o.challenge() for _ in range(3)])
    assert all(np.array_equal(x, exp) for x in outs)


# ---------------------------------------------------------------------------------------------
# 3. fixtures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("key", sorted(R.CHAINS))
def test_plonk_fixture_transcripts(sp, key, lanes):
    cname, _ = R.CHAINS[key]
    _, recs = R.load_chain(PROOFS, key)
    with sp.tuning(poseidon_lanes=lanes):
        for step, rec in enumerate(recs):
            s = sponge.Sponge(cname, "PLONK")
            s.absorb_g(rec.C_ws)
            beta, gamma = s.challenge(), s.challenge()
            s.absorb_g([rec.C_z])
            alpha = s.challenge()
            s.absorb_g(rec.C_ts)
            zeta, xi = s.challenge(), s.challenge()
            exp = PROOFS[f"{key}_{step}_challenges"]
            assert exp.shape == (5, 4) and np.array_equal(np.stack([beta, gamma, alpha, zeta, xi]), exp), (key, step)


@pytest.mark.parametrize("lanes", LANES)
def test_pcdl_fixture_transcript(sp, lanes):
    key = "open_pallas_n16_plain"
    z, v = T[key + "_zv"]
    exp = T[key + "_xis"]
    assert exp.shape == (5, 4)
    with sp.tuning(poseidon_lanes=lanes):
        s = sponge.Sponge("pallas", "PCDL")
        s.absorb_g([T[key + "_C"][0]])
        s.absorb_fr([z, v])
        xis = [s.challenge()]
        for L, Rr in zip(T[key + "_Ls"], T[key + "_Rs"]):
            s.absorb_fr([xis[-1]])
            s.absorb_g([L, Rr])
            xis.append(s.challenge())
    assert np.array_equal(np.stack(xis), exp)


@pytest.mark.parametrize("cname", CURVES)
def test_signature_sponge_is_the_schnorr_hash(sp, golden, cname):
    rng = np.random.default_rng(11)
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    k = 3
    pk, Rp = srs[10:10 + k], srs[20:20 + k]
    msgs = np.stack([base_fe(cname, rand_ints(rng, P.CURVES[cname].base, 10)) for _ in range(k)])
    exp = schnorr.hash_message_batch(pk, Rp, msgs, curve=cname)
    for i in range(k):
        s = sponge.Sponge(cname, "SIGNATURE")
        s.absorb_g_affine([pk[i], Rp[i]])
        s.absorb_fq(msgs[i])
        assert np.array_equal(s.challenge(), exp[i]), i
    b = sponge.SpongeBatch(cname, "SIGNATURE", k)
    b.absorb_g(np.stack([pk, Rp], axis=1))
    b.absorb_fq(msgs)
    assert np.array_equal(b.challenge()[:, 0], exp)


# ---------------------------------------------------------------------------------------------
# 4. lockstep batches
# ---------------------------------------------------------------------------------------------
_BATCH = {}


def batch_case(golden, cname, k):
    """Distinct data per sponge and what k oracle sponges make of it: absorb_g of 2, absorb_fr of 1, two challenges,
    absorb_fq of 3, three challenges (the last one permutes again).  Once per (curve, k)."""
    if (cname, k) not in _BATCH:
        c = P.CURVES[cname]
        rng = np.random.default_rng(100 + k)
        srs = golden[f"ref_srs_{cname}_b00_first64"]
        pts = srs[rng.integers(0, 64, size=(k, 2))]
        pts[k // 2, 1] = 0  # an identity in the middle of the batch
        frs = np.stack([scalar_fe(cname, rand_ints(rng, c.scalar, 1)) for _ in range(k)])
        fqs = np.stack([base_fe(cname, rand_ints(rng, c.base, 3)) for _ in range(k)])
        first, second = [], []
        for i in range(k):
            o = Oracle(cname, "ASDL")
            o.absorb_g(pts[i])
            o.absorb_fr(frs[i])
            first.append([o.challenge(), o.challenge()])
            o.absorb_fq(fqs[i])
            second.append([o.challenge(), o.challenge(), o.challenge()])
        _BATCH[cname, k] = (np.ascontiguousarray(pts), frs, fqs, np.array(first, dtype=np.uint64), np.array(second, dtype=np.uint64))
    return _BATCH[cname, k]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("k", [1, 3, 22, 65])
@pytest.mark.parametrize("cname", CURVES)
def test_lockstep_batches(sp, golden, cname, k, lanes, dev):
    import torch
    pts, frs, fqs, first, second = batch_case(golden, cname, k)
    assert len({p.tobytes() for p in pts}) > k // 2 and len({x.tobytes() for x in frs}) == k
    with sp.tuning(poseidon_lanes=lanes):
        b = sponge.SpongeBatch(cname, "ASDL", k)
        if dev:
            up = lambda a: torch.from_numpy(a.view(np.int64)).cuda()  # noqa: E731
            down = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
            b.absorb_g_dev(up(pts))
            b.absorb_fr_dev(up(frs))
            got1 = down(b.challenge_dev(2))
            b.absorb_fq_dev(up(fqs))
            got2 = down(b.challenge_dev(3))
        else:
            b.absorb_g(pts)
            b.absorb_fr(frs)
            got1 = b.challenge(2)
            b.absorb_fq(fqs)
            got2 = b.challenge(3)
        b.close()
    assert got1.shape == (k, 2, 4) and got2.shape == (k, 3, 4)
    assert np.array_equal(got1, first) and np.array_equal(got2, second)  # sponge i is its own oracle sponge


# ---------------------------------------------------------------------------------------------
# 5. reset and handle reuse
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", CURVES)
def test_reset_and_a_new_handle(sp, golden, cname, lanes):
    gen = golden[f"ref_srs_{cname}_b00_first64"][1]
    with sp.tuning(poseidon_lanes=lanes):
        d, o = both(cname, "PLONK")
        d.absorb_g([gen]), o.absorb_g([gen])
        same_challenge(d, o)
        d.reset(), o.reset()
        after_reset = d.challenge()
        assert np.array_equal(after_reset, o.challenge())
        assert not np.array_equal(after_reset, sponge.Sponge(cname, "PLONK").challenge())  # no label was absorbed
        d.reset(), o.reset()
        d.absorb_fr(scalar_fe(cname, [5])), o.absorb_fr(scalar_fe(cname, [5]))
        d.absorb_g([gen]), o.absorb_g([gen])
        same_challenge(d, o, "a transcript after reset")
        # a handle made after a free does not see the freed one's state, and ids are not reused
        old = d._id
        d.close()
        n, on = both(cname, "PLONK")
        assert n._id > old
        same_challenge(n, on, "after a free")
        d.close()  # a second close is a no-op


# ---------------------------------------------------------------------------------------------
# 6. drop-in use
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["open_pallas_n16_plain", "open_pallas_n64_hiding"])
def test_drop_in_pcdl_open(sp, golden, corc, key):
    n = int(key.split("_")[2][1:])
    use_srs(corc, golden, "pallas", n)
    z, _ = T[key + "_zv"]
    w = q = w_bar = None
    if key.endswith("hiding"):
        (w, w_bar), q = T[key + "_w"], T[key + "_q"]
    pi = pcdl.open(T[key + "_p"], T[key + "_C"][0], n - 1, z, w=w, transcript=sponge.Sponge("pallas", "PCDL"), q=q, w_bar=w_bar)
    assert np.array_equal(np.stack(pi["Ls"]), T[key + "_Ls"]) and np.array_equal(np.stack(pi["Rs"]), T[key + "_Rs"])
    assert np.array_equal(pi["U"], T[key + "_U"][0]) and np.array_equal(pi["c"], T[key + "_c"][0])
    if w is not None:
        assert np.array_equal(pi["C_bar"], T[key + "_Cbar"][0]) and np.array_equal(pi["w_prime"], T[key + "_wprime_alpha"][0])


@pytest.mark.parametrize("cname", CURVES)
def test_drop_in_accumulation(sp, golden, corc, cname):
    n = 16
    use_srs(corc, golden, cname, n)
    rng = np.random.default_rng(33)
    qs = []
    for _ in range(2):
        ins = scalar_fe(cname, rand_ints(rng, P.CURVES[cname].scalar, n + 1))
        C = pcdl.commit(ins[:n], n - 1, curve=cname)
        pi = pcdl.open(ins[:n], C, n - 1, ins[n], transcript=R.SpongeAdapter(cname, "PCDL"), curve=cname)
        qs.append(pcdl.Instance(C, n - 1, ins[n], pi["v"], dict(pi, Ls=np.stack(pi["Ls"]), Rs=np.stack(pi["Rs"]))))
    a = acc.prover(qs, sponge.new_transcript(cname), cname)
    e = acc.prover(qs, R.new_transcript(cname), cname)
    assert np.array_equal(a.C, e.C) and a.d == e.d and np.array_equal(a.z, e.z) and np.array_equal(a.v, e.v)
    for f in ("Ls", "Rs"):
        assert len(a.pi[f]) == 4 and all(np.array_equal(x, y) for x, y in zip(a.pi[f], e.pi[f]))
    assert np.array_equal(a.pi["U"], e.pi["U"]) and np.array_equal(a.pi["c"], e.pi["c"])
    acc.verifier(qs, a, sponge.new_transcript(cname), curve=cname)
    acc.decider(a, sponge.new_transcript(cname), curve=cname)


# ---------------------------------------------------------------------------------------------
# 7. the prover
# ---------------------------------------------------------------------------------------------
def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, np.asarray(b))
    return a == b


@pytest.mark.parametrize("cname", CURVES)
def test_prover_bit_identity(sp, golden, corc, cname):
    """device_plonk on and off over one synthetic witness and one acc_prev at n = 2^4: the same proof, and with all
    three device flags the factory is asked for no sponge at all."""
    from halo_amd.prover import DeviceBackend, naive_prover, synthetic_witness
    n = 16
    use_srs(corc, golden, cname, n)
    asked = []

    def nt(label):
        asked.append(label)
        return R.SpongeAdapter(cname, label)

    B0 = DeviceBackend(cname, True, True, device_plonk=False)
    B1 = DeviceBackend(cname, True, True, device_plonk=True)
    wit = synthetic_witness(B0, n, seed=3)
    p0 = B0.random_vec(n, np.random.default_rng(4))
    acc_prev = B0.acc_prove([B0.instance_open(p0, n - 1, 12345, nt)], n - 1, nt)
    assert asked == []  # device_transcripts, device_acc
    out0 = naive_prover(B0, wit, n, None, acc_prev=acc_prev, transcript=nt)
    assert asked == ["PLONK"]
    out1 = naive_prover(B1, wit, n, None, acc_prev=acc_prev, transcript=nt)
    assert asked == ["PLONK"]
    for f in ("C_ws", "C_z", "C_ts", "vs", "q_r", "q_r_omega", "acc"):
        assert same(out1[f], out0[f]), f
    with pytest.raises(ValueError, match="device_plonk"):
        naive_prover(B0, wit, n, None, acc_prev=acc_prev, transcript="device")


def test_prover_round_trip_with_no_host_sponge(sp, golden, corc):
    """n = 2^6 over a satisfiable circuit: the proof made with transcript="device" passes plonk.verify, its challenges
    are the restatement's, and a flipped evaluation is rejected with the identity's message."""
    from halo_amd.prover import DeviceBackend, naive_prover
    from test_gpu_plonk_verify import circuit_of, restated
    cname, n = "pallas", 64
    m = P.CURVES[cname].scalar
    S, Hh = golden[f"ref_sh_{cname}"]
    srs = corc.srs_generate(cname, n)
    group.PublicParams.upload(cname, srs, S, Hh, precompute_windows=True)
    B = DeviceBackend(cname, device_transcripts=True, device_acc=True, device_plonk=True)
    host = R.satisfiable_circuit(R.CpuBackend(cname, srs[:1], S, Hh), n, seed=5, cname=cname)
    wit = {k: [B.from_ints(p) for p in host[k]] for k in ("qs", "ws", "rs", "ids", "sigmas")}
    wit["w_evals"] = [B.ntt(p, n) for p in wit["ws"]]
    wit["public_inputs"], wit["mds"] = host["public_inputs"], host["mds"]
    p0 = B.from_ints(rand_ints(np.random.default_rng(6), m, n))
    acc_prev = B.acc_prove([B.instance_open(p0, n - 1, 12345, None)], n - 1, None)
    out = naive_prover(B, wit, n, None, acc_prev=acc_prev, transcript="device")
    C_qs = np.stack(B.commit_many(wit["qs"]))
    proof = plonk.PlonkProof.from_prover(out, cname)
    circuit = circuit_of(cname, n, C_qs)
    pub = np.stack([R.fe(x, m) for x in host["public_inputs"]])
    prev = pcdl.Instance(acc_prev["C"], n - 1, R.fe(acc_prev["z"], m), R.fe(acc_prev["v"], m),
                         {"Ls": np.stack(acc_prev["Ls"]), "Rs": np.stack(acc_prev["Rs"]), "U": acc_prev["U"],
                          "c": R.fe(acc_prev["c"], m), "C_bar": None, "w_prime": None})
    plonk.verify(proof, circuit, pub, prev, curve=cname)
    verdict, chal, _, _ = plonk.verify_succinct_batch(circuit, [pub], [prev], [proof], cname, readbacks=True)
    code, rb = restated(cname, n, C_qs, golden, R.rec_from_prover(B, out, acc_prev, host["public_inputs"]))
    assert code == 0 and verdict.tolist() == [0]
    assert np.array_equal(chal[0], rb["challenges"])
    flipped = proof._replace(vs=proof.vs._replace(z=R.plus_one(proof.vs.z, m)))
    with pytest.raises(pcdl.CheckFailed) as e:
        plonk.verify(flipped, circuit, pub, prev, curve=cname)
    assert e.value.msg == plonk.IDENTITY_MSG


# ---------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------
def test_errors_name_the_call(sp):
    import ctypes
    L = sp.load()
    hid = ctypes.c_uint64(0)
    assert L.halo_sponge_new(0, 4, 1, ctypes.byref(hid)) == EINVAL and "halo_sponge_new" in sp.last_error()
    assert L.halo_sponge_new(0, -1, 1, ctypes.byref(hid)) == EINVAL and "halo_sponge_new" in sp.last_error()
    assert L.halo_sponge_new(1, 2, 0, ctypes.byref(hid)) == EINVAL and "halo_sponge_new" in sp.last_error()
    with pytest.raises(ValueError, match="label"):
        sponge.Sponge("pallas", "plonk")
    with pytest.raises(sp.HaloError, match="halo_sponge_new"):
        sponge.SpongeBatch("pallas", "PLONK", 0)
    s = sponge.Sponge("pallas", "PLONK")
    freed = s._id
    s.close()
    x, pt, out = np.ones((1, 4), dtype=np.uint64), np.zeros((1, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    for bad in (freed, 1 << 40):  # a freed id, one that was never made
        calls = {"halo_sponge_free": lambda: L.halo_sponge_free(bad), "halo_sponge_reset": lambda: L.halo_sponge_reset(bad),
                 "halo_sponge_absorb_g": lambda: L.halo_sponge_absorb_g(bad, sp.ptr(pt), 1),
                 "halo_sponge_absorb_fr": lambda: L.halo_sponge_absorb_fr(bad, sp.ptr(x), 1),
                 "halo_sponge_absorb_fq": lambda: L.halo_sponge_absorb_fq(bad, sp.ptr(x), 1),
                 "halo_sponge_challenge": lambda: L.halo_sponge_challenge(bad, 1, sp.ptr(out)),
                 "halo_sponge_absorb_g_dev": lambda: L.halo_sponge_absorb_g_dev(bad, None, 1, None),
                 "halo_sponge_absorb_fr_dev": lambda: L.halo_sponge_absorb_fr_dev(bad, None, 1, None),
                 "halo_sponge_absorb_fq_dev": lambda: L.halo_sponge_absorb_fq_dev(bad, None, 1, None),
                 "halo_sponge_challenge_dev": lambda: L.halo_sponge_challenge_dev(bad, 1, None, None)}
        for name, call in calls.items():
            assert call() == EINVAL, name
            assert name + ":" in sp.last_error(), name
    assert not out.any()


def test_parameters_not_set():
    """A process that never installed the Poseidon parameters: halo_sponge_new is HALO_EINVAL before it touches a device."""
    code = ("import ctypes\nfrom halo_amd import _lib as H\nL = H.load()\nhid = ctypes.c_uint64(0)\n"
            "rc = L.halo_sponge_new(0, 2, 1, ctypes.byref(hid))\nprint(rc, H.last_error())\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, check=True)
    rc, msg = out.stdout.strip().split(" ", 1)
    assert int(rc) == EINVAL and "halo_sponge_new" in msg and "halo_poseidon_set_params" in msg


@pytest.mark.parametrize("cname", CURVES)
def test_host_form_rejects_what_is_not_below_the_modulus(sp, golden, cname):
    c = P.CURVES[cname]
    limbs = lambda v: np.array([P.int_to_limbs(v)], dtype=np.uint64)  # noqa: E731
    gen = golden[f"ref_srs_{cname}_b00_first64"][2]
    d, o = both(cname, "PLONK")
    d.absorb_g([gen]), o.absorb_g([gen])
    with pytest.raises(sp.HaloError, match="halo_sponge_absorb_fr: a scalar is not below the modulus") as e:
        d.absorb_fr(np.concatenate([scalar_fe(cname, [9]), limbs(c.scalar)]))
    assert e.value.code == EINVAL
    with pytest.raises(sp.HaloError, match="halo_sponge_absorb_fq"):
        d.absorb_fq(limbs(c.base))
    with pytest.raises(sp.HaloError, match="halo_sponge_absorb_g"):
        d.absorb_g(np.concatenate([gen[:4], limbs(c.base)[0]])[None])
    same_challenge(d, o, "the state never saw them")
