"""GPU tests of pcdl::open in one call with its transcript on the device (halo_amd/csrc/pcdl_open_fs.hip behind
halo_pcdl_open_fs and halo_pcdl_open_fs_dev_multi; halo_amd.pcdl.open_device / open_without_eval_device /
open_device_many): the proofs equal, bit for bit, the committed fixture of tests/golden/make_transcript.py, which
the reference made under its own Poseidon PCDL sponge -- so every challenge the device derived, its inverse and
every fold that read it from device memory is covered.

  1. every open_* case (n = 16..1024: the fused tail round up to 256, the three-launch round above), both lane
     layouts of the sponge;
  2. the big_* cases (4096, 2^14) on every path the tuning keys select;
  3. n = 2 and n = 4 against pcdl.open under the oracle sponge;
  4. k openings side by side (open_device_many) against the single call;
  5. every proof of 1-2 passes pcdl.check_device;
  6. the session pool: device and host transcripts alternate, a failed assertion leaves the pool usable;
  7. the prover and 8. the accumulation prover with device transcripts against the caller's sponges."""
import functools
import os

import numpy as np
import pytest

from halo_amd import acc, group, pcdl
from test_gpu_pcdl_check import SpongeAdapter, det_scalars
from test_gpu_pcdl_fs import fs  # noqa: F401  (the Poseidon constants, installed once per module)

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "transcript.npz"))
CASES = sorted({k[:-2] for k in G.files if k.startswith("open_") and k.endswith("_p")})
BIG = sorted({k[:-5] for k in G.files if k.startswith("big_") and k.endswith("_seed")})
LANES = [1, 3]
_SRS = {}


def upload(corc, golden, cname, n):
    """The recipe SRS of length n with the reference's (S, H); generated once per (curve, n)."""
    if (cname, n) not in _SRS:
        _SRS[(cname, n)] = corc.srs_generate(cname, n)
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, _SRS[(cname, n)], S, Hh, precompute_windows=True)


def parse(key):
    return key.split("_")[1], int(key.split("_")[2][1:]), key.endswith("hiding")


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(p, z, v, w, q, w_bar) of a fixture case; the big cases' inputs are regenerated from the stored seed."""
    cname, n, hiding = parse(key)
    z, v = G[key + "_zv"]
    w = q = w_bar = None
    if key.startswith("big_"):
        ins = det_scalars(int(G[key + "_seed"][0]), 2 * n + 4)
        p = ins[: n - 1]
        assert np.array_equal(z, ins[2 * n])
        if hiding:
            q, w, w_bar = ins[n: 2 * n - 1], ins[2 * n + 1], ins[2 * n + 2]
    else:
        p = G[key + "_p"]
        if hiding:
            (w, w_bar), q = G[key + "_w"], G[key + "_q"]
    return p, z, v, w, q, w_bar


def assert_fixture(key, pi):
    hiding = key.endswith("hiding")
    assert np.array_equal(np.stack(pi["Ls"]), G[key + "_Ls"]), key
    assert np.array_equal(np.stack(pi["Rs"]), G[key + "_Rs"]), key
    assert np.array_equal(pi["U"], G[key + "_U"][0]) and np.array_equal(pi["c"], G[key + "_c"][0]), key
    assert np.array_equal(pi["v"], G[key + "_zv"][1]), key
    if hiding:
        assert np.array_equal(pi["C_bar"], G[key + "_Cbar"][0]), key
        assert np.array_equal(pi["w_prime"], G[key + "_wprime_alpha"][0]), key
    else:
        assert pi["C_bar"] is None and pi["w_prime"] is None


def open_case(key, with_v):
    """The case's opening on the device; with_v: open_without_eval_device with the fixture's v, else open_device."""
    cname, n, _ = parse(key)
    p, z, v, w, q, w_bar = inputs(key)
    C = G[key + "_C"][0]
    if with_v:
        return pcdl.open_without_eval_device(p, C, n - 1, z, v, w=w, q=q, w_bar=w_bar, curve=cname)
    return pcdl.open_device(p, C, n - 1, z, w=w, q=q, w_bar=w_bar, curve=cname)


def check_round_trip(key, pi):
    cname, n, _ = parse(key)
    pcdl.check_device(G[key + "_C"][0], n - 1, G[key + "_zv"][0], pi["v"], dict(pi, Ls=np.stack(pi["Ls"]), Rs=np.stack(pi["Rs"])),
                      curve=cname)


# ---------------------------------------------------------------------------------------------
# 1. the committed openings (and 5. their round trip)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("key", CASES)
def test_fixture_parity(fs, golden, corc, key, lanes):
    cname, n, hiding = parse(key)
    upload(corc, golden, cname, n)
    with fs.tuning(poseidon_lanes=lanes):
        pi = open_case(key, with_v=not hiding)  # plain: open_without_eval_device; hiding: open_device
        assert_fixture(key, pi)
        check_round_trip(key, pi)


def test_both_entry_points_on_one_case(fs, golden, corc):
    """open_device on a plain case and open_without_eval_device on a hiding one (the other pairing of item 1)."""
    for key, with_v in (("open_vesta_n64_plain", False), ("open_pallas_n64_hiding", True)):
        cname, n, _ = parse(key)
        upload(corc, golden, cname, n)
        assert_fixture(key, open_case(key, with_v))


# ---------------------------------------------------------------------------------------------
# 2. the larger paths
# ---------------------------------------------------------------------------------------------
BIG_PATHS = [(k, {}) for k in BIG] + [(k, {"ipa_srs_tail_n": 0}) for k in BIG if parse(k)[1] == 4096] + [
    (k, {t: 0}) for k in BIG for t in ("ipa_weighted", "ipa_tail", "ipa_mat_n", "ipa_pair_max")]


@pytest.mark.parametrize("key,tune", BIG_PATHS, ids=[f"{k}-{next(iter(t), 'default')}" for k, t in BIG_PATHS])
def test_big_paths(fs, golden, corc, key, tune):
    """default: 4096 starts in the tail rounds over the SRS table, 2^14 runs weighted -> materialised -> tail;
    ipa_srs_tail_n=0 pins 4096 to that switch too; ipa_weighted=0 folds G every round (k_ipa_fold reads the
    challenge the transcript kernel left), ipa_tail=0 / ipa_mat_n=0 keep the other rounds to the end,
    ipa_pair_max=0 runs the weighted rounds as two MSMs on two streams."""
    cname, n, _ = parse(key)
    upload(corc, golden, cname, n)
    with fs.tuning(**tune):
        pi = open_case(key, with_v=True)
    assert_fixture(key, pi)
    if not tune:
        check_round_trip(key, pi)


# ---------------------------------------------------------------------------------------------
# 3. the smallest shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_smallest_shapes(fs, golden, corc, cname, n, hiding):
    """One round and two: no fixture exists, so the host-driven opening under the oracle sponge is the reference."""
    upload(corc, golden, cname, n)
    ins = det_scalars(1000 + n, 2 * n + 4)
    p, z = ins[:n], ins[2 * n]
    w = q = w_bar = None
    if hiding:
        q, w, w_bar = ins[n: 2 * n - 1], ins[2 * n + 1], ins[2 * n + 2]
    C = pcdl.commit(p, n - 1, w=w, curve=cname)
    exp = pcdl.open(p, C, n - 1, z, w=w, transcript=SpongeAdapter(cname), q=q, w_bar=w_bar, curve=cname)
    for lanes in LANES:
        with fs.tuning(poseidon_lanes=lanes):
            got = pcdl.open_device(p, C, n - 1, z, w=w, q=q, w_bar=w_bar, curve=cname)
        assert len(got["Ls"]) == n.bit_length() - 1
        for f in ("Ls", "Rs"):
            assert np.array_equal(np.stack(got[f]), np.stack(exp[f])), f
        for f in ("U", "c", "v") + (("C_bar", "w_prime") if hiding else ()):
            assert np.array_equal(got[f], exp[f]), f


# ---------------------------------------------------------------------------------------------
# 4. k openings side by side
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 4096])
def test_lockstep(fs, golden, corc, n):
    """open_device_many with k = 1, 2, 3, 5: k different polynomials at k different points, each opening equal to
    the single call's (a session that read a neighbour's challenge or sponge would differ)."""
    import torch
    cname = "pallas"
    upload(corc, golden, cname, n)
    ps = [det_scalars(1100 + i, n - (i % 2)) for i in range(5)]  # (two lengths: the zero padding differs)
    zs = det_scalars(1200, 5)
    Cs = np.stack([pcdl.commit(p, n - 1, curve=cname) for p in ps])
    single = [pcdl.open_device(ps[i], Cs[i], n - 1, zs[i], curve=cname) for i in range(5)]
    dev = [torch.from_numpy(p.view(np.int64).reshape(-1)).cuda() for p in ps]
    for k in (1, 2, 3, 5):
        got = pcdl.open_device_many(dev[:k], Cs[:k], n - 1, zs[:k], curve=cname)
        assert len(got) == k
        for i in range(k):
            for f in ("Ls", "Rs"):
                assert np.array_equal(np.stack(got[i][f]), np.stack(single[i][f])), (k, i, f)
            for f in ("U", "c", "v"):
                assert np.array_equal(got[i][f], single[i][f]), (k, i, f)
    pcdl.check_device(Cs[4], n - 1, zs[4], single[4]["v"],
                      dict(single[4], Ls=np.stack(single[4]["Ls"]), Rs=np.stack(single[4]["Rs"])), curve=cname)
    assert pcdl.open_device_many([], Cs[:0], n - 1, zs[:0], curve=cname) == []


# ---------------------------------------------------------------------------------------------
# 6. the session pool
# ---------------------------------------------------------------------------------------------
def test_pool_hygiene(fs, golden, corc):
    """On one device, in order: a device-transcript opening, a host-sponge opening, a hiding device opening, a plain
    device opening -- each its fixture (no stale sponge state, status word, pending fold or ping-pong swap); then
    an opening that fails its assertion, and the pool still serves the next one."""
    plain, hid = "open_pallas_n256_plain", "open_pallas_n64_hiding"

    def run(key, with_v):
        upload(corc, golden, "pallas", parse(key)[1])
        assert_fixture(key, open_case(key, with_v))

    run(plain, True)
    p, z, v, *_ = inputs(plain)
    pi = pcdl.open_without_eval(p, G[plain + "_C"][0], 255, z, v, transcript=SpongeAdapter("pallas"))
    assert_fixture(plain, pi)
    run(hid, False)
    run(plain, True)
    with pytest.raises(AssertionError, match=r"p.degree\(\) <= d"):
        pcdl.open_device(np.ones((9, 4), dtype=np.uint64), G[plain + "_C"][0], 7, z)
    with pytest.raises(AssertionError, match=r"d <= pp.D"):
        pcdl.open_device(p[:4], G[plain + "_C"][0], 1023, z)
    with pytest.raises(AssertionError, match=r"n \(11\) is not a power of two"):
        pcdl.open_device(p[:4], G[plain + "_C"][0], 10, z)
    run(hid, True)
    run(plain, False)


# ---------------------------------------------------------------------------------------------
# 7. the prover, 8. the accumulation prover
# ---------------------------------------------------------------------------------------------
def same(a, b):
    """Equality of the prover's nested results (dicts, lists, arrays, integers)."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, np.asarray(b))
    return a == b


def test_prover_with_device_transcripts(fs, golden, corc):
    """naive_prover under the reference's transcripts at n = 2^6 on DeviceBackend(device_transcripts=True) -- its two
    Instance::open as one k = 2 call over device-resident polynomials, acc::prover with its sponges on the device --
    returns what the default backend returns, and halo_amd.plonk verifies the proof."""
    import pasta as P
    import plonk_ref as R
    from halo_amd import plonk
    from halo_amd.prover import DeviceBackend, naive_prover
    from test_gpu_plonk_verify import circuit_of
    cname, n = "pallas", 64
    m = P.CURVES[cname].scalar
    upload(corc, golden, cname, n)
    S, Hh = golden[f"ref_sh_{cname}"]
    host = R.satisfiable_circuit(R.CpuBackend(cname, _SRS[(cname, n)][:1], S, Hh), n, seed=5, cname=cname)
    rng = np.random.default_rng(6)
    p0_ints = [int.from_bytes(rng.bytes(32), "little") % m for _ in range(n)]
    runs = []
    for dev in (False, True):
        B = DeviceBackend(cname, device_transcripts=dev)
        wit = {k: [B.from_ints(p) for p in host[k]] for k in ("qs", "ws", "rs", "ids", "sigmas")}
        wit["w_evals"] = [B.ntt(p, n) for p in wit["ws"]]
        wit["public_inputs"], wit["mds"] = host["public_inputs"], host["mds"]
        nt = R.new_transcript(cname)
        acc_prev = B.acc_prove([B.instance_open(B.from_ints(p0_ints), n - 1, 12345, nt)], n - 1, nt)
        out = naive_prover(B, wit, n, None, acc_prev=acc_prev, transcript=nt)
        runs.append((B, wit, acc_prev, out))
    (_, _, prev_host, out_host), (B, wit, acc_prev, out) = runs
    assert same(acc_prev, prev_host)
    for f in ("C_ws", "C_z", "C_ts", "vs", "q_r", "q_r_omega", "acc"):
        assert same(out[f], out_host[f]), f
    proof = plonk.PlonkProof.from_prover(out, cname)
    pub = np.stack([R.fe(x, m) for x in host["public_inputs"]])
    prev = pcdl.Instance(acc_prev["C"], n - 1, R.fe(acc_prev["z"], m), R.fe(acc_prev["v"], m),
                         {"Ls": np.stack(acc_prev["Ls"]), "Rs": np.stack(acc_prev["Rs"]), "U": acc_prev["U"],
                          "c": R.fe(acc_prev["c"], m), "C_bar": None, "w_prime": None})
    plonk.verify(proof, circuit_of(cname, n, np.stack(B.commit_many(wit["qs"]))), pub, prev, curve=cname)


def test_accumulation_prover_with_device_transcripts(fs, golden, corc):
    """acc.prover with the PCDL sponges on the device equals acc.prover under the caller's, on three n = 16
    instances; acc.verifier and acc.decider accept the accumulator."""
    from test_gpu_pcdl_fs import fresh_opening
    cname = "pallas"
    qs = []
    for i in range(3):
        C, z, v, pi = fresh_opening(corc, golden, cname, 16, False, 1300 + i)
        qs.append(pcdl.Instance(C, 15, z, v, pi))

    def new_transcript(label):
        return SpongeAdapter(cname, label)

    exp = acc.prover(qs, new_transcript, curve=cname)
    got = acc.prover(qs, new_transcript, curve=cname, device_transcripts=True)
    assert np.array_equal(got.C, exp.C) and got.d == exp.d and np.array_equal(got.z, exp.z) and np.array_equal(got.v, exp.v)
    for f in ("Ls", "Rs"):
        assert np.array_equal(np.stack(got.pi[f]), np.stack(exp.pi[f])), f
    assert np.array_equal(got.pi["U"], exp.pi["U"]) and np.array_equal(got.pi["c"], exp.pi["c"])
    got = got._replace(pi=dict(got.pi, Ls=np.stack(got.pi["Ls"]), Rs=np.stack(got.pi["Rs"])))
    acc.verifier(qs, got, new_transcript, curve=cname)
    acc.verifier(qs, got, new_transcript, curve=cname, device_transcripts=True)
    acc.decider(got, new_transcript, curve=cname)
