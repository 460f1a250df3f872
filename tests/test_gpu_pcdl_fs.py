"""GPU tests of pcdl::succinct_check from raw proofs (halo_amd/csrc/pcdl_fs.hip behind
halo_pcdl_succinct_check_fs_batch and its _dev form; halo_amd.pcdl.succinct_check_device / check_device): every
challenge the device derives -- alpha, xi_0 .. xi_lg_n -- bit for bit against the CPU restatement of the
reference's Poseidon PCDL transcript (oracle/poseidon.py), and the verdicts, for

  * every opening of tests/golden/transcript.npz: both curves (the two branches of absorb_fr and challenge),
    plain and hiding (both parities at the rate-2 boundary), 4 to 14 rounds, both lane layouts;
  * one round (n = 2) and no round (d = 0);
  * batches that cross a three-lane wave (21 sponges) and a one-lane wave (64), mixing hiding and plain
    instances and tampered ones: the transcript does not depend on whether the check passes;
  * the identity as a round point and as C', a point off the curve next to good instances;
  * the device-pointer form; the Python layer (two degree bounds in one list, the first failing instance)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import pasta as P
import pcdl_check
import poseidon
from halo_amd import acc, group, pcdl
from test_gpu_pcdl_check import SpongeAdapter, det_scalars, fe, load_case, plus_one, unwrapped, wrapped

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "transcript.npz"))
CASES = sorted({k[:-2] for k in G.files if (k.startswith("open_") or k.startswith("big_")) and k.endswith("_C")})
LANES = [1, 3]


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
def _transcript(cname, C, z, v, Ls, Rs, C_bar, w_prime, S):
    """(alpha, xis) of one instance as ark scalars, from its bytes: the walk of pcdl.rs:496-534 alone, so it
    is defined for proofs that fail the check too."""
    cv = P.CURVES[cname]
    m = cv.scalar
    pt = lambda b: unwrapped(cv, np.frombuffer(b, dtype=np.uint64))  # noqa: E731
    sc = lambda b: to_int(np.frombuffer(b, dtype=np.uint64), m)  # noqa: E731
    t = poseidon.Sponge(cname, poseidon.PCDL)
    Cp, alpha = pt(C), 0
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
    return fe(alpha, m) if C_bar is not None else np.zeros(4, dtype=np.uint64), np.stack([fe(x, m) for x in xis])


def oracle_transcript(cname, golden, C, z, v, pi):
    b = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()  # noqa: E731
    hid = pi.get("C_bar") is not None
    return _transcript(cname, b(C), b(z), b(v), b(pi["Ls"]), b(pi["Rs"]), b(pi["C_bar"]) if hid else None,
                       b(pi["w_prime"]) if hid else None, b(golden[f"ref_sh_{cname}"][0]))


def run_batch(cname, d, items):
    """items: [(C, z, v, pi)] of degree bound d -> (ok, xis, alphas) of one host-array call."""
    hid = [pi.get("C_bar") is not None for _, _, _, pi in items]
    zero_pt, zero_fe = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    return pcdl.succinct_check_fs_verdicts(
        np.stack([C for C, _, _, _ in items]), d, np.stack([z for _, z, _, _ in items]), np.stack([v for _, _, v, _ in items]),
        np.concatenate([pi["Ls"] for *_, pi in items]) if d else None,
        np.concatenate([pi["Rs"] for *_, pi in items]) if d else None, np.stack([pi["U"] for *_, pi in items]),
        np.stack([pi["c"] for *_, pi in items]), hiding=hid if any(hid) else None,
        C_bars=np.stack([pi["C_bar"] if h else zero_pt for (*_, pi), h in zip(items, hid)]),
        w_primes=np.stack([pi["w_prime"] if h else zero_fe for (*_, pi), h in zip(items, hid)]), curve=cname)


def fresh_opening(corc, golden, cname, n, hiding, seed):
    """An opening made on the device under the oracle sponge (as test_accumulation makes its instances) over
    the recipe SRS of length n, which stays uploaded: (C, z, v, pi)."""
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, corc.srs_generate(cname, n), S, Hh, precompute_windows=True)
    ins = det_scalars(seed, 2 * n + 4)
    p, z = ins[:n], ins[2 * n]
    w = q = w_bar = None
    if hiding:
        q, w, w_bar = ins[n: 2 * n - 1], ins[2 * n + 1], ins[2 * n + 2]
    C = pcdl.commit(p, n - 1, w=w, curve=cname)
    pi = pcdl.open(p, C, n - 1, z, w=w, transcript=SpongeAdapter(cname), q=q, w_bar=w_bar, curve=cname)
    pi = dict(pi, Ls=np.stack(pi["Ls"]), Rs=np.stack(pi["Rs"]))
    return C, z, pi["v"], pi


# ---------------------------------------------------------------------------------------------
# 1. the committed openings
# ---------------------------------------------------------------------------------------------
_ORACLE_XIS = {}


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("key", CASES)
def test_fixture_challenges_bit_exact(fs, golden, corc, key, lanes):
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    m = P.CURVES[cname].scalar
    hid = key.endswith("hiding")
    S, Hh = golden[f"ref_sh_{cname}"]
    if key + "_xis" in G.files:
        exp = G[key + "_xis"]
    else:  # the oracle's own succinct check under its transcript (it also asserts the algebra); once per key
        if key not in _ORACLE_XIS:
            _ORACLE_XIS[key] = np.stack([fe(x, m) for x in pcdl_check.succinct_check_transcript(
                cname, C, d, to_int(z, m), to_int(v, m), pi["Ls"], pi["Rs"], pi["U"], to_int(pi["c"], m), Hh, S=S,
                C_bar=pi["C_bar"], w_prime=to_int(pi["w_prime"], m) if hid else None)])
        exp = _ORACLE_XIS[key]
    with fs.tuning(poseidon_lanes=lanes):
        ok, xis, alphas = run_batch(cname, d, [(C, z, v, pi)])
        assert np.array_equal(xis[0], exp), key
        assert np.array_equal(alphas[0], G[key + "_wprime_alpha"][1] if hid else np.zeros(4, dtype=np.uint64)), key
        assert ok.tolist() == [1]
        pcdl.check_device(C, d, z, v, pi, curve=cname)


# ---------------------------------------------------------------------------------------------
# 2. one round and no round
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_one_round(fs, golden, corc, cname, lanes):
    C, z, v, pi = fresh_opening(corc, golden, cname, 2, False, 900)
    with fs.tuning(poseidon_lanes=lanes):
        ok, xis, _ = run_batch(cname, 1, [(C, z, v, pi)])
    assert xis.shape == (1, 2, 4) and np.array_equal(xis[0], oracle_transcript(cname, golden, C, z, v, pi)[1])
    assert ok.tolist() == [1]


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_no_round(fs, golden, corc, cname, lanes):
    """d = 0: Ls / Rs NULL, one challenge; the verdict is what halo_pcdl_succinct_check_batch gives for xi_0."""
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, corc.srs_generate(cname, 2), S, Hh, precompute_windows=True)
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    z, v, c = det_scalars(901, 3)
    empty = np.zeros((0, 8), dtype=np.uint64)
    pi = {"Ls": empty, "Rs": empty, "U": srs[2].copy(), "c": c, "C_bar": None, "w_prime": None}
    C = srs[1].copy()
    with fs.tuning(poseidon_lanes=lanes):
        ok, xis, _ = run_batch(cname, 0, [(C, z, v, pi)])
    exp = oracle_transcript(cname, golden, C, z, v, pi)[1]
    assert xis.shape == (1, 1, 4) and np.array_equal(xis[0], exp)
    ref = pcdl.succinct_check_verdicts(C[None], 0, z[None], v[None], exp, None, None, pi["U"][None], c[None], curve=cname)
    assert ok.tolist() == ref.tolist()


# ---------------------------------------------------------------------------------------------
# 3. batch boundaries
# ---------------------------------------------------------------------------------------------
def tampered(item, kind, m):
    C, z, v, pi = item
    if kind == "v":
        return C, z, plus_one(v, m), pi
    if kind == "c":
        return C, z, v, dict(pi, c=plus_one(pi["c"], m))
    if kind == "swap":
        Ls, Rs = pi["Ls"].copy(), pi["Rs"].copy()
        Ls[0], Rs[0] = pi["Rs"][0], pi["Ls"][0]
        return C, z, v, dict(pi, Ls=Ls, Rs=Rs)
    return C, z, v, dict(pi, U=pi["Ls"][1].copy())


@pytest.fixture(scope="module")
def n16(fs, golden, corc):
    """Per curve, the committed n = 16 opening and a fresh one of the other kind (Pallas: plain + hiding,
    Vesta: hiding + plain), so that a batch mixes both; the SRS of the last curve made stays uploaded, and
    the succinct check reads only (S, H) and D."""
    out = {}
    for cname, key in (("pallas", "open_pallas_n16_plain"), ("vesta", "open_vesta_n16_hiding")):
        other = fresh_opening(corc, golden, cname, 16, not key.endswith("hiding"), 910)
        _, C, d, z, v, pi = load_case(golden, corc, key)
        out[cname] = [(C, z, v, pi), other]
    return out


def mixed_batch(cname, pair, k):
    """k items alternating the two openings, tampered at 0, 20, 21, 22 and k - 1: (items, expected verdicts)."""
    m = P.CURVES[cname].scalar
    items = [pair[i % 2] for i in range(k)]
    exp = [1] * k
    for i, kind in zip((0, 20, 21, 22, k - 1), ("v", "c", "swap", "U", "v")):
        items[i] = tampered(items[i], kind, m)
        exp[i] = 0
    return items, exp


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("k", [23, 67])
@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_batch_boundaries(fs, golden, n16, cname, k, lanes):
    items, exp = mixed_batch(cname, n16[cname], k)
    with fs.tuning(poseidon_lanes=lanes):
        ok, xis, alphas = run_batch(cname, 15, items)
    assert ok.tolist() == exp
    for i, (C, z, v, pi) in enumerate(items):
        a, x = oracle_transcript(cname, golden, C, z, v, pi)
        assert np.array_equal(xis[i], x) and np.array_equal(alphas[i], a), i


# ---------------------------------------------------------------------------------------------
# 4. the identity and invalid points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_identity_round_point(fs, golden, n16, lanes):
    """L_1 = (0, 0): the transcript absorbs two zeros; the check fails."""
    C, z, v, pi = n16["pallas"][0]
    Ls = pi["Ls"].copy()
    Ls[1] = 0
    pi = dict(pi, Ls=Ls)
    with fs.tuning(poseidon_lanes=lanes):
        ok, xis, _ = run_batch("pallas", 15, [(C, z, v, pi)])
    assert np.array_equal(xis[0], oracle_transcript("pallas", golden, C, z, v, pi)[1]) and ok.tolist() == [0]


@pytest.mark.parametrize("lanes", LANES)
def test_identity_c_prime(fs, golden, n16, lanes):
    """C_bar = (0, 0) and C = w' S: C' = C + alpha C_bar - w' S is the identity, absorbed as (0, 0)."""
    cname = "vesta"
    cv = P.CURVES[cname]
    C, z, v, pi = n16[cname][0]
    S = golden[f"ref_sh_{cname}"][0]
    C = wrapped(cv, P.mul_fast(cv, to_int(pi["w_prime"], cv.scalar), unwrapped(cv, S)))
    pi = dict(pi, C_bar=np.zeros(8, dtype=np.uint64))
    with fs.tuning(poseidon_lanes=lanes):
        _, xis, alphas = run_batch(cname, 15, [(C, z, v, pi)])
    a, x = oracle_transcript(cname, golden, C, z, v, pi)
    assert np.array_equal(xis[0], x) and np.array_equal(alphas[0], a)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("cname,where", [("pallas", "L0"), ("vesta", "C_bar"), ("pallas", "U")])
def test_point_off_the_curve(fs, golden, n16, cname, where, lanes):
    """The middle instance has a point that is neither (0, 0) nor on the curve: verdict 0 for it alone."""
    good = n16[cname][0]
    C, z, v, pi = good
    if where == "L0":
        Ls = pi["Ls"].copy()
        Ls[0, 0] ^= np.uint64(1)
        bad = (C, z, v, dict(pi, Ls=Ls))
    else:
        off = pi[where].copy()
        off[0] ^= np.uint64(1)
        bad = (C, z, v, dict(pi, **{where: off}))
    with fs.tuning(poseidon_lanes=lanes):
        ok, xis, _ = run_batch(cname, 15, [good, bad, good])
    assert ok.tolist() == [1, 0, 1]
    x = oracle_transcript(cname, golden, *good)[1]
    assert np.array_equal(xis[0], x) and np.array_equal(xis[2], x)


# ---------------------------------------------------------------------------------------------
# 5. the device-pointer form
# ---------------------------------------------------------------------------------------------
def run_batch_dev(fs, cname, d, items):
    """run_batch through halo_pcdl_succinct_check_fs_batch_dev over torch buffers on the current stream."""
    import torch
    k, lg = len(items), (d + 1).bit_length() - 1

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
    d_xis = torch.zeros(k * (lg + 1) * 4, dtype=torch.int64, device="cuda")
    d_alpha = torch.full((k * 4,), 7, dtype=torch.int64, device="cuda")
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fs.check(fs.load().halo_pcdl_succinct_check_fs_batch_dev(
        fs.CURVES[cname], d, k, *[b.data_ptr() for b in bufs], d_xis.data_ptr(), d_alpha.data_ptr(), d_ok.data_ptr(),
        ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    return (d_ok.cpu().numpy(), d_xis.cpu().numpy().view(np.uint64).reshape(k, lg + 1, 4),
            d_alpha.cpu().numpy().view(np.uint64).reshape(k, 4))


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_dev_form_equals_the_host_form(fs, golden, n16, cname):
    items, exp = mixed_batch(cname, n16[cname], 67)
    ok, xis, alphas = run_batch(cname, 15, items)
    d_ok, d_xis, d_alpha = run_batch_dev(fs, cname, 15, items)
    assert d_ok.tolist() == ok.tolist() == exp
    assert np.array_equal(d_xis, xis) and np.array_equal(d_alpha, alphas)


@pytest.mark.parametrize("cname,which", [("pallas", "z"), ("pallas", "c"), ("vesta", "v"), ("vesta", "w_prime")])
def test_dev_form_scalar_not_below_the_modulus(fs, golden, n16, cname, which):
    """The host form rejects such a call (tests/test_pcdl_fs_abi.py); the device form gives that instance
    verdict 0 and leaves its neighbours alone."""
    good = n16[cname][0]
    C, z, v, pi = good
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    bad = {"z": (C, big, v, pi), "v": (C, z, big, pi)}.get(which) or (C, z, v, dict(pi, **{which: big}))
    ok, xis, _ = run_batch_dev(fs, cname, 15, [good, bad, good])
    assert ok.tolist() == [1, 0, 1]
    x = oracle_transcript(cname, golden, *good)[1]
    assert np.array_equal(xis[0], x) and np.array_equal(xis[2], x)


# ---------------------------------------------------------------------------------------------
# 6. the Python layer
# ---------------------------------------------------------------------------------------------
def test_succinct_check_device_matches_succinct_check_many(fs, golden, corc):
    """A list with two degree bounds, plain and hiding; then the first failing instance is named."""
    insts = []
    for key in ("open_pallas_n16_plain", "open_pallas_n64_hiding"):  # the longer SRS is uploaded last
        cname, C, d, z, v, pi = load_case(golden, corc, key)
        insts.append(pcdl.Instance(C, d, z, v, pi))
    insts = [insts[0], insts[1], insts[0], insts[1]]
    exp = pcdl.succinct_check_many(insts, [SpongeAdapter("pallas") for _ in insts], curve="pallas")
    got = pcdl.succinct_check_device(insts, curve="pallas")
    assert len(got) == len(exp) == 4
    for (h, U), (he, Ue) in zip(got, exp):
        assert np.array_equal(h.xis, he.xis) and np.array_equal(U, Ue)
    m = P.CURVES["pallas"].scalar
    bad = list(insts)
    bad[1] = bad[1]._replace(v=plus_one(bad[1].v, m))
    bad[2] = bad[2]._replace(v=plus_one(bad[2].v, m))
    with pytest.raises(pcdl.CheckFailed, match="^C_\\(log_n\\) ≠ CM.Commit_Σ\\(c \\|\\| v'\\) \\(instance 1\\)$") as e:
        pcdl.succinct_check_device(bad, curve="pallas")
    assert e.value.index == 1 and e.value.msg == pcdl.SUCCINCT_MSG
    with pytest.raises(pcdl.CheckFailed, match="^C_\\(log_n\\) ≠ CM.Commit_Σ\\(c \\|\\| v'\\)$"):
        pcdl.check_device(bad[1].C, bad[1].d, bad[1].z, bad[1].v, bad[1].pi, curve="pallas")
    with pytest.raises(pcdl.CheckFailed, match="d was larger than D!"):
        pcdl.succinct_check_device([insts[0]._replace(d=127)], curve="pallas")
    with pytest.raises(AssertionError, match=r"n \(11\) is not a power of two"):
        pcdl.succinct_check_device([insts[0]._replace(d=10)], curve="pallas")


def test_accumulation_with_device_transcripts(fs, golden, corc):
    """acc.common_subroutine / verifier with the PCDL sponges on the device give what the caller's sponges give."""
    cname = "pallas"
    qs = []
    for i in range(3):
        C, z, v, pi = fresh_opening(corc, golden, cname, 16, False, 920 + i)
        qs.append(pcdl.Instance(C, 15, z, v, pi))

    def new_transcript(label):
        return SpongeAdapter(cname, label)

    exp = acc.common_subroutine(qs, new_transcript, curve=cname)
    got = acc.common_subroutine(qs, new_transcript, curve=cname, device_transcripts=True)
    assert np.array_equal(got[0], exp[0]) and got[1] == exp[1] and np.array_equal(got[2], exp[2])
    assert all(np.array_equal(a.xis, b.xis) for a, b in zip(got[3], exp[3])) and np.array_equal(got[4], exp[4])
    a = acc.prover(qs, new_transcript, curve=cname)
    acc.verifier(qs, a, new_transcript, curve=cname, device_transcripts=True)
    bad = list(qs)
    bad[1] = qs[1]._replace(v=plus_one(qs[1].v, P.CURVES[cname].scalar))
    with pytest.raises(pcdl.CheckFailed, match="instance 1"):
        acc.common_subroutine(bad, new_transcript, curve=cname, device_transcripts=True)
