"""GPU tests of the PCDL verifier on the device (halo_amd/csrc/lincomb.hip behind halo_point_lincomb_batch,
halo_point_lincomb_batch_dev and halo_pcdl_succinct_check_batch; halo_amd.pcdl.succinct_check / check and
halo_amd.acc):

  * the batched linear combinations against the big-integer oracle (pasta.mul_fast / pasta.add) on both
    curves, over shapes that cross a quad, a wave of 16 quads and a block, with the scalars that exercise
    the GLV signs and an empty half-scalar, identity points and addends, a sum that needs a doubling, one
    that cancels, and a point off the curve;
  * acceptance of every opening of tests/golden/transcript.npz under the oracle's Poseidon sponge, with the
    challenges the fixture recorded (tests/test_oracle.py shows that the oracle's own succinct check, and so
    the reference, accepts these proofs);
  * rejection of tampered proofs with the reference's messages, per-item verdicts of a batch;
  * acc.prover / verifier / decider over three fresh instances against values recomputed with the oracle's
    ASDL sponge.
"""
import ctypes
import os

import numpy as np
import pytest

import pasta as P
import pcdl_check
import poseidon
from halo_amd import acc, group, pcdl

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "transcript.npz"))
CASES = sorted({k[:-2] for k in G.files if k.startswith("open_") and k.endswith("_p")})
LAMBDA = {"pallas": 0x397E65A7D7C1AD71AEE24B27E308F0A61259527EC1D4752E619D1840AF55F1B1,
          "vesta": 0x12CCCA834ACDBA712CAAD5DC57AAB1B01D1F8BD237AD31491DAD5EBDFDFE4AB9}  # gen_consts.py GLV
LABELS = {"PCDL": poseidon.PCDL, "ASDL": poseidon.ASDL}


class SpongeAdapter:
    """The oracle sponge behind the reference's Sponge interface, over WrappedPoints / ark scalars
    (tests/test_gpu_transcript.py), recording the challenges it hands out."""

    def __init__(self, cname, label="PCDL"):
        self.c = P.CURVES[cname]
        self.s = poseidon.Sponge(cname, LABELS[label])
        self.challenges = []

    def absorb_g(self, pts):
        self.s.absorb_g([P.wrapped_to_point(self.c, [int(x) for x in q]) for q in pts])

    def absorb_fr(self, xs):
        self.s.absorb_fr([P.from_mont(P.limbs_to_int(x), self.c.scalar) for x in xs])

    def challenge(self):
        x = np.array(P.int_to_limbs(P.to_mont(self.s.challenge(), self.c.scalar)), dtype=np.uint64)
        self.challenges.append(x)
        return x


def fe(x: int, m: int) -> np.ndarray:
    return np.array(P.int_to_limbs(P.to_mont(x % m, m)), dtype=np.uint64)


def plus_one(x, m: int) -> np.ndarray:
    return fe(P.from_mont(P.limbs_to_int(x), m) + 1, m)


def wrapped(c, pt) -> np.ndarray:
    return np.array(P.point_to_wrapped(c, pt), dtype=np.uint64)


def unwrapped(c, w):
    return P.wrapped_to_point(c, [int(x) for x in w])


def det_scalars(seed: int, k: int) -> np.ndarray:
    """tests/golden/make_transcript.py det_scalars: k Montgomery-form scalars < 2^254 from seed."""
    a = np.random.default_rng(seed).integers(0, 2**64 - 1, size=(k, 4), dtype=np.uint64, endpoint=True)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return np.ascontiguousarray(a)


# ---------------------------------------------------------------------------------------------
# linear combinations
# ---------------------------------------------------------------------------------------------
def lincomb_dev(hal, cname, add, pts, sc):
    """halo_point_lincomb_batch_dev over torch buffers; (k affine sums, k identity bytes)."""
    import torch
    cid = hal.CURVES[cname]
    k, t = pts.shape[0], pts.shape[1]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()

    d_pts, d_sc = dev(pts), dev(sc)
    d_add = dev(add) if add is not None else None
    d_out = torch.zeros(k * 16, dtype=torch.int64, device="cuda")
    d_id = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    hal.check(hal.load().halo_point_lincomb_batch_dev(cid, d_add.data_ptr() if add is not None else None, d_pts.data_ptr(),
                                                      d_sc.data_ptr(), k, t, d_out.data_ptr(), d_id.data_ptr(),
                                                      ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    xyzz = np.ascontiguousarray(d_out.cpu().numpy().view(np.uint64))
    out = np.zeros((k, 8), dtype=np.uint64)
    hal.check(hal.load().halo_xyzz_to_wrapped(cid, hal.ptr(xyzz), k, hal.ptr(out)))
    return out, d_id.cpu().numpy()


def oracle_lincomb(c, add, pts, ks):
    """out_i = A_i + sum_j ks[i][j] pts[i][j] over affine points (None: the identity)."""
    out = []
    for i in range(len(pts)):
        a = add[i] if add is not None else P.INF
        for pt, s in zip(pts[i], ks[i]):
            a = P.add(c, a, P.mul_fast(c, s, pt))
        out.append(a)
    return out


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
@pytest.mark.parametrize("k,t", [(1, 1), (1, 10), (17, 1), (3, 11), (5, 7)])
def test_lincomb_matches_the_oracle(hal, golden, cname, k, t):
    """(k, t) cross a quad (1 term), a wave of 16 quads (17 terms) and a block (33, 35 terms), and each
    leaves a ragged last block.  The first scalars are 0, 1, r - 1, 2^128 and lambda (in an order that
    depends on the shape, so the one-term shape gets r - 1): both GLV signs, a half-scalar of 2^128's
    size and an empty one.  Term 6 is the identity point, item 0's addend the identity; the 17 x 1 shape
    has no addends at all."""
    c = P.CURVES[cname]
    r = c.scalar
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    rng = np.random.default_rng(1000 * k + t)
    n = k * t
    ks = [int.from_bytes(rng.bytes(32), "little") % r for _ in range(n)]
    special = [0, 1, r - 1, 1 << 128, LAMBDA[cname]]
    for i in range(min(5, n)):
        ks[i] = special[(i + k + t) % 5]
    pts_w = np.stack([srs[(7 * i + t) % 64] for i in range(n)])
    if n > 6:
        pts_w[6] = 0
    add_w = None
    if (k, t) != (17, 1):
        add_w = np.stack([srs[(63 - i) % 64] for i in range(k)])
        add_w[0] = 0
    pts_w = np.ascontiguousarray(pts_w.reshape(k, t, 8))
    sc = np.stack([fe(x, r) for x in ks]).reshape(k, t, 4)
    exp = oracle_lincomb(c, None if add_w is None else [unwrapped(c, a) for a in add_w],
                         [[unwrapped(c, q) for q in row] for row in pts_w], np.array(ks, dtype=object).reshape(k, t))
    exp_w = np.stack([wrapped(c, e) for e in exp])
    got = pcdl.point_lincomb(pts_w, sc, add=add_w, curve=cname)
    assert np.array_equal(got, exp_w)
    got_dev, is_id = lincomb_dev(hal, cname, add_w, pts_w, sc)
    assert np.array_equal(got_dev, got)
    assert np.array_equal(is_id, np.array([e is P.INF for e in exp], dtype=np.uint8))


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_lincomb_doubling_cancellation_and_invalid_point(hal, golden, cname):
    """Rows of two terms, summed by two lanes of the sum kernel: [s P, s P] needs a doubling, [s P, (r - s) P]
    cancels to the identity (byte 1), a row with a point off the curve is invalid ((0, 0), byte 0) and the
    rows around it are untouched."""
    c = P.CURVES[cname]
    r = c.scalar
    srs = golden[f"ref_srs_{cname}_b00_first64"]
    s = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % r
    Pw, Qw = srs[3], srs[4]
    off = Pw.copy()
    off[0] ^= np.uint64(1)
    assert not P.on_curve(c, (P.from_mont(P.limbs_to_int(off[:4]), c.base), P.from_mont(P.limbs_to_int(off[4:]), c.base)))
    pts_w = np.ascontiguousarray(np.stack([[Pw, Pw], [Pw, Pw], [Qw, off], [Qw, Pw], [Pw, Pw]]))
    ks = [[s, s], [s, r - s], [s, 5], [s, 5], [r - s, r - s]]
    sc = np.stack([fe(x, r) for row in ks for x in row]).reshape(5, 2, 4)
    Pp, Qp = unwrapped(c, Pw), unwrapped(c, Qw)
    sP = P.mul_fast(c, s, Pp)
    exp = [P.add(c, sP, sP), P.INF, P.INF, P.add(c, P.mul_fast(c, s, Qp), P.mul_fast(c, 5, Pp)),
           P.neg(c, P.add(c, sP, sP))]
    exp_w = np.stack([wrapped(c, e) for e in exp])
    got = pcdl.point_lincomb(pts_w, sc, curve=cname)
    assert np.array_equal(got, exp_w)
    got_dev, is_id = lincomb_dev(hal, cname, None, pts_w, sc)
    assert np.array_equal(got_dev, exp_w)
    assert is_id.tolist() == [0, 1, 0, 0, 0]
    # the same cancellation against the addend: A = -(2 s P), and an addend off the curve
    add_w = np.stack([wrapped(c, P.neg(c, exp[0])), off, Qw, Qw, Qw])
    got_dev, is_id = lincomb_dev(hal, cname, add_w, pts_w, sc)
    assert not got_dev[0].any() and not got_dev[1].any() and not got_dev[2].any()
    assert is_id.tolist() == [1, 0, 0, 0, 0]
    assert np.array_equal(got_dev[3], wrapped(c, P.add(c, exp[3], Qp)))
    assert np.array_equal(pcdl.point_lincomb(pts_w, sc, add=add_w, curve=cname), got_dev)


def test_lincomb_dev_without_terms_returns_the_addends(hal, golden):
    srs = golden["ref_srs_pallas_b00_first64"]
    add_w = np.ascontiguousarray(srs[:3].copy())
    add_w[1] = 0
    empty = np.zeros((3, 0, 8), dtype=np.uint64)
    got, is_id = lincomb_dev(hal, "pallas", add_w, empty, np.zeros((3, 0, 4), dtype=np.uint64))
    assert np.array_equal(got, add_w) and is_id.tolist() == [0, 1, 0]
    got, is_id = lincomb_dev(hal, "pallas", None, empty, np.zeros((3, 0, 4), dtype=np.uint64))
    assert not got.any() and is_id.tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------
# succinct_check and check on the committed openings
# ---------------------------------------------------------------------------------------------
def load_case(golden, corc, key, reverse_srs=False):
    """Uploads the recipe SRS of the case's length with the reference's (S, H); (cname, C, d, z, v, pi)."""
    cname = key.split("_")[1]
    n = int(key.split("_")[2][1:])
    S, Hh = golden[f"ref_sh_{cname}"]
    g = corc.srs_generate(cname, n)
    group.PublicParams.upload(cname, np.ascontiguousarray(g[::-1]) if reverse_srs else g, S, Hh, precompute_windows=True)
    z, v = G[key + "_zv"]
    pi = {"Ls": G[key + "_Ls"].copy(), "Rs": G[key + "_Rs"].copy(), "U": G[key + "_U"][0].copy(), "c": G[key + "_c"][0].copy(),
          "C_bar": None, "w_prime": None}
    if key.endswith("hiding"):
        pi["C_bar"] = G[key + "_Cbar"][0].copy()
        pi["w_prime"] = G[key + "_wprime_alpha"][0].copy()
    return cname, G[key + "_C"][0].copy(), n - 1, z.copy(), v.copy(), pi


@pytest.mark.parametrize("key", CASES)
def test_succinct_check_and_check_accept_the_fixture(hal, golden, corc, key):
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    t = SpongeAdapter(cname)
    h, U = pcdl.succinct_check(C, d, z, v, pi, t, curve=cname)
    assert np.array_equal(h.xis, G[key + "_xis"]), key
    assert np.array_equal(U, G[key + "_U"][0])
    if key.endswith("hiding"):  # the first challenge of a hiding check is alpha (pcdl.rs:510)
        assert np.array_equal(t.challenges[0], G[key + "_wprime_alpha"][1]), key
        assert len(t.challenges) == len(h.xis) + 1
    else:
        assert len(t.challenges) == len(h.xis)
    pcdl.check(C, d, z, v, pi, SpongeAdapter(cname), curve=cname)


def test_succinct_check_rejects_tampered_proofs(hal, golden, corc):
    key = "open_pallas_n16_plain"
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    m = P.CURVES[cname].scalar
    msg = "C_\\(log_n\\) ≠ CM.Commit_Σ\\(c \\|\\| v'\\)$"
    pcdl.succinct_check(C, d, z, v, pi, SpongeAdapter(cname), curve=cname)
    with pytest.raises(pcdl.CheckFailed, match=msg):
        pcdl.succinct_check(C, d, z, plus_one(v, m), pi, SpongeAdapter(cname), curve=cname)
    with pytest.raises(pcdl.CheckFailed, match=msg):
        pcdl.succinct_check(C, d, z, v, dict(pi, c=plus_one(pi["c"], m)), SpongeAdapter(cname), curve=cname)
    Ls, Rs = pi["Ls"].copy(), pi["Rs"].copy()
    Ls[0], Rs[0] = pi["Rs"][0], pi["Ls"][0]
    with pytest.raises(pcdl.CheckFailed, match=msg):
        pcdl.succinct_check(C, d, z, v, dict(pi, Ls=Ls, Rs=Rs), SpongeAdapter(cname), curve=cname)
    with pytest.raises(pcdl.CheckFailed, match=msg):
        pcdl.succinct_check(C, d, z, v, dict(pi, U=pi["Ls"][1]), SpongeAdapter(cname), curve=cname)
    with pytest.raises(pcdl.CheckFailed, match=msg):  # check() reports the succinct check's failure
        pcdl.check(C, d, z, plus_one(v, m), pi, SpongeAdapter(cname), curve=cname)


def test_succinct_check_rejects_a_tampered_hiding_proof(hal, golden, corc):
    key = "open_vesta_n16_hiding"
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    m = P.CURVES[cname].scalar
    pcdl.succinct_check(C, d, z, v, pi, SpongeAdapter(cname), curve=cname)
    with pytest.raises(pcdl.CheckFailed, match="C_\\(log_n\\) ≠ CM.Commit_Σ\\(c \\|\\| v'\\)$"):
        pcdl.succinct_check(C, d, z, v, dict(pi, w_prime=plus_one(pi["w_prime"], m)), SpongeAdapter(cname), curve=cname)


def test_check_rejects_another_srs(hal, golden, corc):
    """Over the reversed SRS the succinct check still passes (it reads only H) and the decider's
    commitment to h differs from U."""
    key = "open_pallas_n16_plain"
    cname, C, d, z, v, pi = load_case(golden, corc, key, reverse_srs=True)
    pcdl.succinct_check(C, d, z, v, pi, SpongeAdapter(cname), curve=cname)
    with pytest.raises(pcdl.CheckFailed, match="^U ≠ CM.Commit\\(ck, h_vec\\)$"):
        pcdl.check(C, d, z, v, pi, SpongeAdapter(cname), curve=cname)


def test_batch_verdicts(hal, golden, corc):
    key = "open_pallas_n16_plain"
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    m = P.CURVES[cname].scalar
    k = 5
    vs = np.stack([v] * k)
    cs = np.stack([pi["c"]] * k)
    vs[1] = plus_one(v, m)
    cs[3] = plus_one(pi["c"], m)
    ok = pcdl.succinct_check_verdicts(np.stack([C] * k), d, np.stack([z] * k), vs, np.concatenate([G[key + "_xis"]] * k),
                                      np.concatenate([pi["Ls"]] * k), np.concatenate([pi["Rs"]] * k), np.stack([pi["U"]] * k),
                                      cs, curve=cname)
    assert ok.tolist() == [1, 0, 1, 0, 1]
    # succinct_check_many names the first failing instance
    insts = [pcdl.Instance(C, d, z, vs[i], dict(pi, c=cs[i])) for i in range(k)]
    with pytest.raises(pcdl.CheckFailed, match="instance 1") as e:
        pcdl.succinct_check_many(insts, [SpongeAdapter(cname) for _ in range(k)], curve=cname)
    assert e.value.index == 1


def test_succinct_check_batch_errors(hal, golden, corc):
    """d > D carries the reference's text (pcdl.rs:494), a zero xi_(j+1) has no inverse (pcdl.rs:537 unwraps
    it) and a scalar that is not below the modulus is an argument error: all before any device work."""
    key = "open_pallas_n16_plain"
    cname, C, d, z, v, pi = load_case(golden, corc, key)
    xis = G[key + "_xis"].copy()

    def call(d_, xis_, z_=z):
        return pcdl.succinct_check_verdicts(C[None], d_, z_[None], v[None], xis_, pi["Ls"][: (d_ + 1).bit_length() - 1],
                                            pi["Rs"][: (d_ + 1).bit_length() - 1], pi["U"][None], pi["c"][None], curve=cname)

    assert call(d, xis).tolist() == [1]
    with pytest.raises(AssertionError, match="d was larger than D!"):
        call(31, np.concatenate([xis, xis[:1]]))
    zero = xis.copy()
    zero[2] = 0
    with pytest.raises(hal.HaloError, match=r"EINVAL.*halo_pcdl_succinct_check_batch: xi_2 of instance 0 is zero"):
        call(d, zero)
    zero0 = xis.copy()
    zero0[0] = 0  # xi_0 is never inverted: a verdict, not an error
    assert call(d, zero0).tolist() in ([0], [1])
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    with pytest.raises(hal.HaloError, match="halo_pcdl_succinct_check_batch: a scalar of instance 0 is not below"):
        call(d, xis, big)
    with pytest.raises(pcdl.CheckFailed, match="d was larger than D!"):
        pcdl.succinct_check(C, 31, z, v, pi, SpongeAdapter(cname), curve=cname)
    with pytest.raises(AssertionError, match=r"n \(11\) is not a power of two"):
        pcdl.succinct_check(C, 10, z, v, pi, SpongeAdapter(cname), curve=cname)


# ---------------------------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------------------------
def test_accumulation(hal, golden, corc):
    cname, n = "pallas", 16
    c = P.CURVES[cname]
    m = c.scalar
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, corc.srs_generate(cname, n), S, Hh, precompute_windows=True)

    def new_transcript(label):
        return SpongeAdapter(cname, label)

    qs = []
    for i in range(3):
        ins = det_scalars(500 + i, n + 1)
        p, z = ins[:n], ins[n]
        C = pcdl.commit(p, n - 1, curve=cname)
        pi = pcdl.open(p, C, n - 1, z, transcript=new_transcript("PCDL"), curve=cname)
        qs.append(pcdl.Instance(C, n - 1, z, pi["v"], pi))
    a = acc.prover(qs, new_transcript, curve=cname)
    # alpha, C and z recomputed with the oracle: the instances' xis from the oracle's own succinct check
    xis = [pcdl_check.succinct_check_transcript(cname, q.C, q.d, P.from_mont(P.limbs_to_int(q.z), m),
                                                P.from_mont(P.limbs_to_int(q.v), m), q.pi["Ls"], q.pi["Rs"], q.pi["U"],
                                                P.from_mont(P.limbs_to_int(q.pi["c"]), m), Hh) for q in qs]
    Us = [unwrapped(c, q.pi["U"]) for q in qs]
    sp = poseidon.Sponge(cname, poseidon.ASDL)
    sp.absorb_fr([x for xs in xis for x in xs])
    sp.absorb_g(Us)
    alpha = sp.challenge()
    Cexp = P.INF
    for i, U in enumerate(Us):
        Cexp = P.add(c, Cexp, P.mul_fast(c, pow(alpha, i, m), U))
    zexp = sp.challenge()
    C_bar, d, z, hs, alphas = acc.common_subroutine(qs, new_transcript, curve=cname)
    assert np.array_equal(alphas[1], fe(alpha, m)) and np.array_equal(alphas[2], fe(alpha * alpha, m))
    assert np.array_equal(C_bar, wrapped(c, Cexp)) and np.array_equal(z, fe(zexp, m)) and d == n - 1
    assert np.array_equal(a.C, wrapped(c, Cexp)) and np.array_equal(a.z, fe(zexp, m)) and a.d == n - 1
    vexp = sum(pow(alpha, i, m) * pcdl_check.h_eval(xs, zexp, m) for i, xs in enumerate(xis)) % m
    assert np.array_equal(a.v, fe(vexp, m)) and np.array_equal(a.pi["v"], a.v)
    acc.verifier(qs, a, new_transcript, curve=cname)
    acc.decider(a, new_transcript, curve=cname)
    bad = list(qs)
    bad[1] = qs[1]._replace(v=plus_one(qs[1].v, m))
    with pytest.raises(pcdl.CheckFailed, match="instance 1"):
        acc.common_subroutine(bad, new_transcript, curve=cname)
    with pytest.raises(pcdl.CheckFailed, match="^z' = z$"):
        acc.verifier(qs, a._replace(z=plus_one(a.z, m)), new_transcript, curve=cname)
    with pytest.raises(pcdl.CheckFailed, match="^h\\(z\\) = v$"):
        acc.verifier(qs, a._replace(v=plus_one(a.v, m)), new_transcript, curve=cname)
