"""GPU tests of the generator's fixed-base comb and of batched Schnorr signing (halo_amd/csrc/fixed_base.hip):
halo_generator_mul_batch limb for limb against the CPU restatement's public_key over the edge scalars of
tests/fixed_base_cases.py and at the batch sizes where the shared inversion's workgroups begin and end,
halo_schnorr_sign_batch bit for bit against the restatement's sign (tests/schnorr_ref.py over oracle/pasta.py), a
round trip through the library's own verifiers, the _dev forms, and the wrappers that draw the scalars.  Both curves.
"""
import ctypes
import os

import numpy as np
import pytest

import pasta as P
import schnorr_ref as SR
from fixed_base_cases import edge_scalars

pytestmark = pytest.mark.gpu

CURVES = ["pallas", "vesta"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")


@pytest.fixture(scope="module")
def sch(hal):
    """halo_amd.schnorr with the reference's Poseidon constants installed for both fields."""
    from halo_amd import schnorr
    g = np.load(GOLDEN)
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    return schnorr


_pk = {}


def expected_pk(cname, x):
    """SR.public_key as a WrappedPoint row, memoised per distinct scalar (shared by every test, never changed)."""
    if (cname, x) not in _pk:
        _pk[(cname, x)] = SR.points(cname, [SR.public_key(cname, x)])[0]
    return _pk[(cname, x)]


def expected_pks(cname, xs):
    return np.array([expected_pk(cname, x) for x in xs], dtype=np.uint64).reshape(-1, 8)


def rand_scalars(rng, m, n):
    return [int.from_bytes(rng.bytes(40), "little") % m for _ in range(n)]


@pytest.fixture(scope="module")
def pool():
    """Per curve 1025 seeded random scalars (distinct), the inputs of the batch-boundary cases."""
    rng = np.random.default_rng(20261021)
    return {c: rand_scalars(rng, P.CURVES[c].scalar, 1025) for c in CURVES}


# ---------------------------------------------------------------------------------------------
# 1. the comb over the edge scalars
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_generator_mul_edge_scalars(sch, cname):
    r = P.CURVES[cname].scalar
    E = edge_scalars(cname)
    got = sch.public_key_batch(SR.fe_rows(E, r), cname)
    exp = expected_pks(cname, E)
    assert got.dtype == np.uint64 and got.shape == exp.shape
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [hex(E[i]) for i in bad[:8]]
    assert E[0] == 0 and not got[0].any()  # 0 G = (0, 0)
    # the doubling case and its negative are each other's negatives: same x, y + y' = 0
    i, j = E.index((1 << 255) - r), E.index(2 * r - (1 << 255))
    assert np.array_equal(got[i, :4], got[j, :4]) and not np.array_equal(got[i, 4:], got[j, 4:])


# ---------------------------------------------------------------------------------------------
# 2. batch boundaries: identities inside a shared inversion
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize("cname", CURVES)
def test_generator_mul_batch_boundaries(sch, pool, cname, k):
    r = P.CURVES[cname].scalar
    xs = list(pool[cname][:k])
    for z in (0, k // 2, k - 1):
        xs[z] = 0
    got = sch.public_key_batch(SR.fe_rows(xs, r), cname)
    exp = expected_pks(cname, xs)
    assert np.array_equal(got, exp), np.nonzero((got != exp).any(axis=1))[0][:8]
    assert not got[0].any() and not got[k // 2].any() and not got[k - 1].any()


@pytest.mark.parametrize("cname", CURVES)
def test_generator_mul_all_identities_and_a_single_point(sch, pool, cname):
    """257 zeros: no workgroup has anything to invert.  257 with one nonzero scalar: one workgroup inverts a
    product of a single factor, the others nothing."""
    r = P.CURVES[cname].scalar
    got = sch.public_key_batch(np.zeros((257, 4), dtype=np.uint64), cname)
    assert got.shape == (257, 8) and not got.any()
    for at in (0, 130, 256):
        xs = [0] * 257
        xs[at] = pool[cname][at]
        got = sch.public_key_batch(SR.fe_rows(xs, r), cname)
        assert np.array_equal(got, expected_pks(cname, xs)), at
        assert got[at].any()


# ---------------------------------------------------------------------------------------------
# 3. signing parity
# ---------------------------------------------------------------------------------------------
def msg_rows(msgs, m, k, msg_len):
    return np.array([SR.fe_rows(mm, m) for mm in msgs], dtype=np.uint64).reshape(k, msg_len, 4)


@pytest.mark.parametrize("msg_len", [0, 1, 10, 11])
@pytest.mark.parametrize("cname", CURVES)
def test_sign_batch_parity(hal, sch, cname, msg_len):
    c = P.CURVES[cname]
    r, k = c.scalar, 65
    rng = np.random.default_rng(7000 + 16 * CURVES.index(cname) + msg_len)
    sk, nonce = rand_scalars(rng, r, k), rand_scalars(rng, r, k)
    nonce[3] = 0                  # R = (0, 0), s = e sk
    sk[5] = 0                     # pk = (0, 0), s = nonce
    nonce[8] = r - 1
    sk[13] = r - 1
    nonce[21] = (1 << 255) - r    # the comb's doubling case
    sk[34], nonce[34] = 0, 0      # both at once: R = pk = (0, 0), s = 0
    nonce[64] = 2 * r - (1 << 255)
    msgs = [tuple(rand_scalars(rng, c.base, msg_len)) for _ in range(k)]
    exp = [SR.sign(cname, sk[i], nonce[i], msgs[i]) for i in range(k)]
    exp_R = SR.points(cname, [e[0] for e in exp])
    exp_s = SR.fe_rows([e[1] for e in exp], r)
    assert exp[3][0] is None and exp[34] == (None, 0) and exp[5][1] == nonce[5]
    pk = expected_pks(cname, sk)
    marr = msg_rows(msgs, c.base, k, msg_len)
    sk_a, nonce_a = SR.fe_rows(sk, r), SR.fe_rows(nonce, r)
    for lanes in (1, 3):
        with hal.tuning(poseidon_lanes=lanes):
            for given in (None, pk):
                R, s = sch.sign_batch(sk_a, marr, cname, nonces=nonce_a, pk=given)
                assert R.shape == (k, 8) and s.shape == (k, 4)
                assert np.array_equal(R, exp_R), (lanes, given is None, np.nonzero((R != exp_R).any(axis=1))[0])
                assert np.array_equal(s, exp_s), (lanes, given is None, np.nonzero((s != exp_s).any(axis=1))[0])
    # a pk that is passed is hashed as given: another key changes s and leaves R alone
    other = np.roll(pk, 1, axis=0)
    R, s = sch.sign_batch(sk_a, marr, cname, nonces=nonce_a, pk=other)
    assert np.array_equal(R, exp_R)
    assert (s != exp_s).any(axis=1).sum() >= k - 3  # all but the items whose sk is 0 (e sk = 0 whatever e)


# ---------------------------------------------------------------------------------------------
# 4. round trip through the library's verifiers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """Per curve k = 4099 random keys, nonces and 10-element messages, as integers and as ABI arrays."""
    out = {}
    for cname in CURVES:
        c = P.CURVES[cname]
        k = 4099
        rng = np.random.default_rng(4099 + CURVES.index(cname))
        sk, nonce = rand_scalars(rng, c.scalar, k), rand_scalars(rng, c.scalar, k)
        msgs = [tuple(rand_scalars(rng, c.base, 10)) for _ in range(k)]
        out[cname] = dict(k=k, sk=sk, nonce=nonce, msgs=msgs, sk_a=SR.fe_rows(sk, c.scalar), nonce_a=SR.fe_rows(nonce, c.scalar),
                          msgs_a=msg_rows(msgs, c.base, k, 10))
    return out


@pytest.mark.parametrize("cname", CURVES)
def test_round_trip_sign_then_verify(sch, big, cname):
    c = P.CURVES[cname]
    b = big[cname]
    k = b["k"]
    pk = sch.public_key_batch(b["sk_a"], cname)
    R, s = sch.sign_batch(b["sk_a"], b["msgs_a"], cname, nonces=b["nonce_a"])
    R2, s2 = sch.sign_batch(b["sk_a"], b["msgs_a"], cname, nonces=b["nonce_a"], pk=pk)
    assert np.array_equal(R, R2) and np.array_equal(s, s2)
    assert sch.verify_batch(pk, R, s, b["msgs_a"], cname).all()
    ok, comb = sch.verify_batch(pk, R, s, b["msgs_a"], cname, rhos="fs", return_combined=True)
    assert ok.all() and comb == 1
    # one message element of item 7 changed: item 7 alone is rejected, by both verifiers
    bad = b["msgs_a"].copy()
    bad[7, 4] = SR.fe((b["msgs"][7][4] + 1) % c.base, c.base)
    want = np.ones(k, dtype=np.uint8)
    want[7] = 0
    assert np.array_equal(sch.verify_batch(pk, R, s, bad, cname), want)
    assert np.array_equal(sch.verify_batch(pk, R, s, bad, cname, rhos="fs"), want)
    # 16 sampled items against the restatement
    for i in np.random.default_rng(16).choice(k, 16, replace=False):
        eR, es = SR.sign(cname, b["sk"][i], b["nonce"][i], b["msgs"][i])
        assert np.array_equal(R[i], SR.points(cname, [eR])[0]) and SR.from_fe(s[i], c.scalar) == es, i
        assert np.array_equal(pk[i], expected_pk(cname, b["sk"][i])), i


# ---------------------------------------------------------------------------------------------
# 5. the _dev forms
# ---------------------------------------------------------------------------------------------
def _dev(t):
    return ctypes.c_void_p(t.data_ptr())


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("cname", CURVES)
def test_dev_variants_match_and_are_asynchronous(hal, sch, big, cname):
    """Over torch device tensors the _dev forms give the host forms' bytes, and they are asynchronous: several
    signing batches are queued and the stream is still busy when the last call has returned (the queued work is tens
    of host call times long; a host stalled for longer than that between the two lines would fail this spuriously)."""
    import torch
    L = hal.load()
    curve = hal.CURVES[cname]
    b = big[cname]
    k = b["k"]
    pk = sch.public_key_batch(b["sk_a"], cname)
    R, s = sch.sign_batch(b["sk_a"], b["msgs_a"], cname, nonces=b["nonce_a"])
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    d_sk, d_n, d_m, d_pk = _cuda(b["sk_a"]), _cuda(b["nonce_a"]), _cuda(b["msgs_a"]), _cuda(pk)
    d_out = torch.zeros((k, 8), dtype=torch.int64, device="cuda")
    hal.check(L.halo_generator_mul_batch_dev(curve, _dev(d_sk), k, _dev(d_out), sp))
    assert np.array_equal(_host(d_out), pk)
    rounds = 8
    d_R = torch.zeros((rounds, k, 8), dtype=torch.int64, device="cuda")
    d_s = torch.zeros((rounds, k, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for q in range(rounds):  # even rounds derive pk, odd rounds take it
        hal.check(L.halo_schnorr_sign_batch_dev(curve, _dev(d_sk), _dev(d_pk) if q & 1 else None, _dev(d_n), _dev(d_m), 10, k,
                                                _dev(d_R[q]), _dev(d_s[q]), sp))
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy, "halo_schnorr_sign_batch_dev returned only after its work had finished"
    hR, hs = _host(d_R), _host(d_s)
    for q in range(rounds):
        assert np.array_equal(hR[q], R) and np.array_equal(hs[q], s), q
    # the secrets the caller passed are untouched
    assert np.array_equal(_host(d_sk), b["sk_a"]) and np.array_equal(_host(d_n), b["nonce_a"])


# ---------------------------------------------------------------------------------------------
# 6. the wrappers that draw the scalars
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CURVES)
def test_generate_keypairs_and_drawn_nonces(sch, cname):
    c = P.CURVES[cname]
    sk, pk = sch.generate_keypairs(64, cname)
    assert sk.shape == (64, 4) and pk.shape == (64, 8)
    ints = [SR.from_fe(x, c.scalar) for x in sk]
    assert all(0 < x < c.scalar for x in ints) and len(set(ints)) == 64
    assert all(P.limbs_to_int(x) < c.scalar for x in sk)  # canonical limbs
    assert np.array_equal(pk, sch.public_key_batch(sk, cname))
    assert np.array_equal(pk[0], expected_pk(cname, ints[0]))
    # 64 signatures of one message under one key: fresh nonces, so pairwise distinct R, and all verify
    msg = SR.fe_rows(rand_scalars(np.random.default_rng(6), c.base, 10), c.base)
    msgs = np.repeat(msg.reshape(1, 10, 4), 64, axis=0)
    one_sk, one_pk = np.repeat(sk[:1], 64, axis=0), np.repeat(pk[:1], 64, axis=0)
    R, s = sch.sign_batch(one_sk, msgs, cname)
    assert len({bytes(x) for x in R}) == 64 and R.any(axis=1).all()
    assert sch.verify_batch(one_pk, R, s, msgs, cname).all()
