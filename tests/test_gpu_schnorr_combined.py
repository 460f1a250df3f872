"""GPU tests of the combined Schnorr batch (halo_amd/csrc/schnorr_combined.hip): one MSM of 2 k + 1 terms under random
or derived weights in place of k ladders.  Expected verdicts always come from the CPU restatement of the reference
(tests/schnorr_ref.py, memoised), the derived weights from tests/schnorr_combined_ref.py; the exact call
(verify_batch(rhos=None)) must agree as well.  Both curves.  Items are drawn from a small pool of signatures, so a
large k costs the oracle nothing."""
import ctypes
import os

import numpy as np
import pytest

import pasta as P
import schnorr_combined_ref as CR
import schnorr_ref as SR

pytestmark = pytest.mark.gpu

CURVES = ["pallas", "vesta"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
# k_sig_prepare reduces rho_i s_i over blocks of 256 items and k_sig_sum, one block of 256 threads, sums the partials:
# 257 items make two partials, 65 537 make 257, so that a thread of the final sum loops twice.
SUM_LOOPS_TWICE = 256 * 256 + 1


@pytest.fixture(scope="module")
def sch(hal):
    """halo_amd.schnorr with the reference's Poseidon constants installed for both fields."""
    from halo_amd import schnorr
    g = np.load(GOLDEN)
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    return schnorr


class Items:
    """Distinct items (pk, msg, R, s), encoded once, with the restatement's verdicts; a batch is an index array."""

    def __init__(self, cname, msg_len, items):
        c = P.CURVES[cname]
        self.cname, self.msg_len, self.items = cname, msg_len, items
        self.pk = SR.points(cname, [it[0] for it in items])
        self.R = SR.points(cname, [it[2] for it in items])
        self.s = SR.fe_rows([it[3] for it in items], c.scalar)
        self.msgs = np.array([SR.fe_rows(it[1], c.base) for it in items], dtype=np.uint64).reshape(len(items), msg_len, 4)
        self.exp = np.array([SR.verify(cname, *it) for it in items], dtype=np.uint8)

    def take(self, idx):
        idx = np.asarray(idx)
        return (self.pk[idx], self.R[idx], self.s[idx], self.msgs[idx]), self.exp[idx]


def variants(cname, msg_len):
    """The pool's six valid items, then the special ones by name."""
    c = P.CURVES[cname]
    sks, pool = CR.signature_pool(cname, msg_len)
    pk, msg, R, s = pool[0]
    other = pool[1]
    named = {
        "s_plus_1": (pk, msg, R, (s + 1) % c.scalar),
        "other_pk": (other[0], msg, R, s),
        "other_R": (pk, msg, other[2], s),
        "pk_off_curve": (((pk[0] + 1) % c.base, pk[1]), msg, R, s),
        "R_off_curve": (pk, msg, (R[0], (R[1] + 1) % c.base), s),
        "dead_and_wrong": (((pk[0] + 1) % c.base, pk[1]), msg, R, (s + 1) % c.scalar),
    }
    if msg_len:
        named["altered_msg"] = (pk, msg[:-1] + ((msg[-1] + 1) % c.base,), R, s)
    R0, s0 = SR.sign(cname, 0, 777, msg)  # sk = 0: pk = identity, s = the nonce
    named["pk_identity"] = (None, msg, R0, s0)
    Rn, sn = SR.sign(cname, sks[1], 0, msg)  # nonce 0: R = identity, s = e sk
    named["R_identity"] = (SR.public_key(cname, sks[1]), msg, Rn, sn)
    Rp, sp = SR.sign(cname, sks[2], sks[2], msg)  # nonce = sk: R = pk
    named["R_equals_pk"] = (SR.public_key(cname, sks[2]), msg, Rp, sp)
    names = list(named)
    return Items(cname, msg_len, pool + [named[n] for n in names]), {n: len(pool) + j for j, n in enumerate(names)}


@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(cname, msg_len):
        if (cname, msg_len) not in cache:
            cache[(cname, msg_len)] = variants(cname, msg_len)
        return cache[(cname, msg_len)]
    return get


def rand_rho(k, seed):
    """k uniform ark scalars below 2^254, so below either modulus; nonzero but for a chance of 2^-254."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)
    return a


def small_rho(cname, ws):
    return SR.fe_rows(ws, P.CURVES[cname].scalar)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _dev(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def combined_dev(hal, cname, arrs, rho, stream=None):
    """halo_schnorr_verify_combined_dev over resident inputs -> (ok bytes, combined byte); rho None: derived."""
    import torch
    pk, R, s, msgs = arrs
    k, msg_len = len(pk), msgs.shape[1]
    d = [_cuda(x) for x in (pk, R, s, msgs)]
    d_rho = _cuda(rho) if rho is not None else None
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_comb = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = stream or torch.cuda.current_stream()
    hal.check(hal.load().halo_schnorr_verify_combined_dev(hal.CURVES[cname], *[_dev(t) for t in d], msg_len, k, _dev(d_rho),
                                                          _dev(d_ok), _dev(d_comb), ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    return d_ok.cpu().numpy(), int(d_comb.cpu()[0])


@pytest.mark.parametrize("msg_len", [10, 0])
@pytest.mark.parametrize("cname", CURVES)
def test_all_valid_under_random_weights(hal, sch, data, cname, msg_len):
    it, _ = data(cname, msg_len)
    for k in (1, 2, 3, 16, 17, 257, SUM_LOOPS_TWICE):
        arrs, exp = it.take(np.arange(k) % 6)
        assert exp.all()
        got, comb = sch.verify_batch(*arrs, cname, rhos=rand_rho(k, k), return_combined=True)
        assert comb == 1, k
        assert got.dtype == np.uint8 and np.array_equal(got, exp), k
        if k <= 257:
            assert np.array_equal(sch.verify_batch(*arrs, cname), exp), k
            dok, dcomb = combined_dev(hal, cname, arrs, rand_rho(k, k + 1))
            assert dcomb == 1 and np.array_equal(dok, exp), k


@pytest.mark.parametrize("wrong", ["s_plus_1", "altered_msg", "other_pk", "other_R"])
@pytest.mark.parametrize("cname", CURVES)
def test_exactly_one_wrong_item(hal, sch, data, cname, wrong):
    it, at = data(cname, 10)
    k = 17
    for pos in (0, k // 2, k - 1):
        idx = np.arange(k) % 6
        idx[pos] = at[wrong]
        arrs, exp = it.take(idx)
        assert exp.sum() == k - 1 and exp[pos] == 0
        got, comb = sch.verify_batch(*arrs, cname, rhos=rand_rho(k, pos), return_combined=True)
        assert comb == 0 and np.array_equal(got, exp), pos
        assert np.array_equal(sch.verify_batch(*arrs, cname), exp)
        dok, dcomb = combined_dev(hal, cname, arrs, rand_rho(k, pos))
        assert dcomb == 0 and not dok.any(), pos


@pytest.mark.parametrize("cname", CURVES)
def test_weights_are_applied_to_every_term(hal, sch, data, cname):
    """s_0 + x, s_1 - x: weights known in advance, (1, 1), let the pair through -- the algebra, and the reason the header
    demands weights drawn after the signatures are fixed.  Any others do not."""
    c = P.CURVES[cname]
    it, _ = data(cname, 10)
    (pk, R, s, msgs), _ = it.take([0, 1])
    x = 987654321
    a, b = it.items[0], it.items[1]
    s = SR.fe_rows([(a[3] + x) % c.scalar, (b[3] - x) % c.scalar], c.scalar)
    assert not SR.verify(cname, a[0], a[1], a[2], (a[3] + x) % c.scalar)
    assert not SR.verify(cname, b[0], b[1], b[2], (b[3] - x) % c.scalar)
    dok, dcomb = combined_dev(hal, cname, (pk, R, s, msgs), small_rho(cname, [1, 1]))
    assert dcomb == 1 and dok.tolist() == [1, 1]
    got, comb = sch.verify_batch(pk, R, s, msgs, cname, rhos=small_rho(cname, [1, 2]), return_combined=True)
    assert comb == 0 and got.tolist() == [0, 0]
    got, comb = sch.verify_batch(pk, R, s, msgs, cname, rhos="fs", return_combined=True)
    assert comb == 0 and got.tolist() == [0, 0]
    assert sch.verify_batch(pk, R, s, msgs, cname).tolist() == [0, 0]


@pytest.mark.parametrize("cname", CURVES)
def test_items_that_are_not_live(hal, sch, data, cname):
    """A pk or an R off the curve: verdict 0, no weight in D, and the batch does not fall back on their account."""
    it, at = data(cname, 10)
    for dead in (["pk_off_curve"], ["R_off_curve"], ["pk_off_curve", "R_off_curve", "dead_and_wrong"]):
        idx = list(np.arange(9) % 6)
        for j, name in enumerate(dead):
            idx[1 + 3 * j] = at[name]
        arrs, exp = it.take(idx)
        assert exp.sum() == 9 - len(dead)
        for rhos in (rand_rho(9, 3), "fs"):
            got, comb = sch.verify_batch(*arrs, cname, rhos=rhos, return_combined=True)
            assert comb == 1 and np.array_equal(got, exp), dead
        assert np.array_equal(sch.verify_batch(*arrs, cname), exp)
        dok, dcomb = combined_dev(hal, cname, arrs, rand_rho(9, 4))
        assert dcomb == 1 and np.array_equal(dok, exp)
    arrs, exp = it.take([at["pk_off_curve"]])  # a batch of one that is not live: nothing to check, nothing accepted
    got, comb = sch.verify_batch(*arrs, cname, rhos=rand_rho(1, 1), return_combined=True)
    assert comb == 1 and got.tolist() == [0]


@pytest.mark.parametrize("cname", CURVES)
def test_identity_points(hal, sch, data, cname):
    """pk = (0, 0) signed by sk = 0 and R = (0, 0) from the nonce 0 are legal points: the MSM skips an identity base."""
    it, at = data(cname, 10)
    for idx in ([at["pk_identity"]], [at["R_identity"]], [0, at["pk_identity"], 1, at["R_identity"], at["pk_identity"]]):
        arrs, exp = it.take(idx)
        assert exp.all()
        for rhos in (rand_rho(len(idx), 9), "fs"):
            got, comb = sch.verify_batch(*arrs, cname, rhos=rhos, return_combined=True)
            assert comb == 1 and np.array_equal(got, exp), idx
        assert np.array_equal(sch.verify_batch(*arrs, cname), exp)


@pytest.mark.parametrize("cname", CURVES)
def test_equal_points(hal, sch, data, cname):
    """Equal and repeated bases inside the MSM's buckets: 65 copies of one signature (under distinct weights and under
    equal ones, which put the copies into the same buckets), and items whose R is their pk."""
    it, at = data(cname, 10)
    arrs, exp = it.take([2] * 65)
    for rho in (rand_rho(65, 2), np.repeat(rand_rho(1, 3), 65, axis=0)):
        got, comb = sch.verify_batch(*arrs, cname, rhos=rho, return_combined=True)
        assert comb == 1 and got.all()
    arrs, exp = it.take([0, at["R_equals_pk"], 1, at["R_equals_pk"]])
    assert exp.all() and np.array_equal(arrs[0][1], arrs[1][1])
    got, comb = sch.verify_batch(*arrs, cname, rhos=rand_rho(4, 4), return_combined=True)
    assert comb == 1 and got.all()
    assert np.array_equal(sch.verify_batch(*arrs, cname), exp)


@pytest.mark.parametrize("msg_len", [10, 0])
@pytest.mark.parametrize("cname", CURVES)
def test_derived_weights(hal, sch, data, cname, msg_len):
    it, at = data(cname, msg_len)
    for k in (1, 2, 3, 5, 21, 22, 64, 65):
        idx = list(np.arange(k) % 6)
        if k >= 5:
            idx[3] = at["R_off_curve"]
        arrs, exp = it.take(idx)
        want = CR.weights(cname, [it.items[j] for j in idx], msg_len)
        assert all(want[j].any() == (idx[j] != at["R_off_curve"]) for j in range(k))
        for lanes in (1, 3):
            with hal.tuning(poseidon_lanes=lanes):
                got = sch.batch_weights(*arrs, cname)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (k, lanes)
        a = sch.verify_batch(*arrs, cname, rhos="fs", return_combined=True)
        b = sch.verify_batch(*arrs, cname, rhos="fs", return_combined=True)
        assert a[1] == b[1] == 1 and np.array_equal(a[0], b[0]) and np.array_equal(a[0], exp), k
        dok, dcomb = combined_dev(hal, cname, arrs, None)
        assert dcomb == 1 and np.array_equal(dok, exp), k
        # the derived weights are what "fs" ran under: passed back by the caller, the same verdicts
        if k >= 5:
            live_w = got.copy()
            live_w[3] = 1  # the host form refuses a zero weight; the item is not live and its weight is not read
            c = sch.verify_batch(*arrs, cname, rhos=live_w, return_combined=True)
            assert c[1] == 1 and np.array_equal(c[0], exp)


@pytest.mark.parametrize("cname", CURVES)
def test_dev_form_rejects_a_bad_weight_of_a_live_item(hal, sch, data, cname):
    """The _dev form cannot refuse on the host: a live item whose rho is zero or not below the modulus gives combined = 0."""
    it, at = data(cname, 10)
    arrs, exp = it.take([0, 1, at["pk_off_curve"], 2])
    rho = rand_rho(4, 6)
    rho[2] = 0  # not live: not read
    dok, dcomb = combined_dev(hal, cname, arrs, rho)
    assert dcomb == 1 and np.array_equal(dok, exp)
    for bad in (0, 0xFFFFFFFFFFFFFFFF):
        r = rho.copy()
        r[1] = bad
        dok, dcomb = combined_dev(hal, cname, arrs, r)
        assert dcomb == 0 and not dok.any()


def test_dev_form_on_a_side_stream_then_the_exact_call(hal, sch, data):
    """Inputs resident, a non-default stream, and an exact _dev call right behind on the same stream: both use the
    challenges' buffer, the stream orders them."""
    import torch
    cname = "pallas"
    it, at = data(cname, 10)
    k = 300
    arrs, exp = it.take(np.arange(k) % 6)
    idx = np.arange(k) % 6
    idx[::7] = at["s_plus_1"]
    arrs2, exp2 = it.take(idx)
    side = torch.cuda.Stream()
    d2 = [_cuda(x) for x in arrs2]
    d_ok2 = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d = [_cuda(x) for x in arrs]
    d_rho = _cuda(rand_rho(k, 8))
    d_ok = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_ok3 = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    d_comb = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = hal.load()
    curve = hal.CURVES[cname]
    sp = ctypes.c_void_p(side.cuda_stream)
    hal.check(L.halo_schnorr_verify_combined_dev(curve, *[_dev(t) for t in d], 10, k, _dev(d_rho), _dev(d_ok), _dev(d_comb), sp))
    hal.check(L.halo_schnorr_verify_batch_dev(curve, *[_dev(t) for t in d2], 10, k, _dev(d_ok2), sp))
    # a third call on the default stream, enqueued behind the two: derived weights over the batch with wrong items
    hal.check(L.halo_schnorr_verify_combined_dev(curve, *[_dev(t) for t in d2], 10, k, None, _dev(d_ok3), None,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert int(d_comb.cpu()[0]) == 1 and np.array_equal(d_ok.cpu().numpy(), exp)
    assert np.array_equal(d_ok2.cpu().numpy(), exp2)
    assert not d_ok3.cpu().numpy().any()  # a rejected batch: the _dev form never falls back
