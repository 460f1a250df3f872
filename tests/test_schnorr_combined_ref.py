"""CPU tests of the tests' own oracle for the combined Schnorr batch (tests/schnorr_combined_ref.py), against the
restatement of the reference's verification (tests/schnorr_ref.py), on batches of 1 to 5 items: D is the identity iff
every live item verifies, the cancelling pair that fixed weights let through, and the derived weights bind what they
should."""
import numpy as np
import pytest

import pasta as P
import schnorr_combined_ref as CR
import schnorr_ref as SR

CURVES = ["pallas", "vesta"]
MSG_LEN = 2


def rand_weights(cname, k, seed=5):
    m = P.CURVES[cname].scalar
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % (m - 1) + 1 for _ in range(k)]


def wrong_variants(cname, item, other):
    """One item per class of error: s + 1, an altered message, another signer's pk, the R of another signature."""
    c = P.CURVES[cname]
    pk, msg, R, s = item
    return [(pk, msg, R, (s + 1) % c.scalar), (pk, msg[:-1] + ((msg[-1] + 1) % c.base,), R, s), (other[0], msg, R, s),
            (pk, msg, other[2], s)]


@pytest.mark.parametrize("cname", CURVES)
def test_defect_is_identity_iff_every_live_item_verifies(cname):
    c = P.CURVES[cname]
    _, pool = CR.signature_pool(cname, MSG_LEN)
    for k in range(1, 6):
        items = pool[:k]
        rhos = rand_weights(cname, k, seed=k)
        assert all(SR.verify(cname, *it) for it in items)
        assert CR.defect(cname, items, rhos) is None, k
        for pos in {0, k // 2, k - 1}:
            for bad in wrong_variants(cname, items[pos], pool[(pos + 1) % len(pool)]):
                assert not SR.verify(cname, *bad)
                assert CR.defect(cname, items[:pos] + [bad] + items[pos + 1:], rhos) is not None, (k, pos)
    # an item that is not live weighs nothing, whatever else is wrong with it
    pk, msg, R, s = pool[1]
    for dead in ((((pk[0] + 1) % c.base, pk[1]), msg, R, s + 1), (pk, msg, (R[0], (R[1] + 1) % c.base), s)):
        assert not CR.live(cname, dead) and not SR.verify(cname, *dead)
        assert CR.defect(cname, [pool[0], dead, pool[2]], rand_weights(cname, 3)) is None


@pytest.mark.parametrize("cname", CURVES)
def test_identity_points_take_part(cname):
    """pk = identity signed by sk = 0 and R = identity from the nonce 0 are legal and verify; a wrong s beside them shows."""
    c = P.CURVES[cname]
    sks, pool = CR.signature_pool(cname, MSG_LEN)
    msg = pool[0][1]
    R0, s0 = SR.sign(cname, 0, 777, msg)
    idpk = (None, msg, R0, s0)
    Rn, sn = SR.sign(cname, sks[1], 0, msg)
    idR = (SR.public_key(cname, sks[1]), msg, Rn, sn)
    assert Rn is None and SR.verify(cname, *idpk) and SR.verify(cname, *idR)
    for items in ([idpk], [idR], [pool[0], idpk, idR]):
        assert CR.defect(cname, items, rand_weights(cname, len(items))) is None
    assert CR.defect(cname, [(None, msg, R0, (s0 + 1) % c.scalar)], [3]) is not None


@pytest.mark.parametrize("cname", CURVES)
def test_cancelling_pair(cname):
    """s_0 + x and s_1 - x: both items are wrong, weights fixed in advance as (1, 1) let them through, any weights that
    differ do not.  This is why the weights are drawn after the signatures are fixed."""
    c = P.CURVES[cname]
    _, pool = CR.signature_pool(cname, MSG_LEN)
    x = 123456789
    a, b = pool[0], pool[1]
    pair = [(a[0], a[1], a[2], (a[3] + x) % c.scalar), (b[0], b[1], b[2], (b[3] - x) % c.scalar)]
    assert not SR.verify(cname, *pair[0]) and not SR.verify(cname, *pair[1])
    assert CR.defect(cname, pair, [1, 1]) is None
    assert CR.defect(cname, pair, [1, 2]) is not None
    assert CR.defect(cname, pair, CR.weights_int(cname, pair, MSG_LEN)) is not None


@pytest.mark.parametrize("cname", CURVES)
def test_derived_weights_bind_the_batch(cname):
    c = P.CURVES[cname]
    _, pool = CR.signature_pool(cname, MSG_LEN)
    for k in range(1, 6):
        items = pool[:k]
        w = CR.weights_int(cname, items, MSG_LEN)
        assert len(w) == k and all(0 < x < c.scalar for x in w) and len(set(w)) == k
        es = [CR.challenge(cname, it) for it in items]
        ss = [it[3] for it in items]
        on = [True] * k
        assert CR.weights_from(cname, es, ss, on, MSG_LEN) == w
        for i in range(k):
            for which in (es, ss):
                alt = list(which)
                alt[i] = (alt[i] + 1) % c.scalar
                w2 = CR.weights_from(cname, alt if which is es else es, alt if which is ss else ss, on, MSG_LEN)
                assert all(x != y for x, y in zip(w, w2)), (k, i)
        assert all(x != y for x, y in zip(w, CR.weights_from(cname, es, ss, on, MSG_LEN + 1)))
        assert all(x != y for x, y in zip(w, CR.weights_from(cname, es, ss, on, MSG_LEN, k=k + 1)))
        assert all(x != y for x, y in zip(w, CR.weights_int(cname, pool[:k + 1], MSG_LEN)))
    # an item that is not live has weight 0 and the leaf 0, whatever it holds
    pk, msg, R, s = pool[1]
    dead = (((pk[0] + 1) % c.base, pk[1]), msg, R, s)
    w = CR.weights_int(cname, [pool[0], dead, pool[2]], MSG_LEN)
    assert w[1] == 0 and w[0] and w[2]
    assert w == CR.weights_int(cname, [pool[0], (dead[0], msg, R, s + 5), pool[2]], MSG_LEN)
