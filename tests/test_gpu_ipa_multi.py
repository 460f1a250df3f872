"""The session lists of halo_ipa_round_lr_multi, halo_ipa_fold_multi and halo_ipa_end_multi: one validator refuses a
session listed twice and a session that is not open, names the call and the index, and runs before the call touches
any session, so a refused call leaves every listed session where it was."""
import ctypes
import random

import numpy as np
import pytest

import pasta as P
from halo_amd import group, pcdl

pytestmark = pytest.mark.gpu
HALO_EINVAL = 1
N = 4


def fe(vals, m):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def handles(*sessions):
    return (ctypes.c_void_p * len(sessions))(*[s._s.value for s in sessions])


@pytest.mark.parametrize("kind", ["srs", "vectors"])  # tail rounds over the SRS's table; explicit G, folded
def test_multi_calls_refuse_a_bad_list_and_touch_nothing(hal, corc, kind):
    c = P.PALLAS
    r = c.scalar
    g = corc.srs_generate("pallas", N)
    group.PublicParams.upload("pallas", g, precompute_windows=False)
    Hp = np.array(P.point_to_wrapped(c, P.mul_fast(c, 3, c.generator)), dtype=np.uint64)
    L = hal.load()
    rng = random.Random(23)
    inputs = [([rng.randrange(r) for _ in range(N)], rng.randrange(r)) for _ in range(2)]

    def begin(cs, z):
        if kind == "srs":
            return pcdl.IpaSession(fe(cs, r), fe([z], r), Hp, "pallas")
        return pcdl.IpaSession.from_vectors(g[:N], fe(cs, r), fe(P.construct_powers(z, N, r), r), Hp, "pallas")

    # every session exists before one is ended: a later begin would take the ended one's object from the pool
    # and its handle would be open again
    a = [begin(*i) for i in inputs]
    fresh = [begin(*i) for i in inputs]
    ended = begin(*inputs[0])
    h_ended = ended._s.value
    ended.end()

    xi = fe([5, 7, 9], r)
    xinv = fe([P.inv(5, r), P.inv(7, r), P.inv(9, r)], r)
    Lb, Rb = np.zeros((3, 8), dtype=np.uint64), np.zeros((3, 8), dtype=np.uint64)

    def rounds(sessions):
        k = len(sessions)
        hal.check(L.halo_ipa_round_lr_multi(handles(*sessions), k, hal.ptr(Lb), hal.ptr(Rb)))
        return Lb[:k].copy(), Rb[:k].copy()

    def folds(sessions):
        hal.check(L.halo_ipa_fold_multi(handles(*sessions), len(sessions), hal.ptr(xi), hal.ptr(xinv)))

    # one round and one fold in, so that a fold is pending in the tail rounds when the refused calls arrive
    first = rounds(a)
    folds(a)

    h = [s._s.value for s in a]
    twice = (ctypes.c_void_p * 3)(h[0], h[1], h[0])
    closed = (ctypes.c_void_p * 3)(h[0], h[1], h_ended)
    calls = {
        "halo_ipa_round_lr_multi": lambda arr, k: L.halo_ipa_round_lr_multi(arr, k, hal.ptr(Lb), hal.ptr(Rb)),
        "halo_ipa_fold_multi": lambda arr, k: L.halo_ipa_fold_multi(arr, k, hal.ptr(xi), hal.ptr(xinv)),
        "halo_ipa_end_multi": lambda arr, k: L.halo_ipa_end_multi(arr, k, None, None),
    }
    for name, call in calls.items():
        assert call(twice, 3) == HALO_EINVAL
        assert hal.last_error() == "%s: session 2 listed twice" % name
        assert call(closed, 3) == HALO_EINVAL
        assert hal.last_error().startswith("%s: session 2 is not open" % name)
        # the two-entry lists of the same kinds
        assert call((ctypes.c_void_p * 2)(h[0], h[0]), 2) == HALO_EINVAL
        assert hal.last_error() == "%s: session 1 listed twice" % name
        assert call((ctypes.c_void_p * 2)(h[0], h_ended), 2) == HALO_EINVAL
        assert hal.last_error().startswith("%s: session 1 is not open" % name)

    # nothing was advanced, folded or released: the same two sessions go on exactly as two fresh ones do
    assert all(np.array_equal(x, y) for x, y in zip(first, rounds(fresh)))
    folds(fresh)
    second, second_fresh = rounds(a), rounds(fresh)
    assert np.array_equal(second[0], second_fresh[0]) and np.array_equal(second[1], second_fresh[1])
    folds(a)
    folds(fresh)
    got, exp = pcdl.IpaSession.end_many(a), pcdl.IpaSession.end_many(fresh)
    for (U, c0), (U1, c1) in zip(got, exp):
        assert np.array_equal(U, U1) and np.array_equal(c0, c1)
