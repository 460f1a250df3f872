"""GPU parity of k_acc's mixed addition with three carry chains (curve.hpp xyzz_madd_run, xyzz_madd_run_aff,
xyzz_run_out): the running sum carries its sign apart and X as signed limbs, and every store (a chunk's
first and last partial, a bucket inside the chunk) settles X and applies the sign.
tests/test_acc_three_chains.py models the step on the CPU.

The SRS cases go through the asynchronous entry over the resident window-shifted SRS (halo_msm_dev_async
with null bases: the bucket pipeline at every length, exactly one k_acc launch, asserted) and are checked
against (sum_j s_j k_j) G with the known discrete logs k_j of a 2^12 synthetic SRS, or against
(sum_j s_j) Q over an uploaded SRS whose points all equal Q.  Signs inside one bucket come from the signed
digits: a scalar a and a scalar 2^200 - a have the digits +a and -a in window 0 whatever the window width
(a small), so they meet in one bucket with opposite signs.
"""
import ctypes
import random

import numpy as np
import pytest

import pasta as P
from halo_amd import group

pytestmark = pytest.mark.gpu
C = P.PALLAS
R = C.scalar
SEED = 29
N = 1 << 12
BIG = 1 << 200


def fe(vals, m=R):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def wrapped(pt):
    return P.point_to_wrapped(C, pt)


class acc_launches:
    """Counts the k_acc launches inside the block (the library's "msm_acc" profile slot)."""

    def __init__(self, hal):
        self.hal, self.L, self.count = hal, hal.load(), 0

    def __enter__(self):
        self.L.halo_profile_reset()
        self.L.halo_profile_enable(1)
        return self

    def __exit__(self, *exc):
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        self.hal.check(self.L.halo_profile_read(b"msm_acc", ctypes.byref(n), ctypes.byref(ms)))
        self.L.halo_profile_enable(0)
        self.count = n.value


def srs_msm(hal, vals):
    """sum_j vals_j G_j over the resident SRS prefix by the asynchronous entry; one k_acc launch, checked."""
    import torch
    L = hal.load()
    d = torch.from_numpy(np.ascontiguousarray(fe(vals)).view(np.int64)).cuda()
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with acc_launches(hal) as prof:
        hal.check(L.halo_msm_dev_async(0, None, ctypes.c_void_p(d.data_ptr()), len(vals), ctypes.c_void_p(out.data_ptr()), sp))
        hal.check(L.halo_msm_join(sp))
        torch.cuda.synchronize()
    assert prof.count == 1, prof.count
    return list(out.cpu().numpy().view(np.uint64))


@pytest.fixture(scope="module")
def logs():
    """Discrete logs of the 2^12 synthetic SRS (computed once)."""
    return [group.synth_scalar(SEED, j) % R for j in range(N)]


@pytest.fixture()
def synth_srs(hal):
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)


@pytest.fixture(scope="module")
def equal_point():
    return P.mul_fast(C, 0x1234567, C.generator)


@pytest.fixture()
def equal_srs(hal, equal_point):
    g = np.ascontiguousarray(np.repeat(np.array(wrapped(equal_point), dtype=np.uint64)[None, :], N, axis=0))
    group.PublicParams.upload("pallas", g, precompute_windows=True)


def log_point(acc):
    return wrapped(P.mul_fast(C, acc % R, C.generator))


def check_logs(hal, logs, vals):
    assert srs_msm(hal, vals) == log_point(sum(a * k for a, k in zip(vals, logs))), len(vals)


def test_random_scalars_by_length(hal, synth_srs, logs):
    """n = 1 .. 5, 17 (chunks of one entry: the copy alone, stored with s = +-1) and 2^12."""
    rng = random.Random(1)
    for n in (1, 2, 3, 4, 5, 17, N):
        check_logs(hal, logs, [rng.randrange(R) for _ in range(n)])


@pytest.mark.parametrize("n", [40, N])
def test_long_buckets_of_mixed_signs(hal, synth_srs, logs, n):
    """Three magnitudes in both signs, d and r - d, then a and 2^200 - a for a = 1, 2, 3: a window's entries
    fall into a few long buckets, window 0's with both signs in any order, so segments of every length end
    at both parities of s in a chunk's first, inner and last store."""
    rng = random.Random(2)
    ds = (5, (1 << 100) + 12345, (1 << 250) + 99)
    check_logs(hal, logs, [rng.choice((d, R - d)) for d in (rng.choice(ds) for _ in range(n))])
    check_logs(hal, logs, [rng.choice((a, BIG - a)) for a in (rng.randrange(1, 4) for _ in range(n))])
    check_logs(hal, logs, [rng.choice((1, BIG - 1)) for _ in range(n)])  # one bucket in window 0


def test_mostly_zero_scalars(hal, synth_srs, logs):
    """Sparse scalars: one-entry segments, stored as the copy with s = +1 or -1."""
    rng = random.Random(3)
    for n, keep in ((17, 5), (N, 64), (N, 1500)):
        s = [0] * n
        for j in rng.sample(range(n), keep):
            s[j] = rng.choice((rng.randrange(R), rng.randrange(1, 1 << 12), BIG - rng.randrange(1, 1 << 12)))
        check_logs(hal, logs, s)


def test_equal_points_doubling_at_every_step(hal, equal_srs, equal_point):
    """All points equal, all scalars equal: a bucket's entries are one point with one sign, so the peeled
    addition doubles and every later one meets q = acc again or adds to a multiple."""
    s = 0x1F2E3D4C5B6A79881726354 % R
    for n, v in ((2, s), (5, s), (17, BIG - 3), (N, s), (N, BIG - 3)):
        assert srs_msm(hal, [v] * n) == wrapped(P.mul_fast(C, v * n % R, equal_point)), (n, v)


def test_equal_points_cancellation_and_restart(hal, equal_srs, equal_point):
    """All points equal, scalars alternating s and r - s, and a and 2^200 - a (+a and -a in window 0's one
    bucket: every second addition cancels and the lane starts fresh), plus one extra of either sign."""
    s = 0x1F2E3D4C5B6A79881726354 % R
    for pos, negv in ((s, R - s), (3, BIG - 3)):
        for n in (2, 17, N):
            alt = [pos if j % 2 == 0 else negv for j in range(n)]
            for extra in ([], [pos], [negv]):
                vals = alt + extra
                if len(vals) > N:
                    vals = vals[1:]  # the SRS has 2^12 points: drop the first instead
                tot = sum(vals) % R
                exp = wrapped(P.mul_fast(C, tot, equal_point)) if tot else wrapped(P.INF)
                assert srs_msm(hal, vals) == exp, (pos, n, len(extra))


def test_variable_base_33_points(hal, corc):
    """The smallest variable-base MSM that takes the bucket pipeline (GLV entries, phi points)."""
    n = 33
    g = corc.srs_generate("pallas", n)
    rng = random.Random(4)
    sc = fe([rng.randrange(R) for _ in range(n - 3)] + [5, R - 5, BIG - 5])
    with acc_launches(hal) as prof:
        got = group.point_dot_affine(sc, g, "pallas")
    assert prof.count == 1, prof.count
    assert np.array_equal(got, corc.msm("pallas", g, sc))


def test_batch_4_by_1024(hal, corc):
    """halo_msm_batch_dev: four polynomials of 2^10 coefficients as one MSM with (polynomial, bucket) keys."""
    import torch
    L = hal.load()
    n, k = 1 << 10, 4
    g = corc.srs_generate("pallas", n)
    group.PublicParams.upload("pallas", g, precompute_windows=True)
    rng = random.Random(5)
    scs = [fe([rng.choice((rng.randrange(R), rng.randrange(1, 4), BIG - rng.randrange(1, 4))) for _ in range(n)])
           for _ in range(k)]
    dev = [torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda() for sc in scs]
    ptrs = (ctypes.c_void_p * k)(*[d.data_ptr() for d in dev])
    lns = (ctypes.c_size_t * k)(*[n] * k)
    out = torch.zeros((k, 8), dtype=torch.int64, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with acc_launches(hal) as prof:
        hal.check(L.halo_msm_batch_dev(0, ptrs, lns, k, ctypes.c_void_p(out.data_ptr()), sp))
        hal.check(L.halo_msm_join(sp))
        torch.cuda.synchronize()
    assert prof.count == 1, prof.count
    got = out.cpu().numpy().view(np.uint64)
    for i in range(k):
        assert np.array_equal(got[i], corc.msm("pallas", g, scs[i])), i
