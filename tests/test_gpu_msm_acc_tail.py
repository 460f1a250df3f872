"""GPU parity of the bucket accumulation's peeled second addition (k_acc: a chunk's second entry adds
to the affine copy of its first, curve.hpp xyzz_madd_run_aff), of the tail's chain addition
(xyzz_add_acc in k_merge, k_rowcol, k_bitterms) and of k_merge's split of a bucket's sources over
its lanes.

Every MSM here goes through the asynchronous entry over the resident window-shifted SRS
(halo_msm_dev_async with null bases), which takes the bucket pipeline (k_acc and the reduction tail)
at every length; the synchronous entries serve n <= 8192 from the multiples table instead.  Results
are checked against (sum_j s_j k_j) G with the known discrete logs k_j of a synthetic SRS, or against
(sum_j s_j) Q over an uploaded SRS whose points all equal Q.
"""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import pasta as P
from halo_amd import group, pcdl

pytestmark = pytest.mark.gpu
C = P.PALLAS
R = C.scalar
SEED = 29


def fe(vals, m=R):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def fe_rep(v, n):
    return np.ascontiguousarray(np.repeat(fe([v]), n, axis=0))


def wrapped(pt):
    return P.point_to_wrapped(C, pt)


class acc_launches:
    """Counts the k_acc launches inside the block (the library's "msm_acc" profile slot), so that a test
    which claims to run k_acc fails when its call takes another path."""

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


def srs_msm(hal, sc):
    """sum_j sc_j G_j over the resident SRS prefix by the asynchronous entry (the bucket pipeline: one
    k_acc launch, checked)."""
    import torch
    L = hal.load()
    n = len(sc)
    d = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with acc_launches(hal) as prof:
        hal.check(L.halo_msm_dev_async(0, None, ctypes.c_void_p(d.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), sp))
        hal.check(L.halo_msm_join(sp))
        torch.cuda.synchronize()
    assert prof.count == 1, prof.count
    return list(out.cpu().numpy().view(np.uint64))


_LOGS = {}


def logs(n):
    """Discrete logs of the synthetic SRS's first n points (computed once per length)."""
    if n not in _LOGS:
        _LOGS[n] = [group.synth_scalar(SEED, j) % R for j in range(n)]
    return _LOGS[n]


def log_point(acc):
    return wrapped(P.mul_fast(C, acc % R, C.generator))


@pytest.fixture(scope="module")
def equal_point():
    return P.mul_fast(C, 0x1234567, C.generator)


def upload_equal(Q, n):
    g = np.ascontiguousarray(np.repeat(np.array(wrapped(Q), dtype=np.uint64)[None, :], n, axis=0))
    group.PublicParams.upload("pallas", g, precompute_windows=True)


def test_peeled_step_lengths_and_sparse(hal):
    """Random scalars at n = 1, 2, 3, 17, 2^12 over a 2^12 synthetic SRS (chunks of one and two entries, a
    last chunk cut by the count), and mostly-zero scalars (bucket boundaries between a chunk's first and
    second entry)."""
    N = 1 << 12
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)
    ks = logs(N)
    rng = random.Random(1)
    for n in (1, 2, 3, 17, N):
        s = [rng.randrange(R) for _ in range(n)]
        assert srs_msm(hal, fe(s)) == log_point(sum(a * k for a, k in zip(s, ks))), n
    for n, keep in ((17, 5), (N, 64), (N, 1500)):
        s = [0] * n
        for j in rng.sample(range(n), keep):
            s[j] = rng.randrange(R)
        assert srs_msm(hal, fe(s)) == log_point(sum(a * k for a, k in zip(s, ks))), (n, keep)


def test_peeled_step_doubling_and_cancellation(hal, equal_point):
    """An SRS whose points all equal Q.  All-equal scalars: a bucket's entries are one point with one
    sign, so every chunk's second addition is the doubling case.  Scalars alternating s, r - s: the
    entries alternate in sign, so every second addition cancels and the lane starts fresh again."""
    N = 1 << 12
    upload_equal(equal_point, N)
    s = 0x1F2E3D4C5B6A79881726354 % R
    for n in (2, 3, 17, N):
        assert srs_msm(hal, fe([s] * n)) == wrapped(P.mul_fast(C, s * n % R, equal_point)), n
        alt = [s if j % 2 == 0 else R - s for j in range(n)]
        exp = wrapped(P.mul_fast(C, s, equal_point)) if n % 2 else wrapped(P.INF)
        assert srs_msm(hal, fe(alt)) == exp, n


def test_peeled_step_variable_base_glv(hal):
    """The variable-base path (GLV entries: the peeled steps meet phi points) at n = 2^10."""
    n = 1 << 10
    group.PublicParams.synthesize("pallas", n, SEED, precompute_windows=False)
    g = group.PublicParams.read("pallas", 0, n)
    ks = logs(n)
    rng = random.Random(2)
    s = [rng.randrange(R) for _ in range(n)]
    with acc_launches(hal) as prof:
        got = list(group.point_dot_affine(fe(s), g, "pallas"))
    assert prof.count == 1, prof.count
    assert got == log_point(sum(a * k for a, k in zip(s, ks)))
    s2 = [s[0]] * n  # one bucket per window and half: the peeled step's doubling test on distinct points
    assert list(group.point_dot_affine(fe(s2), g, "pallas")) == log_point(s[0] * sum(ks))


def test_peeled_step_ipa_pair_round(hal):
    """One pair MSM (L and R of an opening's first round as one MSM with (side, bucket) keys, the R side's
    points at poly_off) at length 2^12: L = <c_hi, G_lo> + <c_hi, z_lo> H', R = <c_lo, G_hi> + <c_lo, z_hi> H'
    (pcdl.rs:404-438).  With the default tuning a session of n <= ipa_srs_tail_n = 4096 starts in the tail
    rounds over the SRS's multiples table and never launches k_acc, so the session is pinned to the weighted
    rounds (ipa_srs_tail_n = 0, as tests/test_gpu_transcript.py pins them): n = 4096 > 2048 runs weighted and
    its first round, 2048 terms per side, is a pair MSM through k_acc."""
    n = 1 << 12
    m = n // 2
    group.PublicParams.synthesize("pallas", n, SEED, precompute_windows=True)
    ks = logs(n)
    rng = random.Random(3)
    cs = [rng.randrange(R) for _ in range(n)]
    z = rng.randrange(R)
    h = rng.randrange(1, R)
    zs = P.construct_powers(z, n, R)
    expL = sum(c * k for c, k in zip(cs[m:], ks[:m])) + P.scalar_dot(cs[m:], zs[:m], R) * h
    expR = sum(c * k for c, k in zip(cs[:m], ks[m:])) + P.scalar_dot(cs[:m], zs[m:], R) * h
    with hal.tuning(ipa_srs_tail_n=0):
        ses = pcdl.IpaSession(fe(cs), fe([z]), np.array(log_point(h), dtype=np.uint64), "pallas")
        with acc_launches(hal) as prof:
            Lp, Rp = ses.round_lr()
        assert prof.count == 1, prof.count  # L and R together: one k_acc launch
        got = list(Lp), list(Rp)
        # finish the opening (returns the session to the pool)
        rounds = n.bit_length() - 1
        xi = None
        for k in range(rounds):
            hsh = hashlib.sha3_256((b"" if xi is None else xi.tobytes()) + Lp.tobytes() + Rp.tobytes())
            xi = fe([int.from_bytes(hsh.digest(), "little") % R or 1])[0]
            ses.fold(xi)
            if k + 1 < rounds:
                Lp, Rp = ses.round_lr()
        ses.end()
    assert got[0] == log_point(expL)
    assert got[1] == log_point(expR)


@pytest.mark.parametrize("lgn", [12, 16])
def test_tail_chain_long_buckets(hal, lgn):
    """All-equal and two-valued scalars at n = 2^12 and 2^16 over a 2^16 synthetic SRS: a window's
    entries fall into one or two buckets, so k_merge sums long runs of chunk partials and the group
    sums."""
    N = 1 << 16
    n = 1 << lgn
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)
    ks = logs(N)
    s1, s2 = R - 99, (1 << 201) + 3
    lo, hi = sum(ks[: n // 2]), sum(ks[n // 2:n])
    assert srs_msm(hal, fe_rep(s1, n)) == log_point(s1 * (lo + hi))
    assert srs_msm(hal, np.concatenate([fe_rep(s1, n // 2), fe_rep(s2, n // 2)])) == log_point(s1 * lo + s2 * hi)


@pytest.mark.parametrize("lgn", [12, 16])
def test_tail_chain_equal_points_doubling_in_merge(hal, equal_point, lgn):
    """The same scalars over an SRS of 2^16 equal points: equal chunks have equal partial sums, so
    k_merge's additions (and the group sums') meet the doubling case."""
    N = 1 << 16
    n = 1 << lgn
    upload_equal(equal_point, N)
    s1, s2 = R - 99, (1 << 201) + 3
    assert srs_msm(hal, fe_rep(s1, n)) == wrapped(P.mul_fast(C, s1 * n % R, equal_point))
    exp = (s1 + s2) * (n // 2) % R
    assert srs_msm(hal, np.concatenate([fe_rep(s1, n // 2), fe_rep(s2, n // 2)])) == wrapped(P.mul_fast(C, exp, equal_point))


def test_tail_chain_pairwise_cancellation(hal, corc):
    """Scalars s_j on the first half and r - s_j on the second over an SRS with G[j + n/2] = G[j]: every
    bucket's sum is the identity, met in k_merge as q = -acc, and so is the result."""
    n = 1 << 12
    g = corc.srs_generate("pallas", n // 2)
    group.PublicParams.upload("pallas", np.ascontiguousarray(np.concatenate([g, g])), precompute_windows=True)
    rng = random.Random(4)
    s = [rng.randrange(1, R) for _ in range(n // 2)]
    assert srs_msm(hal, fe(s + [R - a for a in s])) == wrapped(P.INF)


def sources_per_bucket(sizes, K):
    """(sources, starts on a chunk boundary) of k_merge for consecutive buckets of the given sizes in
    chunks of K sorted entries."""
    out, pos = set(), 0
    for m in sizes:
        out.add(((pos + m - 1) // K - pos // K + 1, pos % K == 0))
        pos += m
    return out


@pytest.mark.parametrize("n", [512, 2048, 4096])
def test_merge_split_small_buckets(hal, n):
    """Small scalars (one nonzero digit, in window 0) with multiplicities 1, 2, ..., 10 repeating: consecutive
    buckets of 1 .. 10 entries at every offset inside the chunks.  At the chunk lengths of these sizes
    (msm_plan.hpp msm_chunk_len: ceil(sqrt(17 n / 2^14)) = 1, 2, 3) the buckets have 1, 2, 3, 4 and more
    sources, odd and even counts, starting on a chunk boundary and inside a chunk.  The library has no query
    for the chunk length it picked, so the source counts are asserted on a model of the sorted layout for
    K = 2 and 3 only (at K = 1 a bucket of m entries has m sources); that the plan gives these K at these n
    rests on msm_plan.hpp's formula and is not checked here.  The MSM itself is a parity check."""
    N = 1 << 12
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)
    ks = logs(N)
    sizes, vals, d = [], [], 1
    while len(vals) < n:
        m = min((d - 1) % 10 + 1, n - len(vals))
        sizes.append(m)
        vals += [d] * m
        d += 1
    for K in (2, 3):
        got = sources_per_bucket(sizes, K)
        assert {(c, st) for c in (1, 2, 3, 4) for st in (False, True)} <= got, K
    random.Random(5).shuffle(vals)
    assert srs_msm(hal, fe(vals)) == log_point(sum(a * k for a, k in zip(vals, ks)))
