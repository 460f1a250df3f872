"""GPU: chunk partials stored raw by k_acc and settled by their loader (curve.hpp partial_store /
partial_load; msm_tail.hip k_group_sums, k_merge), through whole MSMs against the C oracle's MSM.

k_acc stores a chunk's first and last running sums as it holds them (X signed-lazy, the sign of Y in a
spare bit) and k_merge / k_group_sums apply xyzz_run_out's two carry chains on loading; k_merge counts chunk
t0's partial as lane 0's first source.  Every MSM goes through the asynchronous entry over the resident
window-shifted SRS (halo_msm_dev_async with null bases: the bucket pipeline at every length, one k_acc launch,
checked).  At n = 4096 and 2048 over 4096 points the default copies are 15 bits wide and a chunk has K = 3
and 2 entries (msm_plan.hpp msm_chunk_len: ceil(sqrt(17 n / 2^14))); the library has no query for K, so that
rests on the plan's formula as in tests/test_gpu_msm_acc_tail.py.
  * buckets of 1, K - 1, K, K + 1 entries in turn, at every offset inside the chunks: partials of one to
    K entries, first and last segments, buckets written by k_acc beside buckets merged from partials;
  * all-equal and two-valued scalars: a bucket of 4096 or 2048 entries, >= 64 K, so k_group_sums loads raw
    partials and feeds settled ones (s = 0) to the same loader in k_merge;
  * an SRS of equal points (known logs, q = +-acc): all-equal scalars make every addition a doubling, in
    k_acc and in the merge; scalars alternating s, r - s cancel, so lanes restart and store identities;
  * an SRS with G[j + n/2] = G[j] and scalars s_j, r - s_j: every bucket is a pair that cancels, so the
    segments of every chunk are the identity (as partials: the fresh state, or what a cancellation left), alone
    and beside a few buckets that do not cancel.
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
SEED = 37
N = 1 << 12


def fe(vals, m=R):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def srs_msm(hal, sc):
    """sum_j sc_j G_j over the resident SRS prefix by the asynchronous entry (one k_acc launch, checked)."""
    import torch
    L = hal.load()
    n = len(sc)
    d = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    hal.check(L.halo_msm_dev_async(0, None, ctypes.c_void_p(d.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), sp))
    hal.check(L.halo_msm_join(sp))
    torch.cuda.synchronize()
    cnt, ms = ctypes.c_size_t(0), ctypes.c_double(0)
    hal.check(L.halo_profile_read(b"msm_acc", ctypes.byref(cnt), ctypes.byref(ms)))
    L.halo_profile_enable(0)
    assert cnt.value == 1, cnt.value
    return out.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def synthetic(hal):
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)
    assert hal.load().halo_srs_window_bits(0) == 15
    return group.PublicParams.read("pallas", 0, N)


@pytest.mark.parametrize("n,K", [(4096, 3), (2048, 2)])
def test_bucket_sizes_around_the_chunk_length(hal, corc, synthetic, n, K):
    """Small scalars (one nonzero digit, in window 0) with multiplicities 1, K - 1, K, K + 1 repeating."""
    assert -(-17 * n // (1 << 14)) <= K * K and 17 * n > (K - 1) ** 2 << 14  # K = ceil(sqrt(17 n / 2^14))
    cycle = (1, K - 1, K, K + 1)
    vals, d = [], 1
    while len(vals) < n:
        m = min(cycle[(d - 1) % 4], n - len(vals))
        vals += [d] * m
        d += 1
    assert d < 1 << 14  # below 2^(c - 1): one positive digit
    random.Random(5).shuffle(vals)
    sc = fe(vals)
    assert np.array_equal(srs_msm(hal, sc), corc.msm("pallas", synthetic[:n], sc)), n


@pytest.mark.parametrize("n", [4096, 2048])
def test_long_buckets_through_the_group_sums(hal, corc, synthetic, n):
    """All-equal scalars (one bucket of n entries per window, some with the folded sign) and two values."""
    for vals in ([R - 99] * n, [(1 << 201) + 3] * n, [R - 99] * (n // 2) + [(1 << 201) + 3] * (n // 2)):
        sc = fe(vals)
        assert np.array_equal(srs_msm(hal, sc), corc.msm("pallas", synthetic[:n], sc)), n


def test_equal_points_doubling_and_cancellation(hal):
    """G_j = Q for every j (log 0x1234567): q = +-acc at every addition."""
    Q = P.mul_fast(C, 0x1234567, C.generator)
    g = np.ascontiguousarray(np.repeat(np.array(P.point_to_wrapped(C, Q), dtype=np.uint64)[None, :], N, axis=0))
    group.PublicParams.upload("pallas", g, precompute_windows=True)
    s = 0x1F2E3D4C5B6A79881726354 % R
    for n in (3, 193, N):
        got = srs_msm(hal, fe([s] * n))
        assert list(got) == P.point_to_wrapped(C, P.mul_fast(C, s * n % R, Q)), n
        alt = [s if j % 2 == 0 else R - s for j in range(n)]
        exp = P.point_to_wrapped(C, P.mul_fast(C, s, Q)) if n % 2 else P.point_to_wrapped(C, P.INF)
        assert list(srs_msm(hal, fe(alt))) == exp, n


def test_segments_that_cancel_to_the_identity(hal, corc):
    """G[j + n/2] = G[j], scalars s_j and r - s_j: every bucket holds a point and its negative."""
    n = N
    g = corc.srs_generate("pallas", n // 2)
    bases = np.ascontiguousarray(np.concatenate([g, g]))
    group.PublicParams.upload("pallas", bases, precompute_windows=True)
    rng = random.Random(4)
    s = [rng.randrange(1, R) for _ in range(n // 2)]
    vals = s + [R - a for a in s]
    assert list(srs_msm(hal, fe(vals))) == P.point_to_wrapped(C, P.INF)
    for j in rng.sample(range(n), 40):  # a few buckets that do not cancel among the ones that do
        vals[j] = rng.randrange(1, R)
    sc = fe(vals)
    assert np.array_equal(srs_msm(hal, sc), corc.msm("pallas", bases, sc))
