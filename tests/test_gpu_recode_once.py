"""GPU: the fused first sort pass recodes every scalar once (sort.hip k_rs_hist_sc folds and stores,
k_rs_scatter cuts the windows from the stored words), against the C oracle's MSM.

Every MSM goes through the asynchronous entry over the resident window-shifted SRS
(halo_msm_dev_async with null bases: the bucket pipeline at every length, one k_acc launch, checked) with
copies of an explicit width c = 16 and c = 17 (halo_srs_precompute_window_range), so the fused pass with
its constant-width recodings runs at small n: n = 1, 511, 513 (one thread short of and one past a tile of
512 scalars) and 4097 (nine tiles, the last with one scalar).  Scalars: random, all equal, two-valued,
all (p - 1) / 2 and all (p + 1) / 2 (the two sides of the fold: the largest integer kept and the smallest
one replaced by p - s), all zero.  One pair MSM (two outputs, P = 2: an IPA round's L and R) of 4096
terms per side on each curve reads the stored words at 2 (p n + i).
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
SEED = 31
N = 4608
SIZES = (1, 511, 513, 4097)
KINDS = ("random", "all_equal", "two_values", "half_minus", "half_plus", "zero")


def fe(vals, m=R):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def scalars(kind, n):
    rng = random.Random(len(kind) * 1000 + n)
    if kind == "random":
        return [rng.randrange(R) for _ in range(n)]
    if kind == "all_equal":
        return [R - 424242] * n
    if kind == "two_values":
        return [R - 99] * (n // 2) + [(1 << 201) + 3] * (n - n // 2)
    if kind == "half_minus":
        return [(R - 1) // 2] * n
    if kind == "half_plus":
        return [(R + 1) // 2] * n
    return [0] * n


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


@pytest.fixture(scope="module", params=(16, 17))
def shifted(request, hal):
    """(c, the SRS's points): N synthetic points with full window-shifted copies of width c."""
    c_s = request.param
    L = hal.load()
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=False)
    hal.check(L.halo_srs_precompute_window_range(0, c_s, 0, 0))
    assert L.halo_srs_window_bits(0) == c_s
    return c_s, group.PublicParams.read("pallas", 0, N)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_pass_msm_equals_oracle(hal, corc, shifted, kind):
    c_s, bases = shifted
    assert hal.load().halo_srs_window_bits(0) == c_s and group.PublicParams.len("pallas") == N
    for n in SIZES:
        sc = fe(scalars(kind, n))
        got = srs_msm(hal, sc)
        assert np.array_equal(got, corc.msm("pallas", bases[:n], sc)), (c_s, kind, n)


@pytest.mark.parametrize("curve,c_s", [(P.PALLAS, 17), (P.VESTA, 16)], ids=["pallas-c17", "vesta-c16"])
def test_pair_msm_round(hal, curve, c_s):
    """An opening's first weighted round at length 8192: L and R as one MSM of two outputs, 4096 terms per
    side, recoded in the fused pass (17-bit keys at c = 17: an 8- and a 9-bit pass; 16-bit keys at c = 16).
    L = <c_hi, G_lo> + <c_hi, z_lo> H', R = <c_lo, G_hi> + <c_lo, z_hi> H', from the synthetic SRS's logs."""
    r = curve.scalar
    n = 1 << 13
    m = n // 2
    L = hal.load()
    cid = hal.CURVES[curve.name]
    group.PublicParams.synthesize(curve.name, n, SEED, precompute_windows=False)
    hal.check(L.halo_srs_precompute_window_range(cid, c_s, 0, 0))
    assert L.halo_srs_window_bits(cid) == c_s
    ks = [group.synth_scalar(SEED, j, curve.name) % r for j in range(n)]
    rng = random.Random(3 + c_s)
    cs = [rng.randrange(r) for _ in range(n)]
    z = rng.randrange(r)
    h = rng.randrange(1, r)
    zs = P.construct_powers(z, n, r)
    expL = sum(c * k for c, k in zip(cs[m:], ks[:m])) + P.scalar_dot(cs[m:], zs[:m], r) * h
    expR = sum(c * k for c, k in zip(cs[:m], ks[m:])) + P.scalar_dot(cs[:m], zs[m:], r) * h

    def log_point(acc):
        return P.point_to_wrapped(curve, P.mul_fast(curve, acc % r, curve.generator))

    with hal.tuning(ipa_srs_tail_n=0):
        ses = pcdl.IpaSession(fe(cs, r), fe([z], r), np.array(log_point(h), dtype=np.uint64), curve.name)
        L.halo_profile_reset()
        L.halo_profile_enable(1)
        Lp, Rp = ses.round_lr()
        cnt, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        hal.check(L.halo_profile_read(b"msm_acc", ctypes.byref(cnt), ctypes.byref(ms)))
        L.halo_profile_enable(0)
        got = list(Lp), list(Rp)
        # finish the opening (returns the session to the pool)
        rounds = n.bit_length() - 1
        xi = None
        for k in range(rounds):
            hsh = hashlib.sha3_256((b"" if xi is None else xi.tobytes()) + Lp.tobytes() + Rp.tobytes())
            xi = fe([int.from_bytes(hsh.digest(), "little") % r or 1], r)[0]
            ses.fold(xi)
            if k + 1 < rounds:
                Lp, Rp = ses.round_lr()
        ses.end()
    assert cnt.value == 1, cnt.value  # L and R together: one k_acc launch
    assert got[0] == log_point(expL)
    assert got[1] == log_point(expR)
