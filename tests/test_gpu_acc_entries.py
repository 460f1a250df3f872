"""GPU parity of k_acc reading the sorted keys and values four entries per load (acc_entries.hpp: one
16-byte group per array at a chunk's start and at every multiple of four after it).

What can go wrong is in the chunk geometry: the chunk length K decides at which residues mod 4 chunks
start (K = 1, 2, 3, 5, 6, 9: every residue, reloads in some lanes only; K = 16: every chunk starts a
group, reloads uniform over the wave), and the device count decides where inside a group the last chunk
ends.  So every case asserts the K it is about, from msm_plan.hpp through tests/msm_plan_dump.cpp (read
only, as tests/test_msm_plan.py builds it) at the device's CU count; the K below are those of 256 CUs.

Every MSM goes through the asynchronous entry over the resident window-shifted SRS (the bucket pipeline
at every length) with its k_acc launch counted, as in tests/test_gpu_msm_acc_tail.py, and is checked
against (sum_j s_j k_j) G with the known discrete logs k_j of the synthetic SRS.
"""
import ctypes
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import pasta as P
from halo_amd import group, pcdl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = P.PALLAS
R = C.scalar
SEED = 31
INV_MONT = pow(1 << 256, -1, R)


def fe(vals, m=R):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def rand_mont(n, seed):
    """n random scalars as their Montgomery words (any 254-bit value below r is one): (words, the integers S_j
    with s_j = S_j / 2^256)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    a = np.ascontiguousarray(a)
    b = a.tobytes()
    return a, [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(n)]


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


def srs_msm(hal, sc):
    """sum_j sc_j G_j over the resident SRS prefix by the asynchronous entry: one k_acc launch, checked."""
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


_LOGS = []


def logs(n):
    """Discrete logs of the synthetic SRS's first n points (point j's depends on the seed and j alone, so
    one growing list serves every SRS length)."""
    while len(_LOGS) < n:
        _LOGS.append(group.synth_scalar(SEED, len(_LOGS)) % R)
    return _LOGS[:n]


def log_point(acc):
    return P.point_to_wrapped(C, P.mul_fast(C, acc % R, C.generator))


@pytest.fixture(scope="module")
def chunk_len(tmp_path_factory, hal):
    """(SRS length N, MSM length n) -> k_acc's chunk length for the MSM over the window-shifted SRS
    (msm_device_t: c from the SRS, one bucket set, E = W n) on this device's CUs."""
    import torch
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "msm_plan_dump.cpp"), "-o", exe], check=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def ask(line):
        out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True)
        return json.loads(out.stdout)

    def K(N, n):
        c = ask("bits %d" % N)["shifted_window_bits"]
        W = ask("windows %d" % c)["windows"]
        B = 1 << (c - 1)
        return ask("plan %d %d 1 %d %d %d %d %d" % (W * n, B, B, c, cus, W, W * n))["K"]

    return K


# SRS length -> ((n, K), ...): K as msm_chunk_len gives it on 256 CUs
DENSE = {
    1 << 12: ((1, 1), (2, 1), (3, 1), (17, 1), (512, 1), (2048, 2), (4096, 3)),  # E = 17 n: odd at n = 17
    1 << 16: ((1 << 14, 5), (1 << 15, 6), (1 << 16, 9)),  # chunk starts at every residue mod 4
    1 << 18: ((1 << 18, 16),),  # the headline's path: every chunk starts a group
}


@pytest.mark.parametrize("lgN", [12, 16, 18])
def test_dense_random_scalars(hal, chunk_len, lgN):
    N = 1 << lgN
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)
    ks = logs(N)
    for n, K in DENSE[N]:
        assert chunk_len(N, n) == K, (N, n)
        sc, S = rand_mont(n, 100 + n)
        exp = sum(a * k for a, k in zip(S, ks)) * INV_MONT
        assert srs_msm(hal, sc) == log_point(exp), (N, n)


def test_counts_that_cut_the_last_group(hal, chunk_len):
    """n = 4096 scalars over the 2^12 SRS (K = 3) of which exactly m are non-zero, each below 2^14: one
    non-zero digit (window 0 of c = 15, no carry), so the device count is m and the last chunk ends inside a
    group at every residue: m = 1 .. 9, then 4 K - 1 .. 4 K + 2."""
    N = n = 1 << 12
    K = 3
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=True)
    assert chunk_len(N, n) == K
    ks = logs(N)
    rng = random.Random(6)
    for m in list(range(1, 10)) + [4 * K - 1, 4 * K, 4 * K + 1, 4 * K + 2]:
        idx = rng.sample(range(n), m)
        vals = [rng.randrange(1, 1 << 14) for _ in range(m)]
        sc = np.zeros((n, 4), dtype=np.uint64)
        sc[idx] = fe(vals)
        assert srs_msm(hal, sc) == log_point(sum(v * ks[j] for v, j in zip(vals, idx))), m


def test_pair_msm_round(hal):
    """One pair MSM (L and R of an opening's first round, keys (side, bucket), the R side's points at
    poly_off: the cursor under key_lg / poly_off) at length 2^12, the session pinned to the weighted rounds
    (ipa_srs_tail_n = 0) as tests/test_gpu_msm_acc_tail.py pins it."""
    n = 1 << 12
    m = n // 2
    group.PublicParams.synthesize("pallas", n, SEED, precompute_windows=True)
    ks = logs(n)
    rng = random.Random(7)
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


def test_variable_base_glv(hal):
    """The variable-base path at n = 2^10: GLV entries (phi points past glv_n), one sort window per scalar
    window."""
    n = 1 << 10
    group.PublicParams.synthesize("pallas", n, SEED, precompute_windows=False)
    g = group.PublicParams.read("pallas", 0, n)
    ks = logs(n)
    rng = random.Random(8)
    s = [rng.randrange(R) for _ in range(n)]
    with acc_launches(hal) as prof:
        got = list(group.point_dot_affine(fe(s), g, "pallas"))
    assert prof.count == 1, prof.count
    assert got == log_point(sum(a * k for a, k in zip(s, ks)))
