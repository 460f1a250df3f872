"""CPU tests of the argument contract of the batched decider's entry points (include/halo_gpu.h:
halo_pcdl_decide_batch, halo_pcdl_check_fs_batch, halo_plonk_verify_batch and their _dev forms): the errors that
come before any device work carry the call's name, an empty batch is HALO_OK, n must be a power of two, a rho
entry that is zero or not below the modulus is HALO_EINVAL, and the tuning key of the group plan round-trips."""
import os
import subprocess

import numpy as np
import pytest

import pasta as P
from halo_amd import _lib as H

OK, EINVAL, ENOTPOW2 = 0, 1, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
FP_MODULUS = P.CURVES["pallas"].scalar


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(H.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(os.path.dirname(H.LIB_PATH), "..", "csrc")], check=True)
    lib = H.load()
    g = np.load(GOLDEN)
    for name, f in (("fp", H.FP), ("fq", H.FQ)):  # host-only call: no GPU needed
        mds, rc = H.fe_array(g[f"poseidon_{name}_mds"], 9), H.fe_array(g[f"poseidon_{name}_rc"], 165)
        assert lib.halo_poseidon_set_params(f, H.ptr(mds), H.ptr(rc)) == OK
    return lib


def limbs(x):
    return [(x >> (64 * i)) & (2**64 - 1) for i in range(4)]


def test_abi_version_105(L):
    assert L.halo_abi_version() >= 105


def test_group_budget_tuning_key(L):
    assert H.get_tuning("decide_group_scalars") == 1 << 25
    with H.tuning(decide_group_scalars=2048):
        assert H.get_tuning("decide_group_scalars") == 2048
    H.set_tuning("decide_group_scalars", 5)
    H.set_tuning("decide_group_scalars", -1)
    assert H.get_tuning("decide_group_scalars") == 1 << 25


def test_empty_batches(L):
    assert L.halo_pcdl_decide_batch(0, 15, 0, None, None, None, None, None) == OK
    assert L.halo_pcdl_decide_batch_dev(0, 15, 0, None, None, None, None, None, None, None) == OK
    assert L.halo_pcdl_check_fs_batch(1, 15, 0, *[None] * 12) == OK
    assert L.halo_pcdl_check_fs_batch_dev(1, 15, 0, *[None] * 14) == OK
    assert L.halo_plonk_verify_batch(0, 8, 0, None, None, 0, *[None] * 21) == OK
    assert L.halo_plonk_verify_batch_dev(0, 8, 0, None, None, 0, *[None] * 23) == OK


def decide_args(k=3, lg=4):
    xis = np.ones((k * (lg + 1), 4), dtype=np.uint64)
    U = np.zeros((k, 8), dtype=np.uint64)
    rho = np.ones((k, 4), dtype=np.uint64)
    ok = np.zeros(k, dtype=np.uint8)
    return xis, U, rho, ok


def test_decide_batch_argument_errors(L):
    xis, U, rho, ok = decide_args()
    for name, tail in (("halo_pcdl_decide_batch", ()), ("halo_pcdl_decide_batch_dev", (None, None))):
        fn = getattr(L, name)
        assert fn(7, 15, 3, H.ptr(xis), H.ptr(U), None, None, H.ptr(ok), *tail) == EINVAL and name in H.last_error()
        assert fn(0, 14, 3, H.ptr(xis), H.ptr(U), None, None, H.ptr(ok), *tail) == ENOTPOW2
        assert H.last_error() == "n (15) is not a power of two"
        for hole in (0, 1, 4):
            args = [H.ptr(xis), H.ptr(U), None, None, H.ptr(ok)]
            args[hole] = None
            assert fn(0, 15, 3, *args, *tail) == EINVAL and "null pointer" in H.last_error()
    zero = rho.copy()
    zero[1] = 0
    assert L.halo_pcdl_decide_batch(0, 15, 3, H.ptr(xis), H.ptr(U), None, H.ptr(zero), H.ptr(ok)) == EINVAL
    assert H.last_error() == "halo_pcdl_decide_batch: rho[1] is zero"
    big = rho.copy()
    big[2] = limbs(FP_MODULUS)
    assert L.halo_pcdl_decide_batch(0, 15, 3, H.ptr(xis), H.ptr(U), None, H.ptr(big), H.ptr(ok)) == EINVAL
    assert H.last_error() == "halo_pcdl_decide_batch: rho[2] is not below the modulus"
    big[2] = limbs(FP_MODULUS - 1)
    bad_xi = xis.copy()
    bad_xi[7] = limbs(FP_MODULUS)
    assert L.halo_pcdl_decide_batch(0, 15, 3, H.ptr(bad_xi), H.ptr(U), None, H.ptr(big), H.ptr(ok)) == EINVAL
    assert H.last_error() == "halo_pcdl_decide_batch: xi_2 of instance 1 is not below the modulus"


def test_check_fs_batch_rho_errors(L):
    k, lg = 2, 4
    pts = np.zeros((k * lg, 8), dtype=np.uint64)
    fes = np.ones((k, 4), dtype=np.uint64)
    ok = np.zeros(k, dtype=np.uint8)
    p, f = H.ptr(pts), H.ptr(fes)
    rho = np.ones((k, 4), dtype=np.uint64)
    rho[0] = 0
    assert L.halo_pcdl_check_fs_batch(0, 15, k, p, f, f, p, p, p, f, None, None, None, H.ptr(rho), H.ptr(ok)) == EINVAL
    assert H.last_error() == "halo_pcdl_check_fs_batch: rho[0] is zero"
    assert L.halo_pcdl_check_fs_batch(0, 15, k, p, f, f, p, p, None, f, None, None, None, None, H.ptr(ok)) == EINVAL
    assert "halo_pcdl_check_fs_batch: null pointer" in H.last_error()
    assert L.halo_pcdl_check_fs_batch(0, 14, k, p, f, f, p, p, p, f, None, None, None, None, H.ptr(ok)) == ENOTPOW2
