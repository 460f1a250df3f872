"""CPU tests of the argument contract of halo_pcdl_succinct_check_fs_batch and its _dev form
(include/halo_gpu.h): argument errors are reported with the call's name before the device is touched, an
empty batch is HALO_OK, n must be a power of two, the Poseidon parameters of the curve's base field must
be installed, and without a GPU a call is HALO_EDEVICE (no CPU fallback)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE, ENOTPOW2 = 0, 1, 3, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
NAMES = ("halo_pcdl_succinct_check_fs_batch", "halo_pcdl_succinct_check_fs_batch_dev")
REQUIRED = (0, 1, 2, 3, 4, 5, 6, 12)  # C, z, v, Ls, Rs, U, c, ok_out


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


def einval(rc, name):
    assert rc == EINVAL
    assert name in H.last_error()


def fs_args(k=2, lg=4, hiding=False):
    """C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, xis_out, alpha_out, ok_out"""
    pts = np.zeros((k * max(lg, 1), 8), dtype=np.uint64)
    fes = np.ones((k * (lg + 1), 4), dtype=np.uint64)
    ok = np.zeros(k, dtype=np.uint8)
    hid = np.ones(k, dtype=np.uint8)
    p, f = H.ptr(pts), H.ptr(fes)
    return [p, f, f, p, p, p, f, H.ptr(hid) if hiding else None, p if hiding else None, f if hiding else None, None, None,
            H.ptr(ok)]


def call(L, name, curve, d, k, args):
    return getattr(L, name)(curve, d, k, *args, *((None,) if name.endswith("_dev") else ()))


def test_abi_version_103(L):
    assert L.halo_abi_version() >= 103


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers_and_unknown_curve(L, name):
    for hole in REQUIRED:
        args = fs_args()
        args[hole] = None
        einval(call(L, name, H.PALLAS, 15, 2, args), name)
        assert "null pointer" in H.last_error()
    einval(call(L, name, 2, 15, 2, fs_args()), name)
    einval(call(L, name, -1, 15, 2, fs_args()), name)


@pytest.mark.parametrize("name", NAMES)
def test_hiding_needs_c_bar_and_w_prime(L, name):
    for hole in (8, 9):
        args = fs_args(hiding=True)
        args[hole] = None
        einval(call(L, name, H.VESTA, 15, 2, args), name)
        assert "hiding" in H.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_is_ok_and_touches_nothing(L, name):
    assert call(L, name, H.PALLAS, 15, 0, [None] * 13) == OK
    assert call(L, name, H.PALLAS, 10, 0, [None] * 13) == OK  # nothing to check, not even d


@pytest.mark.parametrize("name", NAMES)
def test_not_a_power_of_two(L, name):
    assert call(L, name, H.PALLAS, 10, 2, fs_args()) == ENOTPOW2
    assert "n (11) is not a power of two" in H.last_error()


def test_host_form_rejects_a_scalar_not_below_the_modulus(L):
    name = NAMES[0]
    for slot in (1, 2, 6, 9):  # z, v, c, a read w'
        args = fs_args(hiding=True)
        big = np.ones((10, 4), dtype=np.uint64)
        big[1] = 0xFFFFFFFFFFFFFFFF
        args[slot] = H.ptr(big)
        einval(call(L, name, H.PALLAS, 15, 2, args), name)
        assert "instance 1" in H.last_error()


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
sz = ctypes.c_size_t
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((8, 8), dtype=np.uint64); fes = np.ones((10, 4), dtype=np.uint64); ok = np.zeros(2, dtype=np.uint8)
def host(curve, k=2):
    return [L.halo_pcdl_succinct_check_fs_batch(curve, sz(15), sz(k), p(pts), p(fes), p(fes), p(pts), p(pts), p(pts), p(fes),
                                                None, None, None, None, None, p(ok)), L.halo_last_error().decode()]
def dev(curve, k=2):
    return [L.halo_pcdl_succinct_check_fs_batch_dev(curve, sz(15), sz(k), p(pts), p(fes), p(fes), p(pts), p(pts), p(pts),
                                                    p(fes), None, None, None, None, None, p(ok), None),
            L.halo_last_error().decode()]
res = {"devices": L.halo_device_count()}
res["unset"] = [host(0), dev(0)]
res["unset_empty"] = host(0, 0)[0]
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = host(1)   # Vesta's base field Fp is still unset
res["nogpu"] = [host(0), dev(0)]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """In a child with every device hidden: before halo_poseidon_set_params both calls are HALO_EINVAL naming
    the call and halo_poseidon_set_params (an empty batch is still HALO_OK); afterwards they reach the device
    lookup and fail with HALO_EDEVICE."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH, GOLDEN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0
    for (rc, msg), name in zip(res["unset"], NAMES):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["unset_empty"] == OK
    assert res["set"] == OK
    assert res["other_field_unset"][0] == EINVAL and NAMES[0] in res["other_field_unset"][1]
    for (rc, msg), name in zip(res["nogpu"], NAMES):
        assert rc == EDEVICE and "device" in msg.lower(), (name, rc, msg)
