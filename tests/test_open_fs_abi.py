"""CPU tests of the argument contract of halo_pcdl_open_fs and halo_pcdl_open_fs_dev_multi
(include/halo_gpu.h): argument errors are reported with the call's name before the device is touched, n must be
a power of two, a hiding opening needs its random draws, an empty multi call is HALO_OK, the Poseidon parameters
of the curve's base field must be installed, and without a GPU a call is HALO_EDEVICE (no CPU fallback)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE, ENOTPOW2, EDEGREE = 0, 1, 3, 4, 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
ONE, MULTI = "halo_pcdl_open_fs", "halo_pcdl_open_fs_dev_multi"


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


def one_args(n=16, hiding=False):
    """p, len, d, z, v, C, w, q, w_bar, Ls, Rs, U, c, C_bar, w_prime, v_out"""
    fes = np.ones((n, 4), dtype=np.uint64)
    pts = np.zeros((8, 8), dtype=np.uint64)
    f, p = H.ptr(fes), H.ptr(pts)
    h = f if hiding else None
    return [f, n, n - 1, f, f, p, h, h, h, p, p, p, f, p if hiding else None, h, None]


def multi_args(k=2, n=16):
    """k, d_p, lens, d, z, C, Ls, Rs, U, c, v_out (d_p never dereferenced before the device lookup)"""
    fes = np.ones((k * n, 4), dtype=np.uint64)
    pts = np.zeros((k * 8, 8), dtype=np.uint64)
    ptrs = (ctypes.c_void_p * k)(*[fes.ctypes.data] * k)
    lens = (ctypes.c_size_t * k)(*[n] * k)
    f, p = H.ptr(fes), H.ptr(pts)
    return [k, ptrs, lens, n - 1, f, p, p, p, p, f, None]


def test_abi_version_107(L):
    assert L.halo_abi_version() >= 107
    assert not [s for s in H.missing_symbols() if "open_fs" in s]


def test_one_null_pointers_and_unknown_curve(L):
    for hole in (0, 3, 5, 9, 10, 11, 12):  # p, z, C, Ls, Rs, U, c
        args = one_args()
        args[hole] = None
        einval(L.halo_pcdl_open_fs(H.PALLAS, *args), ONE)
        assert "null argument" in H.last_error()
    einval(L.halo_pcdl_open_fs(2, *one_args()), ONE)
    einval(L.halo_pcdl_open_fs(-1, *one_args()), ONE)


def test_multi_null_pointers_and_unknown_curve(L):
    for hole in (1, 2, 4, 5, 6, 7, 8, 9):  # d_p, lens, z, C, Ls, Rs, U, c
        args = multi_args()
        args[hole] = None
        einval(L.halo_pcdl_open_fs_dev_multi(H.VESTA, *args), MULTI)
        assert "null argument" in H.last_error()
    args = multi_args()
    args[1] = (ctypes.c_void_p * 2)(args[1][0], None)  # one polynomial missing
    einval(L.halo_pcdl_open_fs_dev_multi(H.VESTA, *args), MULTI)
    assert "polynomial 1" in H.last_error()
    einval(L.halo_pcdl_open_fs_dev_multi(2, *multi_args()), MULTI)


def test_shape_assertions(L):
    """The assertions of halo_pcdl_open_begin: n > 1, n a power of two, p.degree() <= d (trailing zeros do not count)."""
    a, m = one_args(), multi_args()
    a[2], m[3] = 10, 10
    assert L.halo_pcdl_open_fs(H.PALLAS, *a) == ENOTPOW2
    assert "n (11) is not a power of two" in H.last_error()
    assert L.halo_pcdl_open_fs_dev_multi(H.PALLAS, *m) == ENOTPOW2
    assert "n (11) is not a power of two" in H.last_error()
    a, m = one_args(), multi_args()
    a[2], m[3] = 0, 0
    einval(L.halo_pcdl_open_fs(H.PALLAS, *a), "n > 1")
    einval(L.halo_pcdl_open_fs_dev_multi(H.PALLAS, *m), "n > 1")
    a, m = one_args(), multi_args()
    a[2], m[3] = 7, 7
    assert L.halo_pcdl_open_fs(H.PALLAS, *a) == EDEGREE and "p.degree() <= d" in H.last_error()
    assert L.halo_pcdl_open_fs_dev_multi(H.PALLAS, *m) == EDEGREE and "p.degree() <= d" in H.last_error()
    a = one_args()
    fes = np.ones((16, 4), dtype=np.uint64)
    fes[8:] = 0  # degree 7 in 16 coefficients: passes the degree check, so the call goes on to the device lookup
    a[0], a[2] = H.ptr(fes), 7
    assert L.halo_pcdl_open_fs(H.PALLAS, *a) != EDEGREE


def test_hiding_needs_its_draws_and_outputs(L):
    for hole in (7, 8, 13, 14):  # q, w_bar, C_bar, w_prime
        args = one_args(hiding=True)
        args[hole] = None
        einval(L.halo_pcdl_open_fs(H.VESTA, *args), ONE)
        assert "hiding" in H.last_error()


def test_empty_multi_is_ok_and_touches_nothing(L):
    assert L.halo_pcdl_open_fs_dev_multi(H.PALLAS, 0, None, None, 15, None, None, None, None, None, None, None) == OK
    assert L.halo_pcdl_open_fs_dev_multi(H.PALLAS, 0, None, None, 10, None, None, None, None, None, None, None) == OK


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
sz = ctypes.c_size_t
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((8, 8), dtype=np.uint64); fes = np.ones((32, 4), dtype=np.uint64)
ptrs = (vp * 2)(fes.ctypes.data, fes.ctypes.data); lens = (sz * 2)(16, 16)
def one(curve):
    return [L.halo_pcdl_open_fs(curve, p(fes), sz(16), sz(15), p(fes), p(fes), p(pts), None, None, None, p(pts), p(pts),
                                p(pts), p(fes), None, None, None), L.halo_last_error().decode()]
def multi(curve, k=2):
    return [L.halo_pcdl_open_fs_dev_multi(curve, sz(k), ptrs, lens, sz(15), p(fes), p(pts), p(pts), p(pts), p(pts), p(fes),
                                          None), L.halo_last_error().decode()]
res = {"devices": L.halo_device_count()}
res["unset"] = [one(0), multi(0)]
res["unset_empty"] = multi(0, 0)[0]
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = one(1)   # Vesta's base field Fp is still unset
res["nogpu"] = [one(0), multi(0)]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """In a child with every device hidden: before halo_poseidon_set_params both calls are HALO_EINVAL naming
    the call and halo_poseidon_set_params (an empty multi call is still HALO_OK); afterwards they reach the
    device lookup and fail with HALO_EDEVICE."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH, GOLDEN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0
    for (rc, msg), name in zip(res["unset"], (ONE, MULTI)):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["unset_empty"] == OK
    assert res["set"] == OK
    assert res["other_field_unset"][0] == EINVAL and ONE in res["other_field_unset"][1]
    for (rc, msg), name in zip(res["nogpu"], (ONE, MULTI)):
        assert rc == EDEVICE and "device" in msg.lower(), (name, rc, msg)
