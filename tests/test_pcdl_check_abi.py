"""CPU tests of the PCDL verifier's entry points' argument contract (include/halo_gpu.h:
halo_point_lincomb_batch, halo_point_lincomb_batch_dev, halo_pcdl_succinct_check_batch): argument errors
are reported with the call's name before the device is touched, an empty batch is HALO_OK, a batch of
no terms is answered on the host, and without a GPU a compute call is HALO_EDEVICE (no CPU fallback)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE, ENOTPOW2 = 0, 1, 3, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(H.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(os.path.dirname(H.LIB_PATH), "..", "csrc")], check=True)
    return H.load()


def einval(rc, name):
    assert rc == EINVAL
    assert name in H.last_error()


def test_abi_version_102(L):
    assert L.halo_abi_version() >= 102


def test_lincomb_null_pointers_and_unknown_curve(L):
    pts = np.zeros((2, 3, 8), dtype=np.uint64)
    sc = np.zeros((2, 3, 4), dtype=np.uint64)
    out = np.zeros((2, 16), dtype=np.uint64)
    p, s, o = H.ptr(pts), H.ptr(sc), H.ptr(out)
    name = "halo_point_lincomb_batch"
    einval(L.halo_point_lincomb_batch(H.PALLAS, None, None, s, 2, 3, o), name)
    einval(L.halo_point_lincomb_batch(H.PALLAS, None, p, None, 2, 3, o), name)
    einval(L.halo_point_lincomb_batch(H.PALLAS, None, p, s, 2, 3, None), name)
    einval(L.halo_point_lincomb_batch(2, None, p, s, 2, 3, o), name)
    name = "halo_point_lincomb_batch_dev"
    einval(L.halo_point_lincomb_batch_dev(H.VESTA, None, None, s, 2, 3, o, None, None), name)
    einval(L.halo_point_lincomb_batch_dev(H.VESTA, None, p, None, 2, 3, o, None, None), name)
    einval(L.halo_point_lincomb_batch_dev(H.VESTA, None, p, s, 2, 3, None, None, None), name)
    einval(L.halo_point_lincomb_batch_dev(-1, None, p, s, 2, 3, o, None, None), name)


def test_lincomb_scalar_not_below_the_modulus(L):
    pts = np.zeros((1, 2, 8), dtype=np.uint64)
    sc = np.zeros((1, 2, 4), dtype=np.uint64)
    sc[0, 1] = 0xFFFFFFFFFFFFFFFF
    out = np.zeros((1, 8), dtype=np.uint64)
    einval(L.halo_point_lincomb_batch(H.PALLAS, None, H.ptr(pts), H.ptr(sc), 1, 2, H.ptr(out)), "halo_point_lincomb_batch")
    assert "scalar 1" in H.last_error()


def _succinct_args(k=2, lg=4):
    pts = np.zeros((k * max(lg, 1), 8), dtype=np.uint64)
    fes = np.ones((k * (lg + 1), 4), dtype=np.uint64)
    ok = np.zeros(k, dtype=np.uint8)
    # C_prime, z, v, xis, Ls, Rs, U, c, ok_out
    return [H.ptr(pts), H.ptr(fes), H.ptr(fes), H.ptr(fes), H.ptr(pts), H.ptr(pts), H.ptr(pts), H.ptr(fes), H.ptr(ok)]


def test_succinct_check_null_pointers_and_unknown_curve(L):
    name = "halo_pcdl_succinct_check_batch"
    for hole in range(9):
        args = _succinct_args()
        args[hole] = None
        einval(L.halo_pcdl_succinct_check_batch(H.PALLAS, 15, 2, *args), name)
    einval(L.halo_pcdl_succinct_check_batch(7, 15, 2, *_succinct_args()), name)


def test_succinct_check_not_a_power_of_two(L):
    assert L.halo_pcdl_succinct_check_batch(H.PALLAS, 10, 2, *_succinct_args()) == ENOTPOW2
    assert "n (11) is not a power of two" in H.last_error()


def test_empty_batch_is_ok_and_touches_nothing(L):
    assert L.halo_point_lincomb_batch(H.PALLAS, None, None, None, 0, 5, None) == OK
    assert L.halo_point_lincomb_batch_dev(H.VESTA, None, None, None, 0, 5, None, None, None) == OK
    assert L.halo_pcdl_succinct_check_batch(H.PALLAS, 15, 0, *([None] * 9)) == OK
    assert L.halo_pcdl_succinct_check_batch(H.PALLAS, 10, 0, *([None] * 9)) == OK  # nothing to check, not even d


def test_no_terms_returns_the_addends_on_the_host(L):
    """t = 0 with k > 0 is HALO_OK without a device: the sums are the addends (the identity without any),
    and an addend that is neither (0, 0) nor on the curve gives (0, 0) as it does on the device."""
    g = np.load(GOLDEN)
    on = np.ascontiguousarray(g["open_pallas_n16_plain_U"][0], dtype=np.uint64)
    off = on.copy()
    off[4] ^= np.uint64(1)
    add = np.stack([on, np.zeros(8, dtype=np.uint64), off])
    out = np.full((3, 8), 7, dtype=np.uint64)
    assert L.halo_point_lincomb_batch(H.PALLAS, H.ptr(add), None, None, 3, 0, H.ptr(out)) == OK
    assert np.array_equal(out[0], on) and not out[1].any() and not out[2].any()
    out[:] = 7
    assert L.halo_point_lincomb_batch(H.PALLAS, None, None, None, 3, 0, H.ptr(out)) == OK
    assert not out.any()
    von = np.ascontiguousarray(g["open_vesta_n16_hiding_U"][0], dtype=np.uint64)
    assert L.halo_point_lincomb_batch(H.VESTA, H.ptr(von), None, None, 1, 0, H.ptr(out)) == OK
    assert np.array_equal(out[0], von)
    assert L.halo_point_lincomb_batch(H.PALLAS, H.ptr(von), None, None, 1, 0, H.ptr(out)) == OK
    assert not out[0].any()  # a Vesta point is not on Pallas


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
vp = ctypes.c_void_p
sz = ctypes.c_size_t
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((8, 8), dtype=np.uint64); fes = np.ones((10, 4), dtype=np.uint64); ok = np.zeros(16, dtype=np.uint64)
res = {"devices": L.halo_device_count()}
res["lincomb"] = [L.halo_point_lincomb_batch(0, None, p(pts), p(fes), sz(2), sz(2), p(ok)), L.halo_last_error().decode()]
res["lincomb_dev"] = [L.halo_point_lincomb_batch_dev(0, None, p(pts), p(fes), sz(2), sz(2), p(ok), None, None),
                      L.halo_last_error().decode()]
res["succinct"] = [L.halo_pcdl_succinct_check_batch(0, sz(15), sz(2), p(pts), p(fes), p(fes), p(fes), p(pts), p(pts), p(pts),
                                                    p(fes), p(ok)), L.halo_last_error().decode()]
res["empty"] = L.halo_pcdl_succinct_check_batch(0, sz(15), sz(0), None, None, None, None, None, None, None, None, None)
print(json.dumps(res))
"""


def test_no_gpu_in_a_fresh_process(L):
    """With every device hidden the three calls reach the device lookup and fail with HALO_EDEVICE; an
    empty batch is still HALO_OK."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0
    for name in ("lincomb", "lincomb_dev", "succinct"):
        rc, msg = res[name]
        assert rc == EDEVICE and "device" in msg.lower(), (name, rc, msg)
    assert res["empty"] == OK
