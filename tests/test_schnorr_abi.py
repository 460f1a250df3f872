"""CPU tests of the Poseidon / Schnorr entry points' argument contract (include/halo_gpu.h): argument
errors are HALO_EINVAL with the call's name in halo_last_error() before the device is touched, an empty
batch is HALO_OK, and without a GPU a compute call is HALO_EDEVICE (no CPU fallback)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE = 0, 1, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")


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


def test_abi_version_101(L):
    assert L.halo_abi_version() >= 101


def test_set_params_argument_errors(L):
    x = np.zeros((165, 4), dtype=np.uint64)
    einval(L.halo_poseidon_set_params(H.FQ, None, H.ptr(x)), "halo_poseidon_set_params")
    einval(L.halo_poseidon_set_params(H.FQ, H.ptr(x), None), "halo_poseidon_set_params")
    einval(L.halo_poseidon_set_params(2, H.ptr(x), H.ptr(x)), "halo_poseidon_set_params")
    big = np.full((165, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # not below the modulus
    einval(L.halo_poseidon_set_params(H.FQ, H.ptr(big), H.ptr(x)), "halo_poseidon_set_params")


def test_null_pointers_and_unknown_ids(L):
    a = np.zeros((4, 8), dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint8)
    p = H.ptr(a)
    for name in ("halo_poseidon_hash_batch", "halo_poseidon_hash_batch_dev"):
        fn = getattr(L, name)
        tail = (None,) if name.endswith("_dev") else ()
        einval(fn(H.FQ, None, 2, 1, p, *tail), name)
        einval(fn(H.FQ, p, 2, 1, None, *tail), name)
        einval(fn(5, p, 2, 1, p, *tail), name)
    for name in ("halo_schnorr_hash_batch", "halo_schnorr_hash_batch_dev"):
        fn = getattr(L, name)
        tail = (None,) if name.endswith("_dev") else ()
        einval(fn(H.PALLAS, None, p, p, 1, 1, p, *tail), name)
        einval(fn(H.PALLAS, p, None, p, 1, 1, p, *tail), name)
        einval(fn(H.PALLAS, p, p, None, 1, 1, p, *tail), name)  # msgs may be NULL only when msg_len = 0
        einval(fn(H.PALLAS, p, p, p, 1, 1, None, *tail), name)
        einval(fn(2, p, p, p, 1, 1, p, *tail), name)
    for name in ("halo_schnorr_verify_batch", "halo_schnorr_verify_batch_dev"):
        fn = getattr(L, name)
        tail = (None,) if name.endswith("_dev") else ()
        o = H.ptr(out)
        einval(fn(H.VESTA, None, p, p, p, 1, 1, o, *tail), name)
        einval(fn(H.VESTA, p, None, p, p, 1, 1, o, *tail), name)
        einval(fn(H.VESTA, p, p, None, p, 1, 1, o, *tail), name)
        einval(fn(H.VESTA, p, p, p, None, 1, 1, o, *tail), name)
        einval(fn(H.VESTA, p, p, p, p, 1, 1, None, *tail), name)
        einval(fn(-1, p, p, p, p, 1, 1, o, *tail), name)


def test_empty_batch_is_ok_and_touches_nothing(L):
    assert L.halo_poseidon_hash_batch(H.FQ, None, 3, 0, None) == OK
    assert L.halo_poseidon_hash_batch_dev(H.FP, None, 3, 0, None, None) == OK
    assert L.halo_schnorr_hash_batch(H.PALLAS, None, None, None, 10, 0, None) == OK
    assert L.halo_schnorr_hash_batch_dev(H.PALLAS, None, None, None, 10, 0, None, None) == OK
    assert L.halo_schnorr_verify_batch(H.VESTA, None, None, None, None, 10, 0, None) == OK
    assert L.halo_schnorr_verify_batch_dev(H.VESTA, None, None, None, None, 10, 0, None, None) == OK


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((2, 8), dtype=np.uint64); fes = np.zeros((2, 4), dtype=np.uint64); ok = np.zeros(2, dtype=np.uint8)
sz = ctypes.c_size_t
res = {}
def verify(curve): return L.halo_schnorr_verify_batch(curve, p(pts), p(pts), p(fes), p(fes), sz(1), sz(2), p(ok))
def phash(field): return L.halo_poseidon_hash_batch(field, p(fes), sz(1), sz(2), p(fes))
def shash(curve): return L.halo_schnorr_hash_batch(curve, p(pts), p(pts), p(fes), sz(1), sz(2), p(fes))
res["unset"] = [[phash(1), L.halo_last_error().decode()], [shash(0), L.halo_last_error().decode()],
                [verify(0), L.halo_last_error().decode()]]
res["unset_empty"] = L.halo_schnorr_verify_batch(0, None, None, None, None, sz(1), sz(0), None)
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = [verify(1), L.halo_last_error().decode()]   # Vesta's base field Fp is still unset
res["devices"] = L.halo_device_count()
res["nogpu"] = [[phash(1), L.halo_last_error().decode()], [shash(0), L.halo_last_error().decode()],
                [verify(0), L.halo_last_error().decode()]]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """The parameters are process-wide state and the device check needs a process that sees no GPU, so
    this runs in a child with every device hidden: before halo_poseidon_set_params the compute calls are
    HALO_EINVAL naming the call (an empty batch is still HALO_OK); afterwards they reach the device
    lookup and fail with HALO_EDEVICE."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH, GOLDEN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    names = ["halo_poseidon_hash_batch", "halo_schnorr_hash_batch", "halo_schnorr_verify_batch"]
    for (rc, msg), name in zip(res["unset"], names):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["unset_empty"] == OK
    assert res["set"] == OK
    assert res["other_field_unset"][0] == EINVAL and "halo_schnorr_verify_batch" in res["other_field_unset"][1]
    assert res["devices"] == 0
    for (rc, msg), name in zip(res["nogpu"], names):
        assert rc == EDEVICE and "device" in msg.lower(), (name, rc, msg)
