"""CPU tests of the argument contract of the signing entry points (include/halo_gpu.h: halo_generator_mul_batch,
halo_schnorr_sign_batch and their _dev forms), in the manner of tests/test_schnorr_abi.py: argument errors are
HALO_EINVAL with the call's name in halo_last_error() before the device is touched, an empty batch is HALO_OK with
all-NULL arguments, a secret that is not below the modulus is refused with its index, and without a GPU a compute
call is HALO_EDEVICE (no CPU fallback)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE = 0, 1, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
MUL = ("halo_generator_mul_batch", "halo_generator_mul_batch_dev")
SIGN = ("halo_schnorr_sign_batch", "halo_schnorr_sign_batch_dev")


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


def einval(rc, *names):
    assert rc == EINVAL
    for n in names:
        assert n in H.last_error(), (n, H.last_error())


def test_abi_version_113_and_the_four_symbols(L):
    assert L.halo_abi_version() >= 113
    for name in MUL + SIGN:
        assert hasattr(L, name) and name in H.SIGNATURES
    header = open(H.HEADER_PATH).read()
    for name in MUL + SIGN:
        assert name + "(" in header
    assert "lib.rs:41-43" in header and "lib.rs:49-66" in header  # each entry cites the reference


def test_null_pointers_and_unknown_curves(L):
    a = np.zeros((4, 8), dtype=np.uint64)
    p = H.ptr(a)
    for name in MUL:
        fn = getattr(L, name)
        tail = (None,) if name.endswith("_dev") else ()
        einval(fn(H.PALLAS, None, 1, p, *tail), name)
        einval(fn(H.PALLAS, p, 1, None, *tail), name)
        einval(fn(2, p, 1, p, *tail), name)
        einval(fn(-1, p, 1, p, *tail), name)
    for name in SIGN:
        fn = getattr(L, name)
        tail = (None,) if name.endswith("_dev") else ()
        for pk in (p, None):  # pk may be NULL: it is never the missing pointer
            einval(fn(H.VESTA, None, pk, p, p, 1, 1, p, p, *tail), name)  # sk
            einval(fn(H.VESTA, p, pk, None, p, 1, 1, p, p, *tail), name)  # nonce
            einval(fn(H.VESTA, p, pk, p, None, 1, 1, p, p, *tail), name)  # msgs may be NULL only when msg_len = 0
            einval(fn(H.VESTA, p, pk, p, p, 1, 1, None, p, *tail), name)  # R_out
            einval(fn(H.VESTA, p, pk, p, p, 1, 1, p, None, *tail), name)  # s_out
            einval(fn(2, p, pk, p, p, 1, 1, p, p, *tail), name)
            einval(fn(-1, p, pk, p, p, 1, 1, p, p, *tail), name)


def test_msg_len_times_k_overflow(L):
    a = np.zeros((4, 8), dtype=np.uint64)
    p = H.ptr(a)
    for name in SIGN:
        tail = (None,) if name.endswith("_dev") else ()
        einval(getattr(L, name)(H.PALLAS, p, None, p, p, 1 << 62, 4, p, p, *tail), name, "overflow")


def test_empty_batch_is_ok_with_all_null_arguments(L):
    assert L.halo_generator_mul_batch(H.PALLAS, None, 0, None) == OK
    assert L.halo_generator_mul_batch_dev(H.VESTA, None, 0, None, None) == OK
    assert L.halo_schnorr_sign_batch(H.PALLAS, None, None, None, None, 10, 0, None, None) == OK
    assert L.halo_schnorr_sign_batch_dev(H.VESTA, None, None, None, None, 10, 0, None, None, None) == OK
    einval(L.halo_generator_mul_batch(7, None, 0, None), "halo_generator_mul_batch")  # ... but not on an unknown curve
    einval(L.halo_schnorr_sign_batch(7, None, None, None, None, 10, 0, None, None), "halo_schnorr_sign_batch")


def test_a_secret_that_is_not_below_the_modulus_is_refused_with_its_index(L):
    k = 5
    ones = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    zero = np.zeros((k, 4), dtype=np.uint64)
    pts = np.zeros((k, 8), dtype=np.uint64)
    msgs = np.zeros((k, 2, 4), dtype=np.uint64)
    for curve in (H.PALLAS, H.VESTA):
        for i in (0, 3, k - 1):
            bad = zero.copy()
            bad[i] = ones
            einval(L.halo_generator_mul_batch(curve, H.ptr(bad), k, H.ptr(pts)), "halo_generator_mul_batch", f"scalars[{i}]")
            einval(L.halo_schnorr_sign_batch(curve, H.ptr(bad), None, H.ptr(zero), H.ptr(msgs), 2, k, H.ptr(pts), H.ptr(zero)),
                   "halo_schnorr_sign_batch", f"sk[{i}]")
            einval(L.halo_schnorr_sign_batch(curve, H.ptr(zero), None, H.ptr(bad), H.ptr(msgs), 2, k, H.ptr(pts), H.ptr(zero)),
                   "halo_schnorr_sign_batch", f"nonce[{i}]")
            einval(L.halo_schnorr_sign_batch(curve, H.ptr(zero), H.ptr(pts), H.ptr(bad), H.ptr(msgs), 2, k, H.ptr(pts),
                                             H.ptr(zero)), "halo_schnorr_sign_batch", f"nonce[{i}]")
    # the modulus itself (its ark limbs are no canonical element) is refused, the modulus - 1 is not a range error
    from halo_amd.schnorr import SCALAR_MODULUS
    for curve in (H.PALLAS, H.VESTA):
        r = SCALAR_MODULUS[curve]
        at = zero.copy()
        at[2] = [(r >> (64 * j)) & (2**64 - 1) for j in range(4)]
        einval(L.halo_generator_mul_batch(curve, H.ptr(at), k, H.ptr(pts)), "halo_generator_mul_batch", "scalars[2]")


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((2, 8), dtype=np.uint64); fes = np.zeros((2, 4), dtype=np.uint64); out = np.zeros((2, 4), dtype=np.uint64)
sz = ctypes.c_size_t
res = {}
def sign(curve, pk): return L.halo_schnorr_sign_batch(curve, p(fes), pk, p(fes), p(fes), sz(1), sz(2), p(pts), p(out))
def mul(curve): return L.halo_generator_mul_batch(curve, p(fes), sz(2), p(pts))
def err(rc): return [rc, L.halo_last_error().decode()]
res["unset"] = [err(sign(0, None)), err(sign(0, p(pts)))]
res["unset_empty"] = L.halo_schnorr_sign_batch(0, None, None, None, None, sz(1), sz(0), None, None)
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["mul_before_params"] = err(mul(1))   # needs no parameters: it reaches the device lookup
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = err(sign(1, None))   # Vesta's base field Fp is still unset
res["devices"] = L.halo_device_count()
res["nogpu"] = [err(sign(0, None)), err(sign(0, p(pts))), err(mul(0))]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """In a child with every device hidden (the parameters are process-wide state): halo_schnorr_sign_batch before
    halo_poseidon_set_params is HALO_EINVAL naming the call (an empty batch is still HALO_OK), afterwards it reaches
    the device lookup and fails with HALO_EDEVICE; halo_generator_mul_batch is HALO_EDEVICE without any parameters."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH, GOLDEN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for rc, msg in res["unset"]:
        assert rc == EINVAL and "halo_schnorr_sign_batch" in msg and "halo_poseidon_set_params" in msg
    assert res["unset_empty"] == OK
    assert res["mul_before_params"][0] == EDEVICE and "device" in res["mul_before_params"][1].lower()
    assert res["set"] == OK
    assert res["other_field_unset"][0] == EINVAL and "halo_schnorr_sign_batch" in res["other_field_unset"][1]
    assert res["devices"] == 0
    for rc, msg in res["nogpu"]:
        assert rc == EDEVICE and "device" in msg.lower(), (rc, msg)
