"""CPU tests of the argument contract of halo_acc_verifier_batch, its _dev form and halo_acc_prover
(include/halo_gpu.h): argument errors are reported with the call's name before the device is touched, an empty
batch is HALO_OK, n must be a power of two (and > 1 for the prover), the Poseidon parameters of the curve's base
field must be installed, and without a GPU a call is HALO_EDEVICE (no CPU fallback)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE, ENOTPOW2 = 0, 1, 3, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
VERIFIER = ("halo_acc_verifier_batch", "halo_acc_verifier_batch_dev")
PROVER = "halo_acc_prover"
NAMES = VERIFIER + (PROVER,)
# instance slots: C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime
INSTANCE_REQUIRED = (0, 1, 2, 3, 4, 5, 6)


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


class Args:
    """Arrays large enough for k = 2, m = 2, lg n = 4; every scalar is 1."""

    def __init__(self, hiding=False):
        self.pts = np.zeros((16, 8), dtype=np.uint64)
        self.fes = np.ones((16, 4), dtype=np.uint64)
        self.hid = np.ones(4, dtype=np.uint8)
        self.verdict, self.first_bad = np.zeros(2, dtype=np.uint8), np.zeros(2, dtype=np.uint32)
        p, f = H.ptr(self.pts), H.ptr(self.fes)
        self.instances = [p, f, f, p, p, p, f, H.ptr(self.hid) if hiding else None, p if hiding else None, f if hiding else None]
        self.acc = [p, f, f]                                           # acc_C, acc_z, acc_v
        self.outs = [H.ptr(self.verdict), H.ptr(self.first_bad), f, p, f]  # verdict, first_bad, asdl_out, C_bar_out, v_out
        self.prover_outs = [p, f, f, p, p, p, f, H.ptr(self.verdict), H.ptr(self.first_bad)]


def call(L, name, curve, d, k, m, a):
    if name == PROVER:
        return L.halo_acc_prover(curve, d, m, *a.instances, *a.prover_outs)
    return getattr(L, name)(curve, d, k, m, *a.instances, *a.acc, *a.outs, *((None,) if name.endswith("_dev") else ()))


def test_abi_version_108(L):
    assert L.halo_abi_version() >= 108


@pytest.mark.parametrize("name", NAMES)
def test_no_instances_given(L, name):
    einval(call(L, name, H.PALLAS, 15, 2, 0, Args()), name)
    assert "No instances given" in H.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers_and_unknown_curve(L, name):
    for hole in INSTANCE_REQUIRED:
        a = Args()
        a.instances[hole] = None
        einval(call(L, name, H.PALLAS, 15, 2, 2, a), name)
        assert "null pointer" in H.last_error()
    einval(call(L, name, 2, 15, 2, 2, Args()), name)
    einval(call(L, name, -1, 15, 2, 2, Args()), name)


@pytest.mark.parametrize("name", VERIFIER)
def test_verifier_outputs(L, name):
    a = Args()
    a.outs[0] = None  # verdict
    einval(call(L, name, H.PALLAS, 15, 2, 2, a), name)
    assert "null pointer" in H.last_error()
    for hole in (2, 3, 4):  # without an accumulator asdl_out, C_bar_out and v_out are the result
        a = Args()
        a.acc = [None, None, None]
        a.outs[hole] = None
        einval(call(L, name, H.PALLAS, 15, 2, 2, a), name)
        assert "null pointer" in H.last_error()


def test_prover_outputs(L):
    for hole in range(8):  # acc_C .. acc_c and verdict; first_bad is optional
        a = Args()
        a.prover_outs[hole] = None
        einval(call(L, PROVER, H.PALLAS, 15, 1, 2, a), PROVER)
        assert "null pointer" in H.last_error()


@pytest.mark.parametrize("name", VERIFIER)
def test_accumulator_only_partly_given(L, name):
    for keep in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
        a = Args()
        a.acc = [x if j in keep else None for j, x in enumerate(a.acc)]
        einval(call(L, name, H.VESTA, 15, 2, 2, a), name)
        assert "together" in H.last_error()


@pytest.mark.parametrize("name", NAMES)
def test_hiding_needs_c_bar_and_w_prime(L, name):
    for hole in (8, 9):
        a = Args(hiding=True)
        a.instances[hole] = None
        einval(call(L, name, H.VESTA, 15, 2, 2, a), name)
        assert "hiding" in H.last_error()


@pytest.mark.parametrize("name", VERIFIER)
def test_empty_batch_is_ok_and_touches_nothing(L, name):
    a = Args()
    a.instances, a.acc, a.outs = [None] * 10, [None] * 3, [None] * 5
    assert call(L, name, H.PALLAS, 15, 0, 2, a) == OK
    assert call(L, name, H.PALLAS, 10, 0, 0, a) == OK  # nothing to check, not even d or m


@pytest.mark.parametrize("name", NAMES)
def test_not_a_power_of_two(L, name):
    assert call(L, name, H.PALLAS, 10, 2, 2, Args()) == ENOTPOW2
    assert "n (11) is not a power of two" in H.last_error()


def test_prover_needs_a_round(L):
    einval(call(L, PROVER, H.PALLAS, 0, 1, 2, Args()), PROVER)
    assert "assertion failed: n > 1" in H.last_error()


@pytest.mark.parametrize("name", (VERIFIER[0], PROVER))
def test_host_forms_reject_a_scalar_not_below_the_modulus(L, name):
    big = np.ones((16, 4), dtype=np.uint64)
    big[1] = 0xFFFFFFFFFFFFFFFF
    for slot in (1, 2, 6, 9):  # z, v, c, a read w'
        a = Args(hiding=True)
        a.instances[slot] = H.ptr(big)
        einval(call(L, name, H.PALLAS, 15, 2, 2, a), name)
        assert "instance 1" in H.last_error() and "not below the modulus" in H.last_error()
    if name == PROVER:
        return
    for slot in (1, 2):  # acc_z, acc_v
        a = Args()
        a.acc[slot] = H.ptr(big)
        einval(call(L, name, H.PALLAS, 15, 2, 2, a), name)
        assert "accumulator 1" in H.last_error() and "not below the modulus" in H.last_error()


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
sz = ctypes.c_size_t
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((16, 8), dtype=np.uint64); fes = np.ones((16, 4), dtype=np.uint64)
verdict = np.zeros(2, dtype=np.uint8); fb = np.zeros(2, dtype=np.uint32)
inst = [p(pts), p(fes), p(fes), p(pts), p(pts), p(pts), p(fes), None, None, None]
def host(curve, k=2):
    return [L.halo_acc_verifier_batch(curve, sz(15), sz(k), sz(2), *inst, p(pts), p(fes), p(fes), p(verdict), p(fb), None, None,
                                      None), L.halo_last_error().decode()]
def dev(curve, k=2):
    return [L.halo_acc_verifier_batch_dev(curve, sz(15), sz(k), sz(2), *inst, p(pts), p(fes), p(fes), p(verdict), p(fb), None,
                                          None, None, None), L.halo_last_error().decode()]
def prover(curve):
    return [L.halo_acc_prover(curve, sz(15), sz(2), *inst, p(pts), p(fes), p(fes), p(pts), p(pts), p(pts), p(fes), p(verdict),
                              p(fb)), L.halo_last_error().decode()]
res = {"devices": L.halo_device_count()}
res["unset"] = [host(0), dev(0), prover(0)]
res["unset_empty"] = host(0, 0)[0]
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = host(1)   # Vesta's base field Fp is still unset
res["nogpu"] = [host(0), dev(0), prover(0)]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """In a child with every device hidden: before halo_poseidon_set_params the calls are HALO_EINVAL naming the
    call and halo_poseidon_set_params (an empty batch is still HALO_OK); afterwards they reach the device lookup
    and fail with HALO_EDEVICE."""
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
