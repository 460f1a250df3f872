"""CPU tests of the argument contract of halo_pcdl_decide_rho, its _dev form and the tuning key "decide_rho_fs"
(include/halo_gpu.h): ABI 111, both symbols, an empty batch is HALO_OK, every argument error is reported with the
call's name before the device is touched, the key round-trips, and in a fresh process without a GPU: the Poseidon
parameters are required (by the two calls always, by the decider's entry points when the key is 1 and rho is NULL),
and once they are installed the calls reach the device lookup and fail with HALO_EDEVICE (no CPU fallback)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE, ENOTPOW2 = 0, 1, 3, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
NAMES = ("halo_pcdl_decide_rho", "halo_pcdl_decide_rho_dev")


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


class Args:
    """Arrays large enough for k = 2, lg n = 4; every scalar is 1."""

    def __init__(self):
        self.xis = np.ones((10, 4), dtype=np.uint64)
        self.U = np.zeros((2, 8), dtype=np.uint64)
        self.out = np.zeros((2, 4), dtype=np.uint64)
        self.ptrs = [H.ptr(self.xis), H.ptr(self.U), None, H.ptr(self.out)]  # xis, U, live, rho_out


def call(L, name, curve, d, k, ptrs):
    return getattr(L, name)(curve, d, k, *ptrs, *((None,) if name.endswith("_dev") else ()))


def einval(rc, name):
    assert rc == EINVAL
    assert name in H.last_error()


def test_abi_version_111_and_symbols(L):
    assert L.halo_abi_version() >= 111
    assert not set(NAMES) & set(H.missing_symbols())
    assert all(n in H.SIGNATURES for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_empty_batch_is_ok_and_touches_nothing(L, name):
    assert call(L, name, H.PALLAS, 15, 0, [None] * 4) == OK
    assert call(L, name, H.VESTA, 10, 0, [None] * 4) == OK  # nothing to check, not even d


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors(L, name):
    einval(call(L, name, 2, 15, 2, Args().ptrs), name)
    einval(call(L, name, -1, 15, 2, Args().ptrs), name)
    assert call(L, name, 2, 15, 0, [None] * 4) == EINVAL  # the curve is checked even for an empty batch
    assert call(L, name, H.PALLAS, 10, 2, Args().ptrs) == ENOTPOW2
    assert "n (11) is not a power of two" in H.last_error()
    einval(call(L, name, H.PALLAS, (1 << 29) - 1, 2, Args().ptrs), name)
    assert "out of range" in H.last_error()
    for hole in (0, 1, 3):  # live may be NULL
        a = Args()
        a.ptrs[hole] = None
        einval(call(L, name, H.PALLAS, 15, 2, a.ptrs), name)
        assert "null pointer" in H.last_error()
    einval(call(L, name, H.PALLAS, 15, 0x7FFFFFFF // 4 + 1, Args().ptrs), name)  # the k bound of the decider
    assert "instances in one call" in H.last_error()


def test_host_form_rejects_an_xi_not_below_the_modulus(L):
    a = Args()
    a.xis[7] = 0xFFFFFFFFFFFFFFFF  # xi_2 of instance 1
    einval(call(L, NAMES[0], H.PALLAS, 15, 2, a.ptrs), NAMES[0])
    assert "xi_2 of instance 1 is not below the modulus" in H.last_error()


def test_tuning_key_round_trips(L):
    assert H.get_tuning("decide_rho_fs") == 0  # the default
    try:
        H.set_tuning("decide_rho_fs", 1)
        assert H.get_tuning("decide_rho_fs") == 1
        H.set_tuning("decide_rho_fs", -1)
        assert H.get_tuning("decide_rho_fs") == 0
        with H.deriving(True):
            assert H.get_tuning("decide_rho_fs") == 1
            with H.deriving(False):
                assert H.get_tuning("decide_rho_fs") == 1  # untouched
        assert H.get_tuning("decide_rho_fs") == 0
    finally:
        H.set_tuning("decide_rho_fs", -1)


def test_fs_rhos_reads_the_argument():
    assert H.fs_rhos(None, 3) == (None, False)
    assert H.fs_rhos("fs", 3) == (None, True)
    got, derive = H.fs_rhos(np.ones((3, 4), dtype=np.uint64), 3)
    assert got.shape == (3, 4) and not derive
    with pytest.raises(ValueError):
        H.fs_rhos("random", 3)


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
L.halo_set_tuning.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
sz = ctypes.c_size_t
def p(a): return a.ctypes.data_as(vp)
xis = np.ones((10, 4), dtype=np.uint64); U = np.zeros((2, 8), dtype=np.uint64); out = np.zeros((2, 4), dtype=np.uint64)
ok = np.zeros(2, dtype=np.uint8)
def err(rc): return [rc, L.halo_last_error().decode()]
def rho(curve, k=2): return err(L.halo_pcdl_decide_rho(curve, sz(15), sz(k), p(xis), p(U), None, p(out)))
def rho_dev(curve, k=2): return err(L.halo_pcdl_decide_rho_dev(curve, sz(15), sz(k), p(xis), p(U), None, p(out), None))
def batch(curve, r=None): return err(L.halo_pcdl_decide_batch(curve, sz(15), sz(2), p(xis), p(U), None, r, p(ok)))
def batch_dev(curve, r=None): return err(L.halo_pcdl_decide_batch_dev(curve, sz(15), sz(2), p(xis), p(U), None, r, p(ok), None, None))
def bisect_dev(curve, r=None): return err(L.halo_pcdl_decide_bisect_dev(curve, sz(15), sz(2), p(xis), p(U), None, r, p(ok), None))
res = {"devices": L.halo_device_count()}
res["unset"] = [rho(0), rho_dev(0)]
res["unset_empty"] = rho(0, 0)[0]
res["key0_unset"] = [batch(0), batch_dev(0), bisect_dev(0)]              # as before the key existed
assert L.halo_set_tuning(b"decide_rho_fs", 1) == 0
res["key1_unset"] = [batch(0), batch_dev(0), bisect_dev(0)]
res["key1_unset_own_rho"] = [batch(0, p(out + 1)), batch_dev(0, p(out)), bisect_dev(0, p(out))]
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = [rho(1), batch(1)]   # Vesta's base field Fp is still unset
res["nogpu"] = [rho(0), rho_dev(0), batch(0), batch_dev(0), bisect_dev(0)]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """In a child with every device hidden.  Before halo_poseidon_set_params: the two calls are HALO_EINVAL naming
    the call and halo_poseidon_set_params (an empty batch is still HALO_OK); the decider's entry points with a NULL
    rho reach the device lookup under the key's default (bisect_dev refuses the NULL rho as ever) and are HALO_EINVAL
    in the same words with the key at 1, while the caller's own rho needs no parameters.  Afterwards everything
    reaches the device lookup and fails with HALO_EDEVICE."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH, GOLDEN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0
    for (rc, msg), name in zip(res["unset"], NAMES):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["unset_empty"] == OK
    deciders = ("halo_pcdl_decide_batch", "halo_pcdl_decide_batch_dev", "halo_pcdl_decide_bisect_dev")
    assert [rc for rc, _ in res["key0_unset"]] == [EDEVICE, EDEVICE, EINVAL]
    assert "null d_rho" in res["key0_unset"][2][1]
    for (rc, msg), name in zip(res["key1_unset"], deciders):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert [rc for rc, _ in res["key1_unset_own_rho"]] == [EDEVICE] * 3
    assert res["set"] == OK
    for (rc, msg), name in zip(res["other_field_unset"], (NAMES[0], deciders[0])):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    for rc, msg in res["nogpu"]:
        assert rc == EDEVICE and "device" in msg.lower(), (rc, msg)
