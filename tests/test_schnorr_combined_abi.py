"""CPU tests of the argument contract of the combined Schnorr batch (include/halo_gpu.h: halo_schnorr_batch_rho,
halo_schnorr_verify_combined and their _dev forms): argument errors are HALO_EINVAL with the call's name in
halo_last_error() before the device is touched, an empty batch is HALO_OK, and without a GPU a compute call is
HALO_EDEVICE (no CPU fallback)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from halo_amd import _lib as H

OK, EINVAL, EDEVICE = 0, 1, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")
RHO_NAMES = ("halo_schnorr_batch_rho", "halo_schnorr_batch_rho_dev")
VERIFY_NAMES = ("halo_schnorr_verify_combined", "halo_schnorr_verify_combined_dev")
FP_MODULUS = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001  # Pallas's scalar field


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


def call(L, name, curve, ptrs, msg_len, k, rest):
    """ptrs: pk, R, s, msgs; rest: rho_out, or rho, ok, combined."""
    tail = (None,) if name.endswith("_dev") else ()
    return getattr(L, name)(curve, *ptrs, msg_len, k, *rest, *tail)


def test_abi_version_112_and_symbols(L):
    assert L.halo_abi_version() >= 112
    assert not set(RHO_NAMES + VERIFY_NAMES) & set(H.missing_symbols())
    assert all(n in H.SIGNATURES for n in RHO_NAMES + VERIFY_NAMES)


def test_null_pointers_and_unknown_curve(L):
    a = np.zeros((4, 8), dtype=np.uint64)
    one = np.ones((4, 4), dtype=np.uint64)
    p, r = H.ptr(a), H.ptr(one)
    for name in RHO_NAMES + VERIFY_NAMES:
        rest = (p,) if name in RHO_NAMES else (r, p, None)  # the combined byte may be NULL
        for hole in range(4):  # pk, R, s; msgs may be NULL only when msg_len = 0
            ptrs = [p, p, p, p]
            ptrs[hole] = None
            einval(call(L, name, H.VESTA, ptrs, 1, 1, rest), name)
            assert "null pointer" in H.last_error()
        out_hole = (None,) if name in RHO_NAMES else (r, None, None)
        einval(call(L, name, H.VESTA, [p, p, p, p], 1, 1, out_hole), name)
        einval(call(L, name, 2, [p, p, p, p], 1, 1, rest), name)
        einval(call(L, name, -1, [p, p, p, p], 1, 1, rest), name)
        einval(call(L, name, H.PALLAS, [p, p, p, p], 1, 119304647, rest), name)  # 2 k + 1 beyond the largest MSM
        assert "signatures in one call" in H.last_error()


def test_empty_batch_is_ok_and_touches_nothing(L):
    for name in RHO_NAMES:
        assert call(L, name, H.PALLAS, [None] * 4, 10, 0, (None,)) == OK
    for name in VERIFY_NAMES:
        assert call(L, name, H.VESTA, [None] * 4, 10, 0, (None, None, None)) == OK


def test_host_form_rejects_a_bad_rho_before_the_device_lookup(L):
    """A zero weight would leave its item unchecked; one not below the modulus is no scalar.  Both are refused with
    the entry named, whether or not a device exists (the child below has none and sees the same error)."""
    a = np.zeros((2, 8), dtype=np.uint64)
    ok = np.zeros(2, dtype=np.uint8)
    p = H.ptr(a)
    rho = np.ones((2, 4), dtype=np.uint64)
    rho[1] = 0
    name = VERIFY_NAMES[0]
    einval(call(L, name, H.PALLAS, [p, p, p, p], 1, 2, (H.ptr(rho), H.ptr(ok), None)), name)
    assert "rho[1] is zero" in H.last_error()
    rho[1] = [(FP_MODULUS >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]  # the modulus itself
    einval(call(L, name, H.PALLAS, [p, p, p, p], 1, 2, (H.ptr(rho), H.ptr(ok), None)), name)
    assert "rho[1] is not below the modulus" in H.last_error()


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
g = np.load(sys.argv[2])
vp = ctypes.c_void_p
sz = ctypes.c_size_t
def p(a): return a.ctypes.data_as(vp)
pts = np.zeros((2, 8), dtype=np.uint64); fes = np.ones((2, 4), dtype=np.uint64); ok = np.zeros(2, dtype=np.uint8)
zero = np.zeros((2, 4), dtype=np.uint64)
def err(rc): return [rc, L.halo_last_error().decode()]
def rho(curve, k=2): return err(L.halo_schnorr_batch_rho(curve, p(pts), p(pts), p(fes), p(fes), sz(1), sz(k), p(fes)))
def rho_dev(curve): return err(L.halo_schnorr_batch_rho_dev(curve, p(pts), p(pts), p(fes), p(fes), sz(1), sz(2), p(fes), None))
def comb(curve, r=None): return err(L.halo_schnorr_verify_combined(curve, p(pts), p(pts), p(fes), p(fes), sz(1), sz(2), r, p(ok), None))
def comb_dev(curve, r=None): return err(L.halo_schnorr_verify_combined_dev(curve, p(pts), p(pts), p(fes), p(fes), sz(1), sz(2), r, p(ok), None, None))
res = {"devices": L.halo_device_count()}
res["unset"] = [rho(0), rho_dev(0), comb(0), comb_dev(0)]
res["unset_empty"] = rho(0, 0)[0]
mds = np.ascontiguousarray(g["poseidon_fq_mds"], dtype=np.uint64); rc = np.ascontiguousarray(g["poseidon_fq_rc"], dtype=np.uint64)
res["set"] = L.halo_poseidon_set_params(1, p(mds), p(rc))
res["other_field_unset"] = [rho(1), comb(1)]   # Vesta's base field Fp is still unset
res["bad_rho"] = comb(0, p(zero))
res["nogpu"] = [rho(0), rho_dev(0), comb(0), comb_dev(0), comb(0, p(fes)), comb_dev(0, p(fes))]
print(json.dumps(res))
"""


def test_unset_parameters_and_no_gpu_in_a_fresh_process(L):
    """In a child with every device hidden.  Before halo_poseidon_set_params the four calls are HALO_EINVAL naming the
    call and halo_poseidon_set_params (an empty batch is still HALO_OK); afterwards a zero rho is still refused first,
    and everything else reaches the device lookup and fails with HALO_EDEVICE."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH, GOLDEN], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["devices"] == 0
    for (rc, msg), name in zip(res["unset"], RHO_NAMES + VERIFY_NAMES):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["unset_empty"] == OK
    assert res["set"] == OK
    for (rc, msg), name in zip(res["other_field_unset"], (RHO_NAMES[0], VERIFY_NAMES[0])):
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["bad_rho"][0] == EINVAL and "rho[0] is zero" in res["bad_rho"][1]
    for rc, msg in res["nogpu"]:
        assert rc == EDEVICE and "device" in msg.lower(), (rc, msg)
