"""CPU tests of the Plonk verifier's restatement (tests/plonk_ref.py), of naive_prover's transcript mode on the
CPU backend and of the argument contract of halo_plonk_verify_succinct_batch (include/halo_gpu.h):

  * the restatement accepts the committed chains of tests/golden/plonk_proofs.npz and reproduces the stored
    challenges; it names the right failure for every tampering tests/test_gpu_plonk_verify.py applies;
  * naive_prover on the CPU backend at n = 8 under the reference's transcripts reproduces the committed Pallas
    chain bit for bit;
  * the new symbols are in the header and the binding; argument errors come before the device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import pasta as P
import plonk_ref as R
from halo_amd import _lib as H

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "plonk_proofs.npz"))
T = np.load(os.path.join(HERE, "golden", "transcript.npz"))
NAMES = ("halo_plonk_verify_succinct_batch", "halo_plonk_verify_succinct_batch_dev")
OK, EINVAL, ENOTPOW2 = 0, 1, 4


@pytest.mark.parametrize("key", sorted(R.CHAINS))
def test_restatement_accepts_the_fixtures(golden, corc, key):
    cname, rows = R.CHAINS[key]
    m = P.CURVES[cname].scalar
    C_qs, recs = R.load_chain(G, key)
    Hh = golden[f"ref_sh_{cname}"][1]
    srs = np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"])
    assert np.array_equal(recs[1].prev, recs[0].next)  # a chain
    for step, rec in enumerate(recs):
        code, rb = R.verify_succinct(cname, rows, C_qs, Hh, rec)
        assert code == R.ACCEPT
        for name in ("challenges", "sides", "asdl"):
            assert np.array_equal(np.stack([R.fe(x, m) for x in rb[name]]), G[f"{key}_{step}_{name}"]), (step, name)
        assert rb["sides"][0] == rb["sides"][1]
        assert R.verify(cname, rows, C_qs, Hh, rec, srs) == (R.ACCEPT, "")
        assert any(not w.any() for w in rec.C_ts)  # the transcript absorbs (0, 0) points


@pytest.mark.parametrize("kind", sorted(R.TAMPERINGS))
@pytest.mark.parametrize("key", ["pallas_n8", "vesta_n16"])
def test_restatement_names_the_failure(golden, corc, key, kind):
    cname, rows = R.CHAINS[key]
    C_qs, recs = R.load_chain(G, key)
    Hh = golden[f"ref_sh_{cname}"][1]
    bad = R.tamper(recs[1], kind, P.CURVES[cname].scalar)
    code, rb = R.verify_succinct(cname, rows, C_qs, Hh, bad)
    assert code == R.TAMPERINGS[kind]
    if kind in ("ws0", "rs3", "ids1", "pub0"):  # the transcript does not read them
        assert np.array_equal(np.stack([R.fe(x, P.CURVES[cname].scalar) for x in rb["challenges"]]),
                              G[f"{key}_1_challenges"])
        assert rb["sides"][0] != rb["sides"][1]
    if kind == "next_pi_c":
        srs = np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"])
        assert R.verify(cname, rows, C_qs, Hh, bad, srs) == (R.ACCEPT, "succinct")


def test_restatement_swapped_selector_commitment(golden):
    C_qs, recs = R.load_chain(G, "pallas_n8")
    C_bad = C_qs.copy()
    C_bad[0], C_bad[1] = C_qs[1], C_qs[0]
    assert R.verify_succinct("pallas", 8, C_bad, golden["ref_sh_pallas"][1], recs[0])[0] == R.INSTANCE_1


def test_cpu_prover_reproduces_the_pallas_fixture(golden, corc):
    cname, n = "pallas", 8
    S, Hh = golden[f"ref_sh_{cname}"]
    C_qs, recs = R.prove_chain(cname, n, np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"]), S, Hh, steps=2, seed=n)
    want_qs, want = R.load_chain(G, "pallas_n8")
    assert np.array_equal(C_qs, want_qs)
    for got, exp in zip(recs, want):
        for f in R.Rec._fields:
            if f == "next_pi":
                assert all(np.array_equal(a, b) for a, b in zip(got.next_pi, exp.next_pi))
            else:
                assert np.array_equal(getattr(got, f), getattr(exp, f)), f


def test_stand_in_path_is_the_default():
    """transcript=None leaves naive_prover on the seeded stand-in; the transcript mode needs an accumulator."""
    import inspect

    from halo_amd import prover
    assert inspect.signature(prover.naive_prover).parameters["transcript"].default is None
    with pytest.raises(ValueError, match="acc_prev"):
        prover.naive_prover(None, {}, 8, None, transcript=R.new_transcript("pallas"))


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(H.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(os.path.dirname(H.LIB_PATH), "..", "csrc")], check=True)
    lib = H.load()
    for name, f in (("fp", H.FP), ("fq", H.FQ)):  # host-only call: no GPU needed
        mds, rc = H.fe_array(T[f"poseidon_{name}_mds"], 9), H.fe_array(T[f"poseidon_{name}_rc"], 165)
        assert lib.halo_poseidon_set_params(f, H.ptr(mds), H.ptr(rc)) == OK
    return lib


def test_symbols_declared_bound_and_exported(L):
    text = re.sub(r"/\*.*?\*/", "", open(H.HEADER_PATH).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text)
        assert name in H.SIGNATURES and hasattr(L, name)
    assert len(H.SIGNATURES[NAMES[0]]) == 25 and len(H.SIGNATURES[NAMES[1]]) == 26
    assert "HALO_PLONK_MALFORMED = 8" in text and "#define HALO_PLONK_EVALS 78" in text
    assert L.halo_abi_version() >= 104


def plonk_args(k=2, lg=3, npi=2):
    """C_qs, public_inputs, npi, then the 19 pointers of the host form."""
    pts = np.zeros((k * 16 * max(lg, 1), 8), dtype=np.uint64)
    fes = np.ones((k * 78, 4), dtype=np.uint64)
    out = np.zeros((k * 5, 4), dtype=np.uint64)
    p, f = H.ptr(pts), H.ptr(fes)
    #       C_qs pub npi  C_ws C_z C_ts vs Ls Rs U  c  prev     next     mds verdict
    return [p, f, npi, p, p, p, f, p, p, p, f, p, f, f, p, f, f, f, H.ptr(out), None, None, None]


def call(L, name, curve, rows, k, args):
    return getattr(L, name)(curve, rows, k, *args, *((None,) if name.endswith("_dev") else ()))


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_come_before_the_device(L, name):
    required = [i for i in range(19) if i != 2]
    for hole in required:
        args = plonk_args()
        args[hole] = None
        assert call(L, name, H.PALLAS, 8, 2, args) == EINVAL
        assert name in H.last_error() and "null pointer" in H.last_error()
    args = plonk_args(npi=0)
    args[1] = None  # no public inputs: the pointer is not read
    assert call(L, name, H.PALLAS, 8, 2, args) != EINVAL or "null pointer" not in H.last_error()
    assert call(L, name, 2, 8, 2, plonk_args()) == EINVAL and "unknown curve" in H.last_error()
    assert call(L, name, H.VESTA, 12, 2, plonk_args()) == ENOTPOW2
    assert "n (12) is not a power of two" in H.last_error()
    assert call(L, name, H.VESTA, 2, 2, plonk_args()) == EINVAL and "2 rows" in H.last_error()
    assert call(L, name, H.PALLAS, 12, 0, [None, None, 0] + [None] * 19) == OK  # an empty batch checks nothing


_CHILD = r"""
import ctypes, json, sys
import numpy as np
L = ctypes.CDLL(sys.argv[1])
L.halo_last_error.restype = ctypes.c_char_p
vp, sz = ctypes.c_void_p, ctypes.c_size_t
pts = np.zeros((96, 8), dtype=np.uint64); fes = np.ones((156, 4), dtype=np.uint64); out = np.zeros(2, dtype=np.uint8)
p, f = pts.ctypes.data_as(vp), fes.ctypes.data_as(vp)
args = [p, f, sz(2), p, p, p, f, p, p, p, f, p, f, f, p, f, f, f, out.ctypes.data_as(vp), None, None, None]
res = {"devices": L.halo_device_count()}
res["host"] = [L.halo_plonk_verify_succinct_batch(0, sz(8), sz(2), *args), L.halo_last_error().decode()]
res["dev"] = [L.halo_plonk_verify_succinct_batch_dev(0, sz(8), sz(2), *args, None), L.halo_last_error().decode()]
res["empty"] = L.halo_plonk_verify_succinct_batch(0, sz(8), sz(0), *args)
print(json.dumps(res))
"""


def test_unset_poseidon_parameters_in_a_fresh_process(L):
    """Before halo_poseidon_set_params both calls are HALO_EINVAL naming the call and that function; an empty
    batch is still HALO_OK."""
    import json
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", _CHILD, H.LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for key, name in zip(("host", "dev"), NAMES):
        rc, msg = res[key]
        assert rc == EINVAL and name in msg and "halo_poseidon_set_params" in msg
    assert res["empty"] == OK


def test_host_form_rejects_a_scalar_not_below_the_modulus(L):
    for slot in (1, 6, 10, 12, 13, 15, 16, 17):  # public inputs, vs, c, acc_prev z v, acc_next z v, mds
        args = plonk_args()
        big = np.ones((2 * 78, 4), dtype=np.uint64)
        big[(3 if slot in (1, 10) else 1) if slot != 6 else 80] = 0xFFFFFFFFFFFFFFFF
        args[slot] = H.ptr(big)
        assert call(L, NAMES[0], H.PALLAS, 8, 2, args) == EINVAL
        assert "not below the modulus" in H.last_error() and ("proof 1" in H.last_error() or slot == 17)
