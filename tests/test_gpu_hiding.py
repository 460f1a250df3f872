"""GPU parity: the hiding branch of pcdl::open_without_eval (pcdl.rs:344-371) outside the MSM shortcut.

Up to 2^16 coefficients halo_pcdl_open_combine forms C' through an MSM; above that, and always in the two
host entry points halo_pcdl_hiding_blind / halo_pcdl_hiding_combine, C' = C + alpha C_bar - w' S comes from
k_hiding_point (two single-lane GLV scalar multiplications) and p' from k_axpy_pad.  Here:
  * the host entry points against the committed reference transcript (tests/golden/transcript.npz) and
    against Python integers / oracle/pasta.py at the smallest shapes (d = 1, 3), one row per edge of the
    kernel: zero, one and r - 1 scalars, identities in and out, both additions forced to double, the
    length edges of p, scalars with an empty GLV half;
  * their refusals, which must leave every output buffer as it was;
  * the session path at n = 2^17 (the smallest size above the MSM shortcut) on a synthetic SRS with known
    discrete logs, through to a proof that passes the oracle's succinct_check.
Every comparison is integer or array equality."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pasta as P
import pcdl_check
import test_field_bounds as TB  # the Python restatement of the GLV constants (lambda)
from halo_amd import group, pcdl
from test_gpu_transcript import SpongeAdapter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
GLV_CFG = {"pallas": "PallasCurveCfg", "vesta": "VestaCurveCfg"}
R_INV = {m: pow(P.R_MONT, -1, m) for m in P.FIELDS.values()}
SENTINEL = 0xA5A5A5A5A5A5A5A5


def mont(x: int, m: int) -> np.ndarray:
    return np.array(P.int_to_limbs(P.to_mont(x % m, m)), dtype=np.uint64)


def mont_rows(xs, m: int) -> np.ndarray:
    return np.array([P.int_to_limbs(P.to_mont(x % m, m)) for x in xs], dtype=np.uint64).reshape(-1, 4)


def words_to_ints(a) -> list:
    """(k, 4) u64 words -> k Python integers (no Montgomery conversion)."""
    o = np.asarray(a, dtype=np.uint64).reshape(-1, 4).astype(object)
    return list(o[:, 0] | (o[:, 1] << 64) | (o[:, 2] << 128) | (o[:, 3] << 192))


def canon(a, m: int) -> list:
    """(k, 4) ark Montgomery scalars -> canonical Python integers."""
    ri = R_INV[m]
    return [x * ri % m for x in words_to_ints(a)]


def wrap(c, pt) -> np.ndarray:
    return np.array(P.point_to_wrapped(c, pt), dtype=np.uint64)


def unwrap(c, w):
    return P.wrapped_to_point(c, [int(x) for x in np.asarray(w).reshape(8)])


def c_prime_ref(c, Cp, alpha, Cb, wp, S):
    """C + alpha C_bar - w' S on affine points (pcdl.rs:371)."""
    return P.add(c, P.add(c, Cp, P.mul_fast(c, alpha, Cb)), P.neg(c, P.mul_fast(c, wp, S)))


def p_bar_ref(q, z, m):
    """(X - z) q for d coefficients q: d + 1 coefficients."""
    d = len(q)
    return [((q[j - 1] if j else 0) - (z * q[j] if j < d else 0)) % m for j in range(d + 1)]


def upload(hal, golden, corc, cname, n):
    S, Hh = golden[f"ref_sh_{cname}"]
    group.PublicParams.upload(cname, corc.srs_generate(cname, n), S, Hh, precompute_windows=False)
    return S, Hh


# ---------------------------------------------------------------------------------------------
# the host entry points against the reference transcript
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["open_pallas_n64_hiding", "open_pallas_n1024_hiding", "open_vesta_n16_hiding"])
def test_hiding_entry_points_match_transcript_fixture(hal, golden, corc, key):
    cname = key.split("_")[1]
    n = int(key.split("_")[2][1:])
    c = P.CURVES[cname]
    m, d = c.scalar, n - 1
    S, _ = upload(hal, golden, corc, cname, n)
    p, q = G[key + "_p"], G[key + "_q"]
    w, w_bar = G[key + "_w"]
    z = G[key + "_zv"][0]
    w_prime, alpha = G[key + "_wprime_alpha"]
    C, C_bar = G[key + "_C"][0], G[key + "_Cbar"][0]
    assert len(q) == d and len(p) <= n

    p_bar, got_cbar = pcdl.hiding_blind(q, d, z, w_bar, cname)
    assert np.array_equal(got_cbar, C_bar), key
    qi, zi = canon(q, m), canon(z, m)[0]
    pb = p_bar_ref(qi, zi, m)
    assert canon(p_bar, m) == pb and max(words_to_ints(p_bar)) < m, key
    _, cbar_only = pcdl.hiding_blind(q, d, z, w_bar, cname, want_p_bar=False)  # p_bar_out = NULL
    assert np.array_equal(cbar_only, C_bar), key

    p_prime, got_wp, got_cp = pcdl.hiding_combine(p, p_bar, d, alpha, C, C_bar, w, w_bar, cname)
    assert np.array_equal(got_wp, w_prime), key
    ai = canon(alpha, m)[0]
    pi = canon(p, m) + [0] * (n - len(p))
    assert canon(p_prime, m) == [(x + ai * y) % m for x, y in zip(pi, pb)] and max(words_to_ints(p_prime)) < m, key
    exp = c_prime_ref(c, unwrap(c, C), ai, unwrap(c, C_bar), canon(w_prime, m)[0], unwrap(c, S))
    assert np.array_equal(got_cp, wrap(c, exp)), key


# ---------------------------------------------------------------------------------------------
# edge rows at the smallest shapes that reach k_hiding_point
# ---------------------------------------------------------------------------------------------
ALPHA_HALVES = (0x0123456789ABCDEF0FEDCBA987654321, -0x0FEDCBA9876543210123456789ABCDEF)  # 121 and 124 bits


def edge_rows(c, lam, S, T, d):
    """(name, alpha, w, w_bar, C, C_bar, len(p)) with points as small known multiples of S and of the
    SRS point T = G_0; p and p_bar are fixed small vectors (see the test)."""
    r = c.scalar
    mul, add, neg = (lambda k, pt: P.mul_fast(c, k, pt)), (lambda a, b: P.add(c, a, b)), (lambda a: P.neg(c, a))
    C0, Cb0 = mul(3, T), add(mul(5, T), mul(2, S))
    # the default alpha has two full-size halves of opposite sign (the test asserts that it decomposes
    # back to them); the rows with an empty half are the named ones below
    a0, w0, wb0 = (ALPHA_HALVES[0] + lam * ALPHA_HALVES[1]) % r, 7, 11
    rows = [("alpha_zero", 0, w0, wb0, C0, Cb0, d + 1),
            ("alpha_one", 1, w0, wb0, C0, Cb0, d + 1),
            ("alpha_r_minus_1", r - 1, w0, wb0, C0, Cb0, d + 1),
            ("w_prime_zero", a0, -a0 * wb0 % r, wb0, C0, Cb0, d + 1),
            ("w_prime_zero_alpha_zero", 0, 0, wb0, C0, Cb0, d + 1),
            ("C_identity", a0, w0, wb0, P.INF, Cb0, d + 1),
            ("C_bar_identity", a0, w0, wb0, C0, P.INF, d + 1),
            ("both_identity", a0, w0, wb0, P.INF, P.INF, d + 1)]
    wp = (w0 + a0 * wb0) % r
    # C' is the identity: C = w' S - alpha C_bar
    rows.append(("C_prime_identity", a0, w0, wb0, add(mul(wp, S), neg(mul(a0, Cb0))), Cb0, d + 1))
    # C = alpha C_bar: lane 0's mixed addition meets its own point and must double
    rows.append(("madd_doubles", a0, w0, wb0, mul(a0, Cb0), Cb0, d + 1))
    rows.append(("madd_cancels", a0, w0, wb0, neg(mul(a0, Cb0)), Cb0, d + 1))
    # C + alpha C_bar = -w' S: the final addition meets its own point and must double
    rows.append(("final_add_doubles", a0, w0, wb0, add(neg(mul(wp, S)), neg(mul(a0, Cb0))), Cb0, d + 1))
    for ln in (0, 1, d, d + 1):
        rows.append((f"len_{ln}", a0, w0, wb0, C0, Cb0, ln))
    # an empty GLV half: small alpha is (alpha, 0), lambda is (0, 1), r - lambda is (0, -1); the same for w'
    for name, a in (("alpha_3", 3), ("alpha_2p100", 1 << 100), ("alpha_lambda", lam), ("alpha_minus_lambda", r - lam),
                    ("alpha_lambda_plus_1", lam + 1)):
        rows.append((name, a, w0, wb0, C0, Cb0, d + 1))
    rows.append(("w_prime_lambda", a0, (lam - a0 * wb0) % r, wb0, C0, Cb0, d + 1))
    rows.append(("w_prime_small", a0, (5 - a0 * wb0) % r, wb0, C0, Cb0, d + 1))
    rows.append(("w_prime_r_minus_1", a0, (r - 1 - a0 * wb0) % r, wb0, C0, Cb0, d + 1))
    return rows


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_hiding_combine_edge_rows(hal, golden, corc, cname):
    c = P.CURVES[cname]
    r = c.scalar
    S, _ = upload(hal, golden, corc, cname, 4)
    Sp = unwrap(c, S)
    T = unwrap(c, corc.srs_generate(cname, 1)[0])
    cfg = TB._glv_consts()[GLV_CFG[cname]]
    lam = TB.glv_lambda(cfg, r)
    assert pow(lam, 3, r) == 1 and lam != 1
    assert TB.glv_decompose(cfg, lam) == (0, 1) and TB.glv_decompose(cfg, r - lam) == (0, -1)
    assert TB.glv_decompose(cfg, 1 << 100) == (1 << 100, 0)
    assert TB.glv_decompose(cfg, (ALPHA_HALVES[0] + lam * ALPHA_HALVES[1]) % r) == ALPHA_HALVES
    pv = [r - 1, 2, (r + 1) // 2, 0x123456789ABCDEF0123456789]  # p, then cut to each row's length
    pbv = [1, r - 1, 0, (r - 1) // 2]
    for d in (1, 3):
        for name, alpha, w, w_bar, Cp, Cb, ln in edge_rows(c, lam, Sp, T, d):
            what = f"{cname} d={d} {name}"
            p = mont_rows(pv[:ln], r) if ln else None
            p_prime, w_prime, C_prime = pcdl.hiding_combine(p, mont_rows(pbv[: d + 1], r), d, mont(alpha, r), wrap(c, Cp),
                                                            wrap(c, Cb), mont(w, r), mont(w_bar, r), cname)
            wp = (w + alpha * w_bar) % r
            assert np.array_equal(w_prime, mont(wp, r)), what
            exp_p = [((pv[j] if j < ln else 0) + alpha * pbv[j]) % r for j in range(d + 1)]
            assert np.array_equal(p_prime, mont_rows(exp_p, r)), what
            exp = c_prime_ref(c, Cp, alpha % r, Cb, wp, Sp)
            assert np.array_equal(C_prime, wrap(c, exp)), what
            if name == "C_prime_identity":
                assert exp is P.INF and not C_prime.any(), what
            if name == "final_add_doubles":
                assert exp == P.neg(c, P.mul_fast(c, 2 * wp % r, Sp)), what


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_hiding_blind_smallest_shapes(hal, golden, corc, cname):
    """d = 1 and d = 3: C_bar = commit((X - z) q, w_bar) against the oracle MSM, with zero and boundary
    scalars among q, z and w_bar."""
    c = P.CURVES[cname]
    r = c.scalar
    S, _ = upload(hal, golden, corc, cname, 4)
    Sp = unwrap(c, S)
    gs = [unwrap(c, g) for g in corc.srs_generate(cname, 4)]
    cases = [([5, 0, r - 1], 3, 7), ([r - 1, r - 2, 1], r - 1, r - 1), ([0, 0, 0], 9, 0), ([1, 1, 1], 0, 1),
             ([2, 3, 4], 1, 0)]
    for d in (1, 3):
        for q, z, w_bar in cases:
            q = q[:d]
            p_bar, C_bar = pcdl.hiding_blind(mont_rows(q, r), d, mont(z, r), mont(w_bar, r), cname)
            pb = p_bar_ref(q, z, r)
            assert np.array_equal(p_bar, mont_rows(pb, r)), (cname, d, q, z)
            exp = P.add(c, P.msm(c, gs[: d + 1], pb), P.mul_fast(c, w_bar, Sp))
            assert np.array_equal(C_bar, wrap(c, exp)), (cname, d, q, z, w_bar)


# ---------------------------------------------------------------------------------------------
# refusals: the reference's assertions and the argument checks; nothing is written
# ---------------------------------------------------------------------------------------------
def _raw_calls(hal, cid, d, ln, null=None):
    """Both entry points through the raw ABI with sentinel-filled outputs.  Returns
    [(rc, message, outputs untouched)] for blind and combine; `null` names one argument passed as NULL."""
    L = hal.load()
    k = max(d + 1, ln, 1) + 2
    one = np.zeros((k, 4), dtype=np.uint64)
    one[:, 0] = 1
    pt = np.zeros(8, dtype=np.uint64)
    res = []
    outs = [np.full((k, 4), SENTINEL, dtype=np.uint64), np.full(8, SENTINEL, dtype=np.uint64)]
    a = {"q": one, "z": one[0], "w_bar": one[0], "p_bar_out": outs[0], "C_bar_out": outs[1]}
    if null in a:
        a[null] = None
    rc = L.halo_pcdl_hiding_blind(cid, hal.ptr(a["q"]), d, hal.ptr(a["z"]), hal.ptr(a["w_bar"]), hal.ptr(a["p_bar_out"]),
                                  hal.ptr(a["C_bar_out"]))
    res.append((rc, hal.last_error() if rc else "", all((o == SENTINEL).all() for o in outs)))
    outs = [np.full((k, 4), SENTINEL, dtype=np.uint64), np.full(4, SENTINEL, dtype=np.uint64),
            np.full(8, SENTINEL, dtype=np.uint64)]
    a = {"p": one, "p_bar": one, "alpha": one[0], "C": pt, "C_bar": pt, "w": one[0], "w_bar": one[0],
         "p_prime_out": outs[0], "w_prime_out": outs[1], "C_prime_out": outs[2]}
    if null in a:
        a[null] = None
    rc = L.halo_pcdl_hiding_combine(cid, hal.ptr(a["p"]), ln, hal.ptr(a["p_bar"]), d, hal.ptr(a["alpha"]), hal.ptr(a["C"]),
                                    hal.ptr(a["C_bar"]), hal.ptr(a["w"]), hal.ptr(a["w_bar"]), hal.ptr(a["p_prime_out"]),
                                    hal.ptr(a["w_prime_out"]), hal.ptr(a["C_prime_out"]))
    res.append((rc, hal.last_error() if rc else "", all((o == SENTINEL).all() for o in outs)))
    return res


EINVAL, ENOTPOW2, ESRSRANGE, EDEGREE = 1, 4, 5, 6


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_hiding_refusals_leave_outputs_untouched(hal, golden, corc, cname):
    cid = hal.CURVES[cname]
    upload(hal, golden, corc, cname, 4)  # D = 3
    for d, code, text in ((0, EINVAL, "n > 1"), (2, ENOTPOW2, "n (3) is not a power of two"),
                          (5, ENOTPOW2, "n (6) is not a power of two"), (7, ESRSRANGE, "d <= pp.D"),
                          (15, ESRSRANGE, "d <= pp.D")):
        for rc, msg, untouched in _raw_calls(hal, cid, d, 1):
            assert rc == code and text in msg and untouched, (d, rc, msg)
    # len > d + 1 (combine only; the blind has no p)
    for d, ln in ((1, 3), (3, 5)):
        ok, (rc, msg, untouched) = _raw_calls(hal, cid, d, ln)
        assert ok[0] == hal.HALO_OK
        assert rc == EDEGREE and untouched, (d, ln, rc, msg)
    # null arguments (p may be NULL only with len = 0; p_bar_out may always be NULL)
    for null in ("q", "z", "w_bar", "C_bar_out"):
        rc, msg, untouched = _raw_calls(hal, cid, 3, 1, null)[0]
        assert rc == EINVAL and "invalid argument" in msg and untouched, null
    for null in ("p", "p_bar", "alpha", "C", "C_bar", "w", "w_bar", "p_prime_out", "w_prime_out", "C_prime_out"):
        rc, msg, untouched = _raw_calls(hal, cid, 3, 1, null)[1]
        assert rc == EINVAL and "invalid argument" in msg and untouched, null
    for bad_curve in (2, -1):
        for rc, msg, untouched in _raw_calls(hal, bad_curve, 3, 1):
            assert rc == EINVAL and untouched, bad_curve
    # and the same calls with nothing wrong succeed
    assert [x[0] for x in _raw_calls(hal, cid, 3, 4)] == [hal.HALO_OK, hal.HALO_OK]


_NO_SH_CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
from halo_amd import _lib as hal
import test_gpu_hiding as T
hal.ensure_device()
out = {{}}
for cname, cid in hal.CURVES.items():
    hal.check(hal.load().halo_srs_synthesize(cid, 4, 7))  # a resident SRS, and no (S, H) in this process
    out[cname] = [[rc, msg, bool(ok)] for rc, msg, ok in T._raw_calls(hal, cid, 3, 4)]
print("RESULT " + json.dumps(out))
"""


def test_hiding_refused_without_s_and_h(hal):
    """(S, H) stay resident for the life of a process once any test has uploaded them, so the refusal is
    taken in a fresh process that only synthesizes an SRS."""
    code = _NO_SH_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oracle"),
                                                       os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    for cname, calls in json.loads(line[7:]).items():
        for rc, msg, untouched in calls:
            assert rc == ESRSRANGE and "(S, H)" in msg and untouched, (cname, rc, msg)


# ---------------------------------------------------------------------------------------------
# the session path above the MSM shortcut: n = 2^17
# ---------------------------------------------------------------------------------------------
def det_scalars(seed: int, k: int) -> np.ndarray:
    """k Montgomery-form scalars (words < 2^254, below both moduli) from seed."""
    a = np.random.default_rng(seed).integers(0, 2**64 - 1, size=(k, 4), dtype=np.uint64, endpoint=True)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return np.ascontiguousarray(a)


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_hiding_open_session_2p17(hal, golden, corc, cname):
    """halo_pcdl_open_begin -> _blind -> _combine at n = 2^17 (pcdl_pbar_device + the bucket MSM with a hiding
    scalar, then k_axpy_pad + k_hiding_point), on G_j = k_j G with known k_j and the reference's (S, H):
    C_bar = (sum p_bar_j k_j) G + w_bar S, w', C' and all 2^17 session coefficients against Python
    integers; then the rounds under the oracle sponge, and the proof through the oracle's succinct_check."""
    L = hal.load()
    c = P.CURVES[cname]
    cid, r = hal.CURVES[cname], c.scalar
    n = 1 << 17
    d, seed = n - 1, 0x48494445 + cid
    S, Hh = golden[f"ref_sh_{cname}"]
    Sp = unwrap(c, S)
    hal.check(L.halo_srs_synthesize(cid, n, seed))
    gs = group.PublicParams.read(cid, 0, n)
    group.PublicParams.upload(cid, gs, S, Hh, precompute_windows=False)
    k = words_to_ints(corc.synth_scalars(seed, n))
    for j in (0, 1, n - 1):
        assert k[j] == group.synth_scalar(seed, j, cname)
    assert np.array_equal(gs[n - 1], wrap(c, P.mul_fast(c, k[n - 1], c.generator)))

    def known_log_point(coeffs):  # (sum_j coeffs_j k_j) G
        acc = sum(x * y for x, y in zip(coeffs, k)) % r
        return unwrap(c, corc.generator_mul(cname, np.array(P.int_to_limbs(acc), dtype=np.uint64)))

    ins = det_scalars(seed + 1, 2 * n + 8)
    plen = n - 5  # shorter than n: the session pads p
    p, q = ins[:plen], ins[n: n + d]
    z, w, w_bar, alpha = ins[2 * n], ins[2 * n + 1], ins[2 * n + 2], ins[2 * n + 3]
    pi, qi = canon(p, r), canon(q, r)
    zi, wi, wbi, ai = canon([z, w, w_bar, alpha], r)
    C = P.add(c, known_log_point(pi), P.mul_fast(c, wi, Sp))
    vi = P.horner(pi, zi, r)

    s = ctypes.c_void_p()
    v_out = np.zeros(4, dtype=np.uint64)
    hal.check(L.halo_pcdl_open_begin(cid, hal.ptr(p), plen, d, hal.ptr(z), hal.ptr(v_out), ctypes.byref(s)))
    ses = pcdl.IpaSession.__new__(pcdl.IpaSession)
    ses.curve, ses.n, ses._s = cid, n, s
    try:
        assert np.array_equal(v_out, mont(vi, r))
        C_bar = np.zeros(8, dtype=np.uint64)
        hal.check(L.halo_pcdl_open_blind(s, hal.ptr(q), hal.ptr(w_bar), hal.ptr(C_bar)))
        pb = p_bar_ref(qi, zi, r)
        Cb = P.add(c, known_log_point(pb), P.mul_fast(c, wbi, Sp))
        assert np.array_equal(C_bar, wrap(c, Cb))

        w_prime = np.zeros(4, dtype=np.uint64)
        C_prime = np.zeros(8, dtype=np.uint64)
        Cw = wrap(c, C)
        hal.check(L.halo_pcdl_open_combine(s, hal.ptr(alpha), hal.ptr(Cw), hal.ptr(w), hal.ptr(w_prime), hal.ptr(C_prime)))
        wpi = (wi + ai * wbi) % r
        assert np.array_equal(w_prime, mont(wpi, r))
        assert np.array_equal(C_prime, wrap(c, c_prime_ref(c, C, ai, Cb, wpi, Sp)))
        m, _, cs, _ = ses.state(with_gs=False)
        assert 2 * m == n
        assert max(words_to_ints(cs)) < r
        assert canon(cs, r) == [(x + ai * y) % r for x, y in zip(pi + [0] * (n - plen), pb)]

        # the rounds (pcdl.rs:387-450) under the oracle sponge, from xi_0 = rho(C', z, v)
        t = SpongeAdapter(cname)
        t.absorb_g([C_prime])
        t.absorb_fr([z, v_out])
        xi = np.ascontiguousarray(t.challenge(), dtype=np.uint64)
        xis = [xi]
        hal.check(L.halo_pcdl_open_start(s, None, hal.ptr(xi)))
        Ls, Rs = [], []
        for _ in range(17):
            Lp, Rp = ses.round_lr()
            Ls.append(Lp)
            Rs.append(Rp)
            t.absorb_fr([xi])
            t.absorb_g([Lp, Rp])
            xi = np.ascontiguousarray(t.challenge(), dtype=np.uint64)
            xis.append(xi)
            ses.fold(xi)
        U, cfin = ses.end()
    finally:
        if ses._s is not None:
            L.halo_ipa_end(ses._s, None, None)
            ses._s = None
    pcdl_check.succinct_check(cname, Cw, d, zi, vi, Ls, Rs, U, canon(cfin, r)[0], canon(np.stack(xis), r), Hh, S=S,
                              C_bar=C_bar, w_prime=wpi, alpha=ai)
