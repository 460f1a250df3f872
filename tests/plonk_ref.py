"""CPU restatement of PlonkProof::verify_succinct / verify (crates/plonk/src/plonk/protocol.rs:357-502) and of the
prover's round 5 under the reference's transcripts.  TEST INFRASTRUCTURE ONLY.

* ``verify_succinct`` / ``verify``: big integers over oracle/poseidon.Sponge (the PLONK, PCDL and ASDL transcripts),
  oracle/pcdl_check (succinct_check, h_eval) and the ``*_generic`` gate functions transcribed in
  halo_amd/prover.py.  They return halo_plonk_verify_succinct_batch's verdict code and readbacks.
* ``CpuBackend``: oracle/prover_ref.RefBackend plus the two round-5 hooks of ``naive_prover(..., transcript=...)``
  over oracle/pcdl_ref.open_without_eval (Instance::open, acc::prover).
* ``satisfiable_circuit``: witness and selector evaluations of a small circuit whose every gate kind but
  affine-mul and range-check is active, with copy cycles.

A proof travels as a ``Rec``: numpy arrays in halo_plonk_verify_succinct_batch's layout (WrappedPoints, ark scalars).
"""
from __future__ import annotations

import functools
import os
import sys
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pasta as P  # noqa: E402
import pcdl_check  # noqa: E402
import poseidon  # noqa: E402
from halo_amd import prover as PR  # noqa: E402
from prover_ref import RefBackend  # noqa: E402

ACCEPT, IDENTITY, INSTANCE_0, INSTANCE_1, INSTANCE_2, C_BAR, Z, V, MALFORMED = range(9)
LABELS = {"PCDL": poseidon.PCDL, "ASDL": poseidon.ASDL, "PLONK": poseidon.PLONK}
SCALAR_FIELD = {"pallas": "fp", "vesta": "fq"}
V_WS, V_RS, V_QS, V_TS, V_IDS, V_SIGMAS, V_Z, V_Z_OMEGA, V_W_OMEGAS, N_EVALS = 0, 16, 31, 41, 57, 65, 73, 74, 75, 78


class Rec(NamedTuple):
    """One proof with its public inputs, as the device reads it."""
    pub: np.ndarray       # (npi, 4)
    C_ws: np.ndarray      # (16, 8)
    C_z: np.ndarray       # (8,)
    C_ts: np.ndarray      # (16, 8)
    vs: np.ndarray        # (78, 4)
    Ls: np.ndarray        # (3, lg, 8): acc_prev, r, r_omega
    Rs: np.ndarray
    U: np.ndarray         # (3, 8)
    c: np.ndarray         # (3, 4)
    prev: np.ndarray      # (16,) u64: C (8), z (4), v (4)
    next: np.ndarray      # (16,)
    next_pi: tuple        # (Ls (lg, 8), Rs (lg, 8), U (8,), c (4,)) of acc_next.pi, read by verify alone


def fe(x: int, m: int) -> np.ndarray:
    return np.array(P.int_to_limbs(P.to_mont(x % m, m)), dtype=np.uint64)


def to_int(x, m: int) -> int:
    return P.from_mont(P.limbs_to_int([int(v) for v in np.asarray(x).reshape(4)]), m)


def wrapped(c, pt) -> np.ndarray:
    return np.array(P.point_to_wrapped(c, pt), dtype=np.uint64)


class Malformed(Exception):
    pass


def _pt(c, w):
    """A WrappedPoint as an affine point; Malformed when it is neither (0, 0) nor on the curve."""
    w = [int(x) for x in np.asarray(w).reshape(8)]
    x, y = P.limbs_to_int(w[:4]), P.limbs_to_int(w[4:])
    if x == 0 and y == 0:
        return P.INF
    if x >= c.base or y >= c.base:
        raise Malformed
    pt = (P.from_mont(x, c.base), P.from_mont(y, c.base))
    if not P.on_curve(c, pt):
        raise Malformed
    return pt


def scalar_mds(cname: str):
    """P::SCALAR_POSEIDON_MDS (wrappers.rs:518,579): the Poseidon MDS matrix of the curve's scalar field."""
    return poseidon.constants(SCALAR_FIELD[cname])[0]


class SpongeAdapter:
    """oracle/poseidon.Sponge behind the reference's interface over WrappedPoints / ark scalars: the
    ``new_transcript(label)`` product of halo_amd.acc and halo_amd.prover.naive_prover."""

    def __init__(self, cname, label):
        self.c = P.CURVES[cname]
        self.s = poseidon.Sponge(cname, LABELS[label])

    def absorb_g(self, pts):
        self.s.absorb_g([P.wrapped_to_point(self.c, [int(x) for x in np.asarray(q).reshape(8)]) for q in pts])

    def absorb_fr(self, xs):
        self.s.absorb_fr([to_int(x, self.c.scalar) for x in xs])

    def challenge(self):
        return fe(self.s.challenge(), self.c.scalar)


def new_transcript(cname):
    return lambda label: SpongeAdapter(cname, label)


# ---------------------------------------------------------------------------------------------
# the verifier
# ---------------------------------------------------------------------------------------------
def pcdl_xis(cname, C, z, v, Ls, Rs):
    """xi_0 .. xi_lg of a plain instance (pcdl.rs:518-534): the transcript walk alone, defined for proofs that
    fail the check too.  Affine points, canonical scalars."""
    t = poseidon.Sponge(cname, poseidon.PCDL)
    t.absorb_g([C])
    t.absorb_fr([z, v])
    xis = [t.challenge()]
    for L, R in zip(Ls, Rs):
        t.absorb_fr([xis[-1]])
        t.absorb_g([L, R])
        xis.append(t.challenge())
    return xis


def gate_identity(m, mds, vs, pub, n, beta, gamma, alpha, xi):
    """(f, t z_H) of protocol.rs:396-444 from the 78 evaluations (canonical integers)."""
    ws, rs, qs, ts = vs[V_WS:V_RS], vs[V_RS:V_QS], vs[V_QS:V_TS], vs[V_TS:V_IDS]
    ids, sigmas, z, z_omega, nw = vs[V_IDS:V_SIGMAS], vs[V_SIGMAS:V_Z], vs[V_Z], vs[V_Z_OMEGA], vs[V_W_OMEGAS:]
    omega = pow(5, (m - 1) // n, m)
    xi_n = pow(xi, n, m)
    f_prime = g_prime = 1
    for i in range(PR.S_POLYS):
        f_prime = f_prime * (ws[i] + beta * ids[i] + gamma) % m
        g_prime = g_prime * (ws[i] + beta * sigmas[i] + gamma) % m
    f_gc = (ws[0] * qs[0] + ws[1] * qs[1] + ws[2] * qs[2] + ws[0] * ws[1] * qs[3] + qs[4]
            + qs[5] * PR.poseidon_constraints(mds, rs, ws, nw, lambda x: pow(x, 7, m))
            + qs[6] * PR.affine_add_constraints(ws, 1)
            + qs[7] * PR.affine_mul_constraints(ws, nw, rs[0], 1)
            + qs[8] * PR.eq_constraints(ws)
            + qs[9] * PR.range_check_constraints(ws, nw, rs))
    omega_j = omega
    for x in pub:  # public_input_eval_generic (protocol.rs:564-589)
        den = n * (xi - omega_j) % m
        if den == 0:
            raise Malformed
        f_gc += (xi_n - 1) * omega_j * pow(den, -1, m) * -x
        omega_j = omega_j * omega % m
    den = n * (xi - omega) % m
    if den == 0:
        raise Malformed
    l1 = omega * (xi_n - 1) * pow(den, -1, m) % m
    f_cc1 = l1 * (z - 1)
    f_cc2 = z * f_prime - z_omega * g_prime
    f = (f_gc + alpha * f_cc1 + alpha * alpha * f_cc2) % m
    t = sum(ts[i] * pow(xi_n, i, m) for i in range(PR.T_POLYS)) % m
    return f, t * (xi_n - 1) % m


def geometric(c, zeta, pts):
    acc, zp = P.INF, 1
    for pt in pts:
        acc = P.add(c, acc, P.mul_fast(c, zp, pt))
        zp = zp * zeta % c.scalar
    return acc


def _verify_succinct(cname, rows, C_qs_b, H_b, rec: Rec):
    c = P.CURVES[cname]
    m = c.scalar
    lg = rows.bit_length() - 1
    d = rows - 1
    out = {"challenges": None, "sides": None, "asdl": None}
    try:
        C_qs = [_pt(c, w) for w in np.frombuffer(C_qs_b, dtype=np.uint64).reshape(10, 8)]
        C_ws, C_ts, C_z = [_pt(c, w) for w in rec.C_ws], [_pt(c, w) for w in rec.C_ts], _pt(c, rec.C_z)
        Ls = [[_pt(c, w) for w in row] for row in rec.Ls]
        Rs = [[_pt(c, w) for w in row] for row in rec.Rs]
        Us = [_pt(c, w) for w in rec.U]
        prev_C, next_C = _pt(c, rec.prev[:8]), _pt(c, rec.next[:8])
        raw = [P.limbs_to_int([int(v) for v in x]) for x in
               list(rec.vs) + list(rec.pub) + list(rec.c) + [rec.prev[8:12], rec.prev[12:], rec.next[8:12], rec.next[12:]]]
        if any(x >= m for x in raw):
            raise Malformed
        vs = [to_int(x, m) for x in rec.vs]
        pub = [to_int(x, m) for x in rec.pub]
        cs = [to_int(x, m) for x in rec.c]
        prev_z, prev_v, next_z, next_v = (to_int(x, m) for x in (rec.prev[8:12], rec.prev[12:], rec.next[8:12], rec.next[12:]))
        # the PLONK transcript (protocol.rs:366-395)
        t = poseidon.Sponge(cname, poseidon.PLONK)
        t.absorb_g(C_ws)
        beta, gamma = t.challenge(), t.challenge()
        t.absorb_g([C_z])
        alpha = t.challenge()
        t.absorb_g(C_ts)
        zeta, xi = t.challenge(), t.challenge()
        out["challenges"] = [beta, gamma, alpha, zeta, xi]
        f, tz = gate_identity(m, scalar_mds(cname), vs, pub, rows, beta, gamma, alpha, xi)
        out["sides"] = [f, tz]
    except Malformed:
        return MALFORMED, out
    code = ACCEPT if f == tz else IDENTITY
    # the instances (protocol.rs:453-487)
    zp = [pow(zeta, i, m) for i in range(43)]
    r_evals = vs[V_QS:V_TS] + vs[V_WS:V_RS] + vs[V_TS:V_IDS] + [vs[V_Z]]
    ro_evals = vs[V_W_OMEGAS:] + [vs[V_Z_OMEGA]]
    v_r = sum(e * p for e, p in zip(r_evals, zp)) % m
    v_ro = sum(e * p for e, p in zip(ro_evals, zp)) % m
    C_r = geometric(c, zeta, C_qs + C_ws + C_ts + [C_z])
    C_ro = geometric(c, zeta, C_ws[:3] + [C_z])
    omega = pow(5, (m - 1) // rows, m)
    insts = [(prev_C, prev_z, prev_v), (C_r, xi, v_r), (C_ro, xi * omega % m, v_ro)]
    H_w = np.frombuffer(H_b, dtype=np.uint64)
    xis = []
    for j, (C, z, v) in enumerate(insts):
        x = pcdl_xis(cname, C, z, v, Ls[j], Rs[j])
        xis.append(x)
        if code == ACCEPT:
            try:
                if any(xx == 0 for xx in x[1:]):
                    raise AssertionError("zero challenge")
                pcdl_check.succinct_check(cname, wrapped(c, C), d, z, v, rec.Ls[j], rec.Rs[j], rec.U[j], cs[j], x, H_w)
            except AssertionError:
                code = INSTANCE_0 + j
    # acc::verifier (acc.rs:157-169, 207-210)
    t = poseidon.Sponge(cname, poseidon.ASDL)
    t.absorb_fr([x for row in xis for x in row])
    t.absorb_g(Us)
    a = t.challenge()
    z_prime = t.challenge()
    out["asdl"] = [a, z_prime]
    if code == ACCEPT:
        C_bar = geometric(c, a, Us)
        hv = sum(pow(a, j, m) * pcdl_check.h_eval(xis[j], z_prime, m) for j in range(3)) % m
        if C_bar != next_C:
            code = C_BAR
        elif z_prime != next_z:
            code = Z
        elif hv != next_v:
            code = V
    return code, out


@functools.lru_cache(maxsize=None)
def _cached(cname, rows, C_qs_b, H_b, rec_b):
    import pickle
    return _verify_succinct(cname, rows, C_qs_b, H_b, Rec(*pickle.loads(rec_b)))


def verify_succinct(cname, rows, C_qs, H_point, rec: Rec):
    """(verdict code, {challenges, sides, asdl}) of one proof; the values canonical integers (None where a
    malformed proof has none).  Memoised on the bytes of its inputs: batches repeat proofs."""
    import pickle
    b = lambda a: np.ascontiguousarray(a, dtype=np.uint64).tobytes()  # noqa: E731
    return _cached(cname, rows, b(C_qs), b(H_point), pickle.dumps(tuple(rec)))


def verify(cname, rows, C_qs, H_point, rec: Rec, srs):
    """verify_succinct, then acc::decider (pcdl::check of acc_next).  Returns (code, message): message "" on
    accept, "succinct" / "decider" naming what pcdl::check rejected."""
    import corc
    code, _ = verify_succinct(cname, rows, C_qs, H_point, rec)
    if code != ACCEPT:
        return code, "verify_succinct"
    c = P.CURVES[cname]
    m = c.scalar
    Ls, Rs, U, cc = rec.next_pi
    z, v = to_int(rec.next[8:12], m), to_int(rec.next[12:], m)
    xis = pcdl_xis(cname, _pt(c, rec.next[:8]), z, v, [_pt(c, w) for w in Ls], [_pt(c, w) for w in Rs])
    try:
        pcdl_check.succinct_check(cname, rec.next[:8], rows - 1, z, v, Ls, Rs, U, to_int(cc, m), xis, H_point)
    except AssertionError:
        return ACCEPT, "succinct"
    if not pcdl_check.decider_commit_matches(cname, U, xis, srs, corc.msm):
        return ACCEPT, "decider"
    return ACCEPT, ""


# ---------------------------------------------------------------------------------------------
# the prover's CPU backend
# ---------------------------------------------------------------------------------------------
class CpuBackend(RefBackend):
    """RefBackend with the round-5 hooks of naive_prover's transcript mode (Instance::open and acc::prover under
    the oracle's sponges, the openings by oracle/pcdl_ref.open_without_eval) and the commitments on the C oracle."""

    def __init__(self, cname, srs_wrapped, s_wrapped, h_wrapped):
        super().__init__(cname, srs_wrapped, h_wrapped)
        self.cname = cname
        self.srs_w = np.ascontiguousarray(srs_wrapped)
        self.S_point = P.wrapped_to_point(self.c, [int(x) for x in s_wrapped])

    def _fes(self, xs):
        return np.array([P.int_to_limbs(P.to_mont(x % self.m, self.m)) for x in xs], dtype=np.uint64).reshape(-1, 4)

    def commit_many(self, polys):
        import corc
        return [corc.msm(self.cname, np.ascontiguousarray(self.srs_w[:len(p)]), self._fes(p)) if len(p)
                else np.zeros(8, dtype=np.uint64) for p in polys]

    def _open(self, p, C_w, d, z, v):
        import pcdl_ref
        o = pcdl_ref.open_without_eval(self.cname, p, P.wrapped_to_point(self.c, [int(x) for x in C_w]), d, z, v,
                                       self.srs_w, self.S_point, self.H_point)
        return {"C": np.asarray(C_w, dtype=np.uint64), "z": z, "v": v, "Ls": [self._w(L) for L in o["Ls"]],
                "Rs": [self._w(R) for R in o["Rs"]], "U": self._w(o["U"]), "c": o["c"], "xis": o["xis"]}

    def instance_open(self, p, d, z, new_transcript):
        """Instance::open (pcdl.rs:41-51), w = None."""
        p = list(p) + [0] * (d + 1 - len(p))
        return self._open(p, self.commit_many([p])[0], d, z, P.horner(p, z, self.m))

    def acc_prove(self, qs, d, new_transcript):
        """acc::prover (acc.rs:178-198); the succinct checks of common_subroutine are the restated verifier's."""
        c, m = self.c, self.m
        pt = lambda w: P.wrapped_to_point(c, [int(x) for x in w])  # noqa: E731
        xis = [pcdl_xis(self.cname, pt(q["C"]), q["z"], q["v"], [pt(w) for w in q["Ls"]], [pt(w) for w in q["Rs"]])
               for q in qs]
        H_w = self._w(self.H_point)
        for q, x in zip(qs, xis):
            pcdl_check.succinct_check(self.cname, q["C"], d, q["z"], q["v"], q["Ls"], q["Rs"], q["U"], q["c"], x, H_w)
        t = poseidon.Sponge(self.cname, poseidon.ASDL)
        t.absorb_fr([x for row in xis for x in row])
        t.absorb_g([pt(q["U"]) for q in qs])
        a = t.challenge()
        C = geometric(c, a, [pt(q["U"]) for q in qs])
        z = t.challenge()
        h = [0] * (d + 1)
        for j, x in enumerate(xis):
            aj = pow(a, j, m)
            h = [(u + aj * w) % m for u, w in zip(h, pcdl_check.h_coeffs(x, m))]
        v = sum(pow(a, j, m) * pcdl_check.h_eval(x, z, m) for j, x in enumerate(xis)) % m
        assert v == P.horner(h, z, m)
        return self._open(h, self._w(C), d, z, v)

    def fresh_accumulator(self, d, seed):
        """acc::prover of one fresh opening: the first acc_prev of a chain."""
        rng = np.random.default_rng(seed)
        p = [int.from_bytes(rng.bytes(32), "little") % self.m for _ in range(d + 1)]
        z = int.from_bytes(rng.bytes(32), "little") % self.m
        return self.acc_prove([self.instance_open(p, d, z, None)], d, None)


# ---------------------------------------------------------------------------------------------
# a satisfiable circuit
# ---------------------------------------------------------------------------------------------
def satisfiable_circuit(B, n: int, seed: int = 1, cname: str = "pallas"):
    """Witness and selector polynomials of an n-row circuit (n >= 8) that naive_prover can prove, as its ``wit``.

    Row i is the evaluation at omega^i.  Evals::from_vec_and_domain rotates by one, so public input j sits at
    omega^(j + 1): row 0 constant (a = 1), rows 1-2 the public inputs, 3 add, 4 mul, 5 eq (q8), 6 a 5-round Poseidon
    row (q5) whose result is row 7's w[0..2], 7 a generic-case affine add (q6) over those values.  The other rows
    are empty.  Copy cycles tie equal cells of the first 8 columns (ids / sigmas)."""
    assert n >= 8 and n & (n - 1) == 0
    m = B.m
    rng = np.random.default_rng(seed)
    rnd = lambda: int.from_bytes(rng.bytes(32), "little") % m  # noqa: E731
    inv = lambda x: pow(x, -1, m)  # noqa: E731
    mds = scalar_mds(cname)
    W = [[0] * n for _ in range(PR.W_POLYS)]
    Q = [[0] * n for _ in range(PR.Q_POLYS)]
    R = [[0] * n for _ in range(PR.R_POLYS)]
    x0, x1 = rnd(), rnd()
    W[0][0], Q[0][0], Q[4][0] = 1, 1, m - 1                                 # a - 1 = 0
    W[0][1], Q[0][1] = x0, 1                                                # a + PI = 0
    W[0][2], Q[0][2] = x1, 1
    s = (x0 + x1) % m
    W[0][3], W[1][3], W[2][3], Q[0][3], Q[1][3], Q[2][3] = x0, x1, s, 1, 1, m - 1    # a + b - c = 0
    b4 = rnd()
    pr = s * b4 % m
    W[0][4], W[1][4], W[2][4], Q[3][4], Q[2][4] = s, b4, pr, 1, m - 1       # a b - c = 0
    W[0][5], W[1][5], W[2][5], W[3][5], W[4][5], Q[8][5] = pr, x0, 1, 0, inv(pr - x0), 1   # eq: a != b
    st = [pr, s, x1]                                                        # Poseidon over three circuit values
    Q[5][6] = 1
    for rd in range(5):
        for j in range(3):
            W[3 * rd + j][6] = st[j]
            R[3 * rd + j][6] = rnd()
        sb = [pow(x, 7, m) for x in st]
        st = [(R[3 * rd + i][6] + sum(mds[i][j] * sb[j] for j in range(3))) % m for i in range(3)]
    xp, yp, xq = st                                                         # affine add, generic case
    yq = rnd()
    lam = (yq - yp) * inv(xq - xp) % m
    xr = (lam * lam - xp - xq) % m
    yr = (lam * (xp - xr) - yp) % m
    row7 = [xp, yp, xq, yq, xr, yr, inv(xq - xp), inv(xp), inv(xq), 0, lam]
    for j, x in enumerate(row7):
        W[j][7] = x
    Q[6][7] = 1
    # copy cycles between equal cells (column, row) of the first S_POLYS columns
    label = lambda col, row: (col * n + row + 1) % m  # noqa: E731
    ids = [[label(col, row) for row in range(n)] for col in range(PR.S_POLYS)]
    sig = [list(col) for col in ids]
    cycles = [[(0, 1), (0, 3), (1, 5)], [(0, 2), (1, 3), (2, 6)], [(2, 3), (0, 4), (1, 6)], [(2, 4), (0, 5), (0, 6)],
              [(0, 0), (2, 5)]]
    for cyc in cycles:
        assert len({W[col][row] for col, row in cyc}) == 1
        for (col, row), (c2, r2) in zip(cyc, cyc[1:] + cyc[:1]):
            sig[col][row] = label(c2, r2)
    poly = lambda ev: B.intt(list(ev))  # noqa: E731
    wit = {"qs": [poly(e) for e in Q], "ws": [poly(e) for e in W], "rs": [poly(e) for e in R],
           "ids": [poly(e) for e in ids], "sigmas": [poly(e) for e in sig]}
    wit["w_evals"] = [B.ntt(p, n) for p in wit["ws"]]
    wit["public_inputs"] = [x0, x1]
    wit["mds"] = mds
    return wit


def rec_from_prover(B, out, acc_prev, public_inputs) -> Rec:
    """The Rec of naive_prover's result under a transcript (z, v, c canonical integers in its dicts)."""
    m = B.m
    v = out["vs"]
    vs = v[:73] + [v[73], v[-1]] + v[74:77]  # ... z, z_omega, w_omegas[0..3]
    three = [acc_prev, out["q_r"], out["q_r_omega"]]

    def acc16(a):
        return np.concatenate([np.asarray(a["C"], dtype=np.uint64).reshape(8), fe(a["z"], m), fe(a["v"], m)])

    a = out["acc"]
    return Rec(pub=np.array([fe(x, m) for x in public_inputs], dtype=np.uint64).reshape(-1, 4),
               C_ws=np.stack(out["C_ws"]).astype(np.uint64), C_z=np.asarray(out["C_z"], dtype=np.uint64),
               C_ts=np.stack(out["C_ts"]).astype(np.uint64), vs=np.stack([fe(x, m) for x in vs]),
               Ls=np.stack([np.stack(q["Ls"]) for q in three]).astype(np.uint64),
               Rs=np.stack([np.stack(q["Rs"]) for q in three]).astype(np.uint64),
               U=np.stack([np.asarray(q["U"], dtype=np.uint64) for q in three]),
               c=np.stack([fe(q["c"], m) for q in three]), prev=acc16(acc_prev), next=acc16(a),
               next_pi=(np.stack(a["Ls"]).astype(np.uint64), np.stack(a["Rs"]).astype(np.uint64),
                        np.asarray(a["U"], dtype=np.uint64), fe(a["c"], m)))


CHAINS = {"pallas_n8": ("pallas", 8), "pallas_n64": ("pallas", 64), "vesta_n16": ("vesta", 16)}  # plonk_proofs.npz


def load_chain(G, key):
    """(C_qs, [Rec, Rec]) of a chain of tests/golden/plonk_proofs.npz (tests/golden/make_plonk_proofs.py)."""
    recs = []
    for step in range(2):
        f = {name: G[f"{key}_{step}_{name}"] for name in Rec._fields if name != "next_pi"}
        recs.append(Rec(next_pi=tuple(G[f"{key}_{step}_next_pi_{name}"] for name in ("Ls", "Rs", "U", "c")), **f))
    return G[f"{key}_C_qs"], recs


def plus_one(x, m):
    return fe(to_int(x, m) + 1, m)


TAMPERINGS = {  # name -> the verdict code the reference's order gives
    "ws0": IDENTITY, "rs3": IDENTITY, "ids1": IDENTITY, "pub0": IDENTITY, "C_ws3": IDENTITY, "prev_v": INSTANCE_0,
    "r_c": INSTANCE_1, "ro_L0": INSTANCE_2, "next_C": C_BAR, "next_z": Z, "next_v": V, "next_pi_c": ACCEPT,
    "C_ts2_off": MALFORMED,
}


def tamper(rec: Rec, kind: str, m: int) -> Rec:
    """rec with one field changed."""
    def bump(a, i):
        a = a.copy()
        a[i] = plus_one(a[i], m)
        return a

    def swap(a, i, j):
        a = a.copy()
        a[i], a[j] = rec_copy(a[j]), rec_copy(a[i])
        return a

    rec_copy = np.copy
    if kind == "ws0":
        return rec._replace(vs=bump(rec.vs, V_WS))
    if kind == "rs3":
        return rec._replace(vs=bump(rec.vs, V_RS + 3))
    if kind == "ids1":
        return rec._replace(vs=bump(rec.vs, V_IDS + 1))
    if kind == "pub0":
        return rec._replace(pub=bump(rec.pub, 0))
    if kind == "C_ws3":
        return rec._replace(C_ws=swap(rec.C_ws, 3, 4))
    if kind == "prev_v":
        return rec._replace(prev=np.concatenate([rec.prev[:12], plus_one(rec.prev[12:], m)]))
    if kind == "r_c":
        return rec._replace(c=bump(rec.c, 1))
    if kind == "ro_L0":
        Ls, Rs = rec.Ls.copy(), rec.Rs.copy()
        Ls[2, 0], Rs[2, 0] = rec.Rs[2, 0], rec.Ls[2, 0]
        return rec._replace(Ls=Ls, Rs=Rs)
    if kind == "next_C":
        return rec._replace(next=np.concatenate([rec.U[0], rec.next[8:]]))
    if kind == "next_z":
        return rec._replace(next=np.concatenate([rec.next[:8], plus_one(rec.next[8:12], m), rec.next[12:]]))
    if kind == "next_v":
        return rec._replace(next=np.concatenate([rec.next[:12], plus_one(rec.next[12:], m)]))
    if kind == "next_pi_c":
        Ls, Rs, U, c = rec.next_pi
        return rec._replace(next_pi=(Ls, Rs, U, plus_one(c, m)))
    if kind == "C_ts2_off":
        C_ts = rec.C_ts.copy()
        C_ts[2, 0] ^= np.uint64(1)
        return rec._replace(C_ts=C_ts)
    raise KeyError(kind)


def prove_chain(cname, n, srs, S, H, steps=2, seed=1):
    """``steps`` proofs of satisfiable_circuit(n) on the CPU backend under the reference's transcripts, each
    accumulating the one before: (C_qs (10, 8), [Rec])."""
    B = CpuBackend(cname, srs, S, H)
    wit = satisfiable_circuit(B, n, seed, cname)
    C_qs = np.stack(B.commit_many(wit["qs"]))
    acc = B.fresh_accumulator(n - 1, seed + 100)
    recs = []
    for _ in range(steps):
        out = PR.naive_prover(B, wit, n, None, acc_prev=acc, transcript=new_transcript(cname))
        recs.append(rec_from_prover(B, out, acc, wit["public_inputs"]))
        acc = out["acc"]
    return C_qs, recs
