"""Plain big-integer reference of the prover's elementwise kernels (halo_amd/csrc/evals.hip): the seven Evals ops
(poly.rs:90-327), the division by X^n - 1 (DensePolynomial::divide_by_vanishing_poly), the running product
(protocol.rs:143-154), the geometric combination (protocol.rs:542-548) and the gate-constraint evaluation of round 4
(protocol.rs:170-191).  Every function works on canonical integers mod m; the ark-word helpers at the end carry them
to and from the 4 x u64 Montgomery words (R = 2^256) that the library reads and writes.

The gate reference feeds an integer-mod-m value class through the ``*_generic`` transcriptions of halo_amd/prover.py
and sums them as naive_prover's round 4 does on the backends without the fused kernels: the formulas are not typed
again here.  tests/test_evals_ref.py holds this file against identities it does not use itself.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), os.path.join(os.path.dirname(_HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pasta as P  # noqa: E402
from halo_amd import prover as PR  # noqa: E402

FIELDS = [("fp", 0), ("fq", 1)]
EV_ADD, EV_SUB, EV_MUL, EV_SCALE, EV_ADD_SCALAR, EV_SUB_SCALAR, EV_POW = range(7)


# ---------------------------------------------------------------------------------------------
# the operations, on canonical integers
# ---------------------------------------------------------------------------------------------
def evals_op(op, a, b, s, e, m):
    """out[i] of halo_evals_op; pow(x, e, m) gives 0^0 = 1 as ark's pow does."""
    if op == EV_ADD:
        return [(x + y) % m for x, y in zip(a, b)]
    if op == EV_SUB:
        return [(x - y) % m for x, y in zip(a, b)]
    if op == EV_MUL:
        return [x * y % m for x, y in zip(a, b)]
    if op == EV_SCALE:
        return [x * s % m for x in a]
    if op == EV_ADD_SCALAR:
        return [(x + s) % m for x in a]
    if op == EV_SUB_SCALAR:
        return [(x - s) % m for x in a]
    if op == EV_POW:
        return [pow(x, e, m) for x in a]
    raise ValueError(op)


def div_vanishing(c, n, m):
    """c = q (X^n - 1) + r by long division from the top coefficient down: the untrimmed quotient (len - n entries)
    and remainder (n entries).  len(c) >= n."""
    rem = list(c)
    q = [0] * (len(c) - n)
    for i in range(len(c) - 1, n - 1, -1):
        q[i - n] = rem[i]
        rem[i - n] = (rem[i - n] + rem[i]) % m
        rem[i] = 0
    return q, rem[:n]


def scan(xs, reverse, m):
    """The sequential running product: out[i] = prod_{j <= i} xs[j] (reverse: prod_{j >= i})."""
    out = [0] * len(xs)
    acc = 1
    for i in (range(len(xs) - 1, -1, -1) if reverse else range(len(xs))):
        acc = acc * xs[i] % m
        out[i] = acc
    return out


def lincomb(polys, zeta, n_out, m):
    """sum_i zeta^i polys[i] over n_out coefficients, missing coefficients zero (zeta^0 = 1 also for zeta = 0)."""
    out = [0] * n_out
    for i, p in enumerate(polys):
        zi = pow(zeta, i, m)
        for e, c in enumerate(p):
            out[e] = (out[e] + zi * c) % m
    return out


class Val:
    """An integer mod m with + - *, for the ``*_generic`` forms."""

    __slots__ = ("v", "m")

    def __init__(self, v, m):
        self.v, self.m = v % m, m

    def _of(self, o):
        return o.v if isinstance(o, Val) else int(o)

    def __add__(self, o):
        return Val(self.v + self._of(o), self.m)

    __radd__ = __add__

    def __sub__(self, o):
        return Val(self.v - self._of(o), self.m)

    def __rsub__(self, o):
        return Val(self._of(o) - self.v, self.m)

    def __mul__(self, o):
        return Val(self.v * self._of(o), self.m)

    __rmul__ = __mul__


def gate_constraints(w, r, q, pi, mds, shift, m):
    """f_gc[i] of protocol.rs:179-190 for every i < N: w (16), r (15), q (10) and pi are vectors of N canonical
    integers, mds the 3 x 3 matrix, and the shifted witness of element i is nw[k] = w[k][(i + shift) % N]."""
    N = len(pi)
    M = [[Val(x, m) for x in row] for row in mds]
    one = Val(1, m)
    out = []
    for i in range(N):
        j = (i + shift) % N
        wi = [Val(c[i], m) for c in w]
        nw = [Val(w[k][j], m) for k in range(3)]
        ri = [Val(c[i], m) for c in r]
        qi = [Val(c[i], m) for c in q]
        poseidon = PR.poseidon_constraints(M, ri, wi, nw, lambda x: Val(pow(x.v, 7, m), m))
        affine_add = PR.affine_add_constraints(wi, one)
        affine_mul = PR.affine_mul_constraints(wi, nw, ri[0], one)
        eq = PR.eq_constraints(wi)
        range_check = PR.range_check_constraints(wi, nw, ri)
        # the f_gc sum of naive_prover round 4 (the non-fused branch)
        f = (wi[0] * qi[0] + qi[1] * wi[1] + qi[2] * wi[2] + qi[3] * wi[0] * wi[1] + qi[4] + qi[5] * poseidon
             + qi[6] * affine_add + qi[7] * affine_mul + qi[8] * eq + qi[9] * range_check + Val(pi[i], m))
        out.append(f.v)
    return out


# ---------------------------------------------------------------------------------------------
# ark words: W = v 2^256 mod m, as Python integers and as (n, 4) uint64 arrays
# ---------------------------------------------------------------------------------------------
_RINV = {}


def rinv(m):
    if m not in _RINV:
        _RINV[m] = pow(P.R_MONT, -1, m)
    return _RINV[m]


def ark(vals, m):
    """canonical values -> ark words (integers)"""
    return [P.to_mont(v % m, m) for v in vals]


def unark(words, m):
    """ark words (integers) -> canonical values; P.from_mont with the inverse of R formed once"""
    ri = rinv(m)
    return [W * ri % m for W in words]


def to_array(words):
    """integers < 2^256 -> (n, 4) uint64 little-endian limbs (P.int_to_limbs for each, in one buffer)"""
    buf = b"".join(W.to_bytes(32, "little") for W in words)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def from_array(a):
    """(n, 4) uint64 -> integers (P.limbs_to_int for each row)"""
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def scan_words(words, reverse, m):
    """scan() on ark words without leaving the Montgomery domain: acc <- acc W / R, one product and one reduction per
    element (what a long input needs: half a million from_mont / to_mont calls are not made)."""
    ri = rinv(m)
    out = [0] * len(words)
    acc = P.R_MONT % m
    for i in (range(len(words) - 1, -1, -1) if reverse else range(len(words))):
        acc = acc * words[i] * ri % m
        out[i] = acc
    return out


def EDGE(m):
    """The edge values, as ark WORDS W (the canonical value of an entry is from_mont(W)): around 0 and p, the top of
    the word range, one and minus one, the middle of the field, and every boundary of the 29-bit limbs the kernels
    repack the words into and of the 64-bit words themselves."""
    one = P.R_MONT % m
    e = [0, 1, 2, m - 1, m - 2, 1 << 254, (1 << 254) - 1, 1 << 252, one, m - one, (m - 1) // 2, (m + 1) // 2]
    for k in range(1, 9):
        e += [1 << (29 * k), (1 << (29 * k)) - 1]
    for k in range(1, 4):
        e += [1 << (64 * k), (1 << (64 * k)) - 1]
    assert all(0 <= W < m for W in e) and len(set(e)) == len(e)
    return e


def full_range(rng: random.Random, n, m):
    """n ark words uniform in [0, m) (not [0, 2^252))"""
    return [rng.randrange(m) for _ in range(n)]
