"""CPU model of k_acc's mixed addition with three carry chains (halo_amd/csrc/curve.hpp xyzz_madd_run,
xyzz_madd_run_aff, xyzz_run_out; the chains are fields.hpp fe_sub_k / fe_sub_k_sgn).

The running sum is (X, s Yt, ZZ, ZZZ): X as signed int32 limbs that are never normalized (|limb| < 2^30,
value in (-4p, 4p)), Yt, ZZ, ZZZ below 2p, the sign s apart.  This replays the step limb by limb for both
base fields:
  * on limb-adversarial operands (every product output at all-zero limbs, at all-ones limbs below the
    largest top limb a value under 2p can then have, and at 2p - 1; X limbs at +-(2^30 - 1) in one sign
    and alternating; Yt at its extremes; both values of m = sigma s) it asserts that every per-limb
    sum of a chain stays inside int32, that each chain's result is positive, normalized and below its
    stated bound, and that fe_mul2's product sum stays below p 2^261;
  * over random runs of 2-8 additions with random signs, Montgomery outputs placed anywhere in [0, 2p),
    it asserts equality with affine addition, sign flag included, in both stored forms (the chunk partial
    with X below 8p, the bucket sum with X below 2p), and the doubling / cancellation exits.
No GPU: this models the code, tests/test_gpu_acc_three_chains.py runs it.
"""
import itertools
import random

import pytest

import pasta as P

N, B = 9, 29
MASK = (1 << B) - 1
RP = 1 << (N * B)  # R' = 2^261
I32 = 1 << 31
CURVES = [P.PALLAS, P.VESTA]


def limbs(x):
    assert x >= 0
    return [(x >> (B * i)) & MASK for i in range(N - 1)] + [x >> (B * (N - 1))]


def value(ls):
    return sum(l << (B * i) for i, l in enumerate(ls))


def i32(x):
    assert -I32 <= x < I32, f"int32 overflow in a chain: {x / I32:.4f} x 2^31"
    return x


def chain(a, b, kp, neg=False):
    """fe_sub_k / fe_sub_k_sgn: (+-a) - b + kp with the signed carry chain; every per-limb sum in int32."""
    out, c = [], 0
    for i in range(N):
        x = i32((-a[i] if neg else a[i]) - b[i] + kp[i] + c)
        out.append(x if i == N - 1 else x & MASK)
        c = x >> B
    return out


def normalized_below(ls, bound):
    assert all(0 <= x <= MASK for x in ls[:-1]) and ls[-1] >= 0, ls
    assert 0 < value(ls) < bound, value(ls) / bound
    return ls


def sub_nc(a, b):
    return [x - y for x, y in zip(a, b)]


class Field:
    def __init__(self, p):
        self.p = p
        self.kp = {k: limbs(k * p) for k in (2, 4, 6)}
        self.rinv = pow(RP, -1, p)
        self.zero = [0] * N

    def combine(self, X, Yt, U2, S2, m_neg, peeled=False):
        """Chains 1 and 2 from the operands; returns P, Rn with their bounds asserted."""
        p = self.p
        Pd = normalized_below(chain(U2, X, self.kp[2 if peeled else 4]), (4 if peeled else 10) * p)
        Rn = normalized_below(chain(S2, Yt, self.kp[4], neg=m_neg), 6 * p)
        return Pd, Rn

    def finish(self, Rn, Yt, R2, PPP, V):
        """X3, chain 3 and the fe_mul2 sum from the products; returns X3, Tn, the sum."""
        p = self.p
        Q = sub_nc(V, PPP)
        X3 = sub_nc(sub_nc(R2, Q), V)
        assert all(abs(x) < 1 << 30 for x in X3) and -4 * p < value(X3) < 4 * p
        Tn = normalized_below(chain(X3, Q, self.kp[6]), 12 * p)
        t = value(Rn) * value(Tn) + value(Yt) * value(PPP)
        assert t < p * RP, t / (p * RP)
        return X3, Tn, t

    def run_out(self, X, Yt, sneg):
        """xyzz_run_out: X + 4p normalized in (0, 8p); Y = Yt or 2p - Yt in (0, 2p]."""
        Xs = normalized_below(chain(X, self.zero, self.kp[4]), 8 * self.p)
        Ys = chain(Yt, self.zero, self.kp[2] if sneg else self.zero, neg=sneg)
        assert all(0 <= x <= MASK for x in Ys[:-1]) and 0 <= value(Ys) <= 2 * self.p
        return Xs, Ys


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_chains_stay_in_int32_on_adversarial_limbs(curve):
    F = Field(curve.base)
    p = F.p
    # a product output's largest limbs: all ones below the largest top limb that keeps the value below 2p
    # (2^255 - 1; with the top limb of 2p itself all-ones limbs are past 2p); 2p - 1 below has that top limb
    top = (2 * p >> (B * (N - 1))) - 1
    hi = [MASK] * (N - 1) + [top]
    assert limbs(2 * p - 1)[-1] == top + 1
    assert p < value(hi) < 2 * p
    lo = [0] * N
    xm = (1 << 30) - 1
    xt = 2 * top - 2  # the largest top limb that keeps |X| < 4p beside low limbs of one sign at the maximum
    xs = [[s * xm for _ in range(N - 1)] + [s * xt] for s in (1, -1)]
    assert all(abs(value(x)) < 4 * p for x in xs)
    xs += [[(xm if (i + k) % 2 else -xm) for i in range(N - 1)] + [s * xt] for k in (0, 1) for s in (1, -1)]
    xs += [hi, lo]
    prods = (hi, lo, limbs(2 * p - 1), limbs(p), limbs(1))
    worst = 0
    for X, Yt, U2, S2, m_neg in itertools.product(xs, prods, prods, prods, (False, True)):
        Pd, Rn = F.combine(X, Yt, U2, S2, m_neg)
        if max(abs(x) for x in X) <= MASK and 0 <= value(X) < 2 * p:  # the peeled form's affine X
            F.combine(X, Yt, U2, S2, m_neg, peeled=True)
        F.run_out(X, Yt, m_neg)
    for Rn, Yt, R2, PPP, V in itertools.product((limbs(6 * p - 1), [MASK] * (N - 1) + [3 * top + 2], limbs(1)),
                                                prods, prods, prods, prods):
        X3, Tn, t = F.finish(Rn, Yt, R2, PPP, V)
        worst = max(worst, t)
        F.run_out(X3, Yt, True)
    # the stated ceiling: Rn Tn + Yt PPP < 6p 12p + 2p 2p = 76 p^2 < p 2^261 (~128 p^2)
    assert worst < 76 * p * p < p * RP


class Model:
    """The device step on Python integers, Montgomery products placed anywhere in [0, 2p)."""

    def __init__(self, curve, rng):
        self.c, self.F, self.rng = curve, Field(curve.base), rng
        self.p = curve.base
        self.one = limbs(RP % self.p)
        self.fresh, self.sneg = True, False
        self.X = self.Yt = self.ZZ = self.ZZZ = None
        self.affine = False
        self.worst = 0

    def mont(self, a, b, c=None, d=None):
        t = value(a) * value(b) + (value(c) * value(d) if c else 0)
        assert 0 <= t < self.p * RP
        return limbs(t * self.F.rinv % self.p + self.rng.choice((0, self.p)))

    def enc(self, v):
        return limbs(v * RP % self.p + self.rng.choice((0, self.p)))

    def add(self, pt, neg):
        """acc += (x2, -y2 if neg else y2); pt affine, true coordinates."""
        F = self.F
        x2, y2 = self.enc(pt[0]), self.enc(pt[1])
        if self.fresh:
            self.fresh, self.sneg, self.affine = False, neg, True
            self.X, self.Yt, self.ZZ, self.ZZZ = x2, y2, self.one, self.one
            return
        peeled, self.affine = self.affine, False
        U2 = x2 if peeled else self.mont(x2, self.ZZ)
        S2 = y2 if peeled else self.mont(y2, self.ZZZ)
        Pd, Rn = F.combine(self.X, self.Yt, U2, S2, neg != self.sneg, peeled)
        PP, R2 = self.mont(Pd, Pd), self.mont(Rn, Rn)
        PPP, V = self.mont(Pd, PP), self.mont(U2, PP)
        ZZ3 = PP if peeled else self.mont(self.ZZ, PP)
        X3, Tn, t = F.finish(Rn, self.Yt, R2, PPP, V)
        self.worst = max(self.worst, t)
        Y3 = self.mont(Rn, Tn, self.Yt, PPP)
        ZZZ3 = PPP if peeled else self.mont(self.ZZZ, PPP)
        if Pd[0] < (4 if peeled else 10) and value(ZZ3) % self.p == 0:  # q = +-acc
            self.sneg = False
            if value(Rn) % self.p == 0:  # doubling of (x2, sigma y2), s = +1
                d = P.add(self.c, pt, pt)
                if neg:
                    d = P.neg(self.c, d)
                self.X, self.Yt, self.ZZ, self.ZZZ = self.enc(d[0]), self.enc(d[1]), self.one, self.one
            else:
                self.fresh = True
            return
        assert value(Pd) % self.p != 0
        self.X, self.Yt, self.ZZ, self.ZZZ, self.sneg = X3, Y3, ZZ3, ZZZ3, not self.sneg

    def stored(self):
        """The point as both stores leave it: (affine from the chunk partial, affine from the bucket sum)."""
        if self.fresh:
            return P.INF, P.INF
        p, ri = self.p, self.F.rinv
        Xs, Ys = self.F.run_out(self.X, self.Yt, self.sneg)
        zz, zzz = value(self.ZZ) * ri % p, value(self.ZZZ) * ri % p
        assert (zz ** 3 - zzz ** 2) % p == 0
        out = []
        for xv in (value(Xs), value(Xs) % (2 * p)):  # partial_store keeps X < 8p; xyzz_settle reduces below 2p
            out.append((xv * ri * P.inv(zz, p) % p, value(Ys) * ri * P.inv(zzz, p) % p))
        return out


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_random_runs_equal_affine_addition(curve):
    rng = random.Random(11)
    G = curve.generator
    pts = [P.mul_fast(curve, rng.randrange(1, curve.scalar), G) for _ in range(24)]
    worst, ends = 0, set()
    for run in range(200):
        m = Model(curve, rng)
        exp = P.INF
        for _ in range(rng.randrange(2, 9)):
            pt, neg = rng.choice(pts), rng.random() < 0.5
            m.add(pt, neg)
            exp = P.add(curve, exp, P.neg(curve, pt) if neg else pt)
        a, b = m.stored()
        assert a == exp and b == exp, run
        ends.add((m.fresh, m.sneg))
        worst = max(worst, m.worst)
    assert {(False, False), (False, True)} <= ends  # stored with s = +1 and with s = -1
    assert worst < 76 * curve.base ** 2


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_doubling_and_cancellation_exits(curve):
    rng = random.Random(12)
    G = curve.generator
    Q = P.mul_fast(curve, 0x1234567, G)
    T = P.mul_fast(curve, 0x7654321, G)
    for seq in ([(Q, 0), (Q, 0)], [(Q, 1), (Q, 1)], [(Q, 0), (Q, 1)], [(Q, 1), (Q, 0), (T, 1)],  # peeled form
                [(T, 0), (T, 0), (T, 0)], [(Q, 0), (T, 1), (P.add(curve, Q, P.neg(curve, T)), 0), (T, 0)],
                [(Q, 1), (T, 1), (P.add(curve, Q, T), 0), (T, 1), (Q, 0)],
                [(Q, 0), (Q, 0), (P.add(curve, Q, Q), 0)], [(Q, 1), (Q, 1), (P.add(curve, Q, Q), 1), (T, 0)],
                [(Q, 0), (Q, 1), (Q, 0), (Q, 1), (Q, 1)]):
        for _ in range(4):  # the representatives in [0, 2p) vary
            m = Model(curve, rng)
            exp = P.INF
            for pt, neg in seq:
                m.add(pt, bool(neg))
                exp = P.add(curve, exp, P.neg(curve, pt) if neg else pt)
            a, b = m.stored()
            assert a == exp and b == exp, seq
