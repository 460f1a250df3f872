"""CPU model of the chunk partials stored raw (halo_amd/csrc/curve.hpp partial_store / partial_load).

k_acc stores a chunk's first and last running sums as it holds them -- X as signed int32 limbs (|limb| <
2^30, value in (-4p, 4p)), Yt, ZZ, ZZZ normalized below 2p, the sign s in bit 31 of ZZ's limb 0 -- and the
loader runs xyzz_run_out's two carry chains (X + 4p; Y = Yt or 2p - Yt) before it settles X.  Before, k_acc ran
xyzz_run_out itself and stored its result, and the loader only settled X.  This replays both limb by limb,
in the style of tests/test_acc_three_chains.py, for both base fields and asserts
  * that the 36 stored words hold X, Yt, ZZ, ZZZ unchanged and s, and that the sign bit never meets a bit of
    ZZ's limb 0 (normalized limbs, the all-ones limb included);
  * that every per-limb sum of the loader's chains stays inside int32;
  * that the loaded point equals, limb for limb, xyzz_run_out followed by the former store and load -- on
    adversarial limbs (X limbs at +-(2^30 - 1) in one sign and alternating, Yt = 1 and 2p - 1, both signs)
    and on random running sums;
  * that a settled sum (k_group_sums: X, Y < 2p, s = 0) loads as itself, and the identity (ZZ = 0) as the
    identity whatever the other words hold.
No GPU: this models the code, tests/test_gpu_raw_partials.py runs it.
"""
import itertools
import random

import pytest

import pasta as P

N, B = 9, 29
MASK = (1 << B) - 1
RP = 1 << (N * B)
I32 = 1 << 31
U32 = (1 << 32) - 1
CURVES = [P.PALLAS, P.VESTA]


def limbs(x):
    assert x >= 0
    return [(x >> (B * i)) & MASK for i in range(N - 1)] + [x >> (B * (N - 1))]


def value(ls):
    return sum(l << (B * i) for i, l in enumerate(ls))


def i32(x):
    assert -I32 <= x < I32, f"int32 overflow in a chain: {x / I32:.4f} x 2^31"
    return x


def s32(w):
    return w - (1 << 32) if w >> 31 else w


def chain(a, b, kp, neg=False):
    """fe_sub_k / xyzz_run_out's Y chain: (+-a) - b + kp, signed carries, every per-limb sum in int32."""
    out, c = [], 0
    for i in range(N):
        x = i32((-a[i] if neg else a[i]) - b[i] + kp[i] + c)
        out.append(x if i == N - 1 else x & MASK)
        c = x >> B
    return out


def cond_sub(x, kp):
    """fe_reduce_2p / the first half of fe_reduce_8p: x - kp when that is not negative."""
    t, c = [], 0
    for i in range(N):
        d = i32(x[i] - kp[i] + c)
        t.append(d & MASK)
        c = d >> B
    return t if c >= 0 else list(x)


class Field:
    def __init__(self, p):
        self.p = p
        self.kp = {k: limbs(k * p) for k in (2, 4)}
        self.zero = [0] * N

    def run_out(self, X, Yt, sneg):
        Xs = chain(X, self.zero, self.kp[4])
        assert all(0 <= x <= MASK for x in Xs[:-1]) and 0 < value(Xs) < 8 * self.p
        Ys = chain(Yt, self.zero, self.kp[2] if sneg else self.zero, neg=sneg)
        assert all(0 <= x <= MASK for x in Ys[:-1]) and 0 <= value(Ys) <= 2 * self.p
        return Xs, Ys

    def reduce_8p(self, x):
        r = cond_sub(cond_sub(x, self.kp[4]), self.kp[2])
        assert 0 <= value(r) < 2 * self.p
        return r

    # the former format: xyzz_run_out in k_acc, 36 plain words, the loader settles X
    def old_store_load(self, X, Yt, ZZ, ZZZ, sneg):
        Xs, Ys = self.run_out(X, Yt, sneg)
        words = [w & U32 for w in Xs + Ys + ZZ + ZZZ]
        Xl, Yl, ZZl, ZZZl = (words[k * N:(k + 1) * N] for k in range(4))
        return self.reduce_8p(Xl), Yl, ZZl, ZZZl

    # the raw format
    def store(self, X, Yt, ZZ, ZZZ, sneg):
        words = [w & U32 for w in X + Yt + ZZ + ZZZ]
        assert words[2 * N] >> 29 == 0, "ZZ's limb 0 reaches the sign bit"
        words[2 * N] |= (U32 if sneg else 0) & 0x80000000
        assert len(words) == 36
        return words

    def load(self, words):
        X = [s32(w) for w in words[:N]]
        Yt, ZZ, ZZZ = (list(words[k * N:(k + 1) * N]) for k in (1, 2, 3))
        sneg = bool(ZZ[0] >> 31)
        ZZ[0] &= 0x7FFFFFFF
        Xs, Ys = self.run_out(X, Yt, sneg)
        return self.reduce_8p(Xs), Ys, ZZ, ZZZ


def adversarial(F):
    p = F.p
    top = (2 * p >> (B * (N - 1))) - 1
    hi = [MASK] * (N - 1) + [top]  # all-ones limbs below 2p
    xm = (1 << 30) - 1
    xt = 2 * top - 2
    xs = [[s * xm for _ in range(N - 1)] + [s * xt] for s in (1, -1)]
    xs += [[(xm if (i + k) % 2 else -xm) for i in range(N - 1)] + [s * xt] for k in (0, 1) for s in (1, -1)]
    assert all(abs(value(x)) < 4 * p for x in xs)
    xs += [hi, [0] * N, limbs(2 * p - 1), limbs(1)]
    ys = [limbs(1), limbs(2 * p - 1), hi, limbs(p)]
    zs = [hi, limbs(1), limbs(2 * p - 1), [MASK] + [0] * (N - 1)]
    return xs, ys, zs


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_raw_partial_loads_as_the_settled_one(curve):
    F = Field(curve.base)
    xs, ys, zs = adversarial(F)
    for X, Yt, ZZ, sneg in itertools.product(xs, ys, zs, (False, True)):
        ZZZ = zs[0]
        words = F.store(X, Yt, ZZ, ZZZ, sneg)
        # the stored words: the four coordinates as they stand, and s
        assert [s32(w) for w in words[:N]] == X and words[N:2 * N] == Yt and words[3 * N:] == ZZZ
        assert words[2 * N] & 0x7FFFFFFF == ZZ[0] and words[2 * N + 1:3 * N] == ZZ[1:]
        assert bool(words[2 * N] >> 31) == sneg
        assert F.load(words) == F.old_store_load(X, Yt, ZZ, ZZZ, sneg)
    rng = random.Random(21)
    p = F.p
    for _ in range(2000):
        # a running X as xyzz_madd_run leaves it: R2 + PPP - 2V limb-wise, products anywhere in [0, 2p)
        r2, ppp, v = (limbs(rng.randrange(2 * p)) for _ in range(3))
        X = [a + b - 2 * c for a, b, c in zip(r2, ppp, v)]
        Yt, ZZ, ZZZ = (limbs(rng.randrange(1, 2 * p)) for _ in range(3))
        sneg = rng.random() < 0.5
        got = F.load(F.store(X, Yt, ZZ, ZZZ, sneg))
        assert got == F.old_store_load(X, Yt, ZZ, ZZZ, sneg)
        assert (value(got[0]) - value(X)) % p == 0 and (value(got[1]) - (-1 if sneg else 1) * value(Yt)) % p == 0


@pytest.mark.parametrize("curve", CURVES, ids=lambda c: c.name)
def test_settled_sum_and_identity(curve):
    F = Field(curve.base)
    p = F.p
    rng = random.Random(22)
    _, ys, zs = adversarial(F)
    settled = [(limbs(rng.randrange(2 * p)), limbs(rng.randrange(2 * p))) for _ in range(200)]
    settled += [(x, y) for x in (limbs(0), limbs(2 * p - 1), zs[0]) for y in ys]
    for X, Y in settled:  # k_group_sums: X, Y < 2p, s = 0 -> unchanged
        ZZ, ZZZ = limbs(rng.randrange(1, 2 * p)), limbs(rng.randrange(1, 2 * p))
        assert F.load(F.store(X, Y, ZZ, ZZZ, False)) == (X, Y, ZZ, ZZZ)
    one = limbs(RP % p)
    zero = [0] * N
    # xyzz_id (the fresh state, a cancelled segment) with either sign word, and ZZ = 0 beside any running X, Yt
    for X, Y, sneg in [(one, one, False), (one, one, True), ([(1 << 30) - 1] * (N - 1) + [5], limbs(2 * p - 1), True),
                       ([-(1 << 30) + 1] * (N - 1) + [-5], limbs(1), False)]:
        got = F.load(F.store(X, Y, zero, zero, sneg))
        assert got[2] == zero and got[3] == zero  # xyzz_is_id: ZZ = 0, the sign bit stripped
        assert all(0 <= x <= MASK for x in got[0][:-1] + got[1][:-1])
