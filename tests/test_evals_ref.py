"""CPU tests of tests/evals_ref.py, the big-integer reference that tests/test_gpu_evals.py holds the evals kernels
against: each operation is checked by an identity that its own code does not use."""
import random

import numpy as np
import pytest

import evals_ref as E
import pasta as P

MODS = [P.FP_MODULUS, P.FQ_MODULUS]


@pytest.mark.parametrize("m", MODS)
def test_edge_values_and_words(m):
    e = E.EDGE(m)
    assert len(e) == 34 and all(W < m for W in e)
    assert E.unark([P.R_MONT % m, m - P.R_MONT % m], m) == [1, m - 1]  # the values one and minus one
    rng = random.Random(1)
    xs = E.full_range(rng, 50, m) + e
    assert max(xs) >= 1 << 254  # the draw reaches above 2^252
    a = E.to_array(xs)
    assert a.shape == (len(xs), 4) and a.dtype == np.uint64
    assert [P.limbs_to_int(r) for r in a] == xs and E.from_array(a) == xs
    assert a.tolist() == [P.int_to_limbs(x) for x in xs]
    assert E.unark(xs, m) == [P.from_mont(x, m) for x in xs] and E.ark(E.unark(xs, m), m) == xs


@pytest.mark.parametrize("m", MODS)
def test_evals_op_inverse_pairs(m):
    rng = random.Random(2)
    a, b = E.full_range(rng, 40, m), E.full_range(rng, 40, m)
    s = rng.randrange(1, m)
    assert E.evals_op(E.EV_SUB, E.evals_op(E.EV_ADD, a, b, None, 0, m), b, None, 0, m) == a
    assert E.evals_op(E.EV_SUB_SCALAR, E.evals_op(E.EV_ADD_SCALAR, a, None, s, 0, m), None, s, 0, m) == a
    assert E.evals_op(E.EV_SCALE, E.evals_op(E.EV_SCALE, a, None, s, 0, m), None, P.inv(s, m), 0, m) == a
    ab = E.evals_op(E.EV_MUL, a, b, None, 0, m)
    assert all(x * P.inv(y, m) % m == z for x, y, z in zip(ab, b, a))
    # x^e by repeated multiplication, and the exponent laws at the 32-bit ends
    x7 = a
    for _ in range(6):
        x7 = E.evals_op(E.EV_MUL, x7, a, None, 0, m)
    assert E.evals_op(E.EV_POW, a, None, None, 7, m) == x7
    hi = E.evals_op(E.EV_POW, a, None, None, 0x80000000, m)
    lo = E.evals_op(E.EV_POW, a, None, None, 0x7FFFFFFF, m)
    assert E.evals_op(E.EV_MUL, hi, lo, None, 0, m) == E.evals_op(E.EV_POW, a, None, None, 0xFFFFFFFF, m)
    assert E.evals_op(E.EV_POW, [0, 1, m - 1], None, None, 0, m) == [1, 1, 1]
    assert E.evals_op(E.EV_POW, [0, 1, m - 1], None, None, 0xFFFFFFFF, m) == [0, 1, m - 1]


@pytest.mark.parametrize("m", MODS)
@pytest.mark.parametrize("ln,n", [(1, 1), (7, 1), (5, 5), (6, 5), (129, 64), (300, 3), (600, 512)])
def test_division_identity_at_a_point(m, ln, n):
    """c(z) == q(z) (z^n - 1) + r(z) at a random z, with the stated lengths."""
    rng = random.Random(ln * 1000 + n)
    c = E.full_range(rng, ln, m)
    q, r = E.div_vanishing(c, n, m)
    assert len(q) == ln - n and len(r) == n
    z = rng.randrange(m)
    assert P.horner(c, z, m) == (P.horner(q, z, m) * (pow(z, n, m) - 1) + P.horner(r, z, m)) % m


@pytest.mark.parametrize("m", MODS)
@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_scan_prefix_times_suffix_is_the_total(m, n):
    rng = random.Random(n)
    xs = E.full_range(rng, n, m)
    pre, suf = E.scan(xs, 0, m), E.scan(xs, 1, m)
    total = pre[-1]
    assert suf[0] == total
    for i in range(n - 1):
        assert pre[i] * suf[i + 1] % m == total
    # the Montgomery-domain form gives the same values
    words = E.ark(xs, m)
    assert E.scan_words(words, 0, m) == E.ark(pre, m) and E.scan_words(words, 1, m) == E.ark(suf, m)
    if n > 2:  # a zero: everything on the far side is zero, the near side untouched
        ys = xs[:]
        ys[2] = 0
        assert E.scan(ys, 0, m) == pre[:2] + [0] * (n - 2) and E.scan(ys, 1, m) == [0] * 3 + suf[3:]


@pytest.mark.parametrize("m", MODS)
@pytest.mark.parametrize("zeta_kind", ["zero", "one", "minus_one", "random"])
def test_lincomb_is_horner_of_the_columns(m, zeta_kind):
    rng = random.Random(3)
    zeta = {"zero": 0, "one": 1, "minus_one": m - 1, "random": rng.randrange(m)}[zeta_kind]
    polys = [E.full_range(rng, ln, m) for ln in (5, 0, 9, 1, 7)]
    n_out = 12
    got = E.lincomb(polys, zeta, n_out, m)
    for e in range(n_out):
        column = [p[e] if e < len(p) else 0 for p in polys]
        assert got[e] == P.horner(column, zeta, m)
    assert E.lincomb([], zeta, 3, m) == [0, 0, 0]


@pytest.mark.parametrize("m", MODS)
def test_gate_reference_is_linear_in_each_selector_and_in_pi(m):
    rng = random.Random(4)
    N, shift = 8, 3
    vec = lambda: E.full_range(rng, N, m)
    w, r, q, pi = [vec() for _ in range(16)], [vec() for _ in range(15)], [vec() for _ in range(10)], vec()
    mds = [E.full_range(rng, 3, m) for _ in range(3)]
    zero = [0] * N
    base = E.gate_constraints(w, r, q, pi, mds, shift, m)
    # f_gc = sum_k (f_gc with only q_k) + (f_gc with only pi)
    parts = [E.gate_constraints(w, r, [q[j] if j == k else zero for j in range(10)], zero, mds, shift, m)
             for k in range(10)]
    parts.append(E.gate_constraints(w, r, [zero] * 10, pi, mds, shift, m))
    assert parts[-1] == pi and parts[4] == q[4]
    assert [sum(col) % m for col in zip(*parts)] == base
    # and homogeneous: scaling q_k by c scales its part by c
    c = rng.randrange(2, m)
    for k in range(10):
        qs = [[c * x % m for x in q[j]] if j == k else zero for j in range(10)]
        assert E.gate_constraints(w, r, qs, zero, mds, shift, m) == [c * x % m for x in parts[k]]
    # the shifted witness wraps: with shift = N the element is its own successor
    assert E.gate_constraints(w, r, q, pi, mds, N, m) == E.gate_constraints(w, r, q, pi, mds, 0, m)
    assert E.gate_constraints(w, r, q, pi, mds, 1, m) != E.gate_constraints(w, r, q, pi, mds, 0, m)
