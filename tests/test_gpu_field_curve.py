"""GPU parity: field and curve (a2) arithmetic through the C ABI vs the oracle."""
import random

import numpy as np
import pytest

import pasta as P
import test_field_bounds as TB  # the Python restatement of glv::decompose and the parsed GLV constants

pytestmark = pytest.mark.gpu

OPS = {
    0: lambda x, y, m: x * y % m,
    1: lambda x, y, m: (x + y) % m,
    2: lambda x, y, m: (x - y) % m,
    3: lambda x, y, m: x * x % m,
    4: lambda x, y, m: pow(x, -1, m) if x else 0,
    5: lambda x, y, m: (-x) % m,
}


def fe(vals, m):
    return np.array([P.int_to_limbs(P.to_mont(v % m, m)) for v in vals], dtype=np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("fname,fid", [("fp", 0), ("fq", 1)])
def test_field_ops(hal, fname, fid):
    m = P.FIELDS[fname]
    rng = random.Random(fid)
    n = 2000
    a = [rng.randrange(m) for _ in range(n)]
    b = [rng.randrange(m) for _ in range(n)]
    # edge values: 0, 1, p-1, 2^k boundaries of the 29-bit limbs, values just below p
    edge = [0, 1, m - 1, m - 2, (1 << 29) - 1, 1 << 29, (1 << 232) - 1, 1 << 232, (1 << 254) - 1, m >> 1]
    a[: len(edge)] = edge
    b[: len(edge)] = edge[::-1]
    A, B = fe(a, m), fe(b, m)
    L = hal.load()
    for op, fn in OPS.items():
        out = np.zeros_like(A)
        hal.check(L.halo_field_op(fid, op, hal.ptr(A), hal.ptr(B), n, hal.ptr(out)))
        assert np.array_equal(out, fe([fn(x, y, m) for x, y in zip(a, b)], m)), f"op {op}"


@pytest.mark.parametrize("cname,cid", [("pallas", 0), ("vesta", 1)])
def test_curve_ops(hal, corc, cname, cid):
    c = P.CURVES[cname]
    n = 96
    g = corc.srs_generate(cname, 400)
    A = np.ascontiguousarray(g[:n])
    B = np.ascontiguousarray(g[200:200 + n])
    B[5] = A[5]                                   # P + P -> doubling branch
    B[6] = 0                                      # P + O
    A[8] = 0                                      # O + Q
    B[7] = P.point_to_wrapped(c, P.neg(c, P.wrapped_to_point(c, list(A[7]))))  # P + (-P) = O
    L = hal.load()
    out = np.zeros_like(A)
    pa = [P.wrapped_to_point(c, list(x)) for x in A]
    pb = [P.wrapped_to_point(c, list(x)) for x in B]
    hal.check(L.halo_curve_op(cid, 0, hal.ptr(A), hal.ptr(B), None, n, hal.ptr(out)))
    assert np.array_equal(out, np.array([P.point_to_wrapped(c, P.add(c, x, y)) for x, y in zip(pa, pb)], dtype=np.uint64))
    hal.check(L.halo_curve_op(cid, 1, hal.ptr(A), None, None, n, hal.ptr(out)))
    assert np.array_equal(out, np.array([P.point_to_wrapped(c, P.add(c, x, x)) for x in pa], dtype=np.uint64))
    rng = random.Random(4)
    ks = [rng.randrange(c.scalar) for _ in range(n)]
    ks[0], ks[1], ks[2] = 0, 1, c.scalar - 1
    K = fe(ks, c.scalar)
    hal.check(L.halo_curve_op(cid, 2, hal.ptr(A), None, hal.ptr(K), n, hal.ptr(out)))
    assert np.array_equal(out, np.array([P.point_to_wrapped(c, P.mul_fast(c, k, x)) for k, x in zip(ks, pa)],
                                        dtype=np.uint64))


# ---------------------------------------------------------------------------------------------
# op 2 (scalar_mul_glv_quad): scalars built from chosen GLV halves, plain edge scalars, ragged batches
# ---------------------------------------------------------------------------------------------
GLV_CFG = {"pallas": "PallasCurveCfg", "vesta": "VestaCurveCfg"}
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _win(d, w):
    return d << (4 * w)


# magnitudes of one half as 4-bit windows (the kernel's joint fixed window), all below 2^125
HALVES = {
    "one": 1,
    "w0_9": _win(9, 0),
    "w0_15": _win(15, 0),
    "w15_9": _win(9, 15),          # the top window of a 32-bit word
    "w16_15": _win(15, 16),        # the bottom window of the next word
    "w31_1": _win(1, 31),          # window 31 (bit 124)
    "all15_below_31": (1 << 124) - 1,
    "all15_and_w31": (1 << 125) - 1,
    "all_ones": int("1" * 32, 16),
    "alt_0f": int("0f" * 16, 16),
    "alt_f0": int("f0" * 15, 16),
    "low_abc": 0xABC,              # leading zero windows from window 3 up
    "u64_max": (1 << 64) - 1,      # leading zero windows from window 16 up
}
# pairs of different halves: leading zero windows in one half only, dense against sparse
CROSS = [("low_abc", "all_ones"), ("all_ones", "low_abc"), ("w0_9", "all15_and_w31"), ("all15_and_w31", "w0_9"),
         ("w31_1", "alt_0f"), ("alt_0f", "w31_1"), ("w15_9", "all15_below_31"), ("all15_below_31", "w15_9"),
         ("u64_max", "all_ones"), ("all_ones", "u64_max"), ("alt_0f", "alt_f0"), ("all15_and_w31", "all15_below_31")]


def glv_directed_scalars(cname):
    """[(name, k)] with k = k1 + lambda k2 (mod r) for chosen signed halves; each is asserted to decompose
    back to (k1, k2) under the restatement of glv::decompose, so the kernel meets exactly these halves."""
    cfg = TB._glv_consts()[GLV_CFG[cname]]
    r = P.CURVES[cname].scalar
    lam = TB.glv_lambda(cfg, r)
    assert pow(lam, 3, r) == 1 and lam != 1
    pairs = []
    for name, h in HALVES.items():
        pairs += [(name + ",0", h, 0), ("0," + name, 0, h), (name + "," + name, h, h)]
    pairs += [(a + "," + b, HALVES[a], HALVES[b]) for a, b in CROSS]
    out = {}
    for name, a, b in pairs:
        for s1 in (1, -1):
            for s2 in (1, -1):
                k1, k2 = s1 * a, s2 * b
                assert abs(k1) < 1 << 125 and abs(k2) < 1 << 125
                k = (k1 + lam * k2) % r
                assert TB.glv_decompose(cfg, k) == (k1, k2), (cname, name, s1, s2)
                out.setdefault(k, f"{name} signs {s1:+d} {s2:+d}")
    return [(v, k) for k, v in out.items()], lam


def plain_scalars(r, lam):
    ks = [0, 1, 2, 15, 16, 17, r - 1, r - 2, lam, lam + 1, lam - 1, r - lam, (r - 1) // 2, (r + 1) // 2]
    for k in (127, 128, 129, 253, 254):
        ks += [1 << k, (1 << k) - 1]
    assert all(0 <= k < r for k in ks)
    return [(f"plain {k:#x}", k) for k in ks]


def _curve_op2(hal, cid, A, K, n):
    """op 2 over the first n rows.  The row after the n-th output belongs to the host buffer only: it shows
    that the call copies back n rows and no more, not what the kernel stores on the device."""
    out = np.full((n + 1, 8), SENTINEL, dtype=np.uint64)
    hal.check(hal.load().halo_curve_op(cid, 2, hal.ptr(np.ascontiguousarray(A[:n])), None,
                                       hal.ptr(np.ascontiguousarray(K[:n])), n, hal.ptr(out)))
    assert (out[n] == SENTINEL).all(), f"op 2, n = {n}: the call copied back more than n rows"
    return out[:n]


@pytest.mark.parametrize("cname,cid", [("pallas", 0), ("vesta", 1)])
def test_curve_scalar_mul_directed_and_ragged(hal, corc, cname, cid):
    c = P.CURVES[cname]
    r = c.scalar
    directed, lam = glv_directed_scalars(cname)
    plain = plain_scalars(r, lam)
    rng = random.Random(40 + cid)
    rand = [(f"random {i}", rng.randrange(r)) for i in range(300)]
    g = corc.srs_generate(cname, 2)
    bases = [g[0], g[1], np.zeros(8, dtype=np.uint64)]  # two points and the identity
    pts = [P.wrapped_to_point(c, list(b)) for b in bases]
    # every scalar on base 0, the directed and plain ones on base 1 too, every eighth on the identity
    rows = [(0, name, k) for name, k in directed + plain + rand]
    rows += [(1, name, k) for name, k in directed + plain]
    rows += [(2, name, k) for name, k in (directed + plain)[::8]]
    assert sum(1 for b, _, _ in rows if b != 2) <= 1500  # the oracle's multiplications, ~1.3 ms each
    n = len(rows)
    A = np.ascontiguousarray(np.stack([bases[b] for b, _, _ in rows]))
    K = fe([k for _, _, k in rows], r)
    exp = np.array([P.point_to_wrapped(c, P.mul_fast(c, k, pts[b])) for b, _, k in rows], dtype=np.uint64)
    got = _curve_op2(hal, cid, A, K, n)
    bad = [(rows[i][0], rows[i][1]) for i in range(n) if not np.array_equal(got[i], exp[i])]
    assert not bad, bad[:10]
    # ragged batches (8 quads per block, the last quads without a row): rows spread over the whole list,
    # every output right
    pick = list(range(0, n, n // 13))[:13]
    A13, K13 = np.ascontiguousarray(A[pick]), np.ascontiguousarray(K[pick])
    assert sum(1 for i in pick if rows[i][0] != 2) >= 11
    for m in (1, 7, 8, 9, 13):
        assert np.array_equal(_curve_op2(hal, cid, A13, K13, m), exp[pick[:m]]), f"n = {m}"


@pytest.mark.parametrize("cname,cid", [("pallas", 0), ("vesta", 1)])
def test_curve_add_dbl_ragged(hal, corc, cname, cid):
    """ops 0 and 1 (one lane per row, 64 per block) at n = 1, 63, 64, 65, the exceptional rows included
    at the block edges.  The sentinel row after the n-th output is host memory: it checks the size of the
    copy back, not the kernel's stores."""
    c = P.CURVES[cname]
    g = corc.srs_generate(cname, 130)
    L = hal.load()
    for n in (1, 63, 64, 65):
        A = np.ascontiguousarray(g[:n])
        B = np.ascontiguousarray(g[65:65 + n])
        B[n - 1] = A[n - 1]                        # the last row doubles
        if n > 1:
            B[0] = P.point_to_wrapped(c, P.neg(c, P.wrapped_to_point(c, list(A[0]))))  # P + (-P) = O
            A[n - 2] = 0                           # O + Q
            B[n // 2] = 0                          # P + O
        pa = [P.wrapped_to_point(c, list(x)) for x in A]
        pb = [P.wrapped_to_point(c, list(x)) for x in B]
        out = np.full((n + 1, 8), SENTINEL, dtype=np.uint64)
        hal.check(L.halo_curve_op(cid, 0, hal.ptr(A), hal.ptr(B), None, n, hal.ptr(out)))
        assert np.array_equal(out[:n], np.array([P.point_to_wrapped(c, P.add(c, x, y)) for x, y in zip(pa, pb)],
                                                dtype=np.uint64)), n
        assert (out[n] == SENTINEL).all(), n
        out = np.full((n + 1, 8), SENTINEL, dtype=np.uint64)
        hal.check(L.halo_curve_op(cid, 1, hal.ptr(A), None, None, n, hal.ptr(out)))
        assert np.array_equal(out[:n], np.array([P.point_to_wrapped(c, P.add(c, x, x)) for x in pa], dtype=np.uint64)), n
        assert (out[n] == SENTINEL).all(), n


# ---------------------------------------------------------------------------------------------
# field edges: every pairing of an edge set for ops 0-5, and fe_inv on structured inputs
#
# A value x travels through k_field_op in three representations: the ark words hold x 2^256 mod p, fe_load
# splits those words into 29-bit limbs, and fe_from_ark's multiplication turns them into the internal
# Montgomery form, whose integer is x 2^261 mod p.  A bit pattern X chosen here therefore appears literally
# in none of them unless x is scaled: x = X 2^-256 puts X into the ark words (and the limbs fe_load makes
# of them), x = X 2^-261 makes X the integer of the internal form -- the one fe_add / fe_sub / fe_neg carry
# and fe_inv's binary GCD starts from.  Each pattern is fed at all three scales.
# ---------------------------------------------------------------------------------------------
SCALES = {"value": 0, "ark words": 256, "internal integer": 261}


def scaled(X, shift, m):
    """The field element x whose representation scaled by 2^shift is the integer X: x = X 2^-shift mod p."""
    return X * pow(1 << shift, -1, m) % m


def field_edge_set(m):
    s = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, (1 << 254) - 1]
    for j in range(1, 9):    # the boundaries of the nine 29-bit limbs (once scaled, see above)
        s += [(1 << (29 * j)) - 1, (1 << (29 * j)) + 1]
    for j in range(1, 8):    # the boundaries of the 32-bit words
        s += [(1 << (32 * j)) - 1, (1 << (32 * j)) + 1]
    assert len(set(s)) == len(s) == 38 and all(0 <= x < m for x in s)
    return s


def _field_op(hal, fid, op, A, B):
    """One halo_field_op call.  The row after the n-th output belongs to the host buffer only: it shows
    that the call copies back n rows and no more, not what the kernel stores on the device."""
    out = np.full((len(A) + 1, 4), SENTINEL, dtype=np.uint64)
    hal.check(hal.load().halo_field_op(fid, op, hal.ptr(A), hal.ptr(B) if B is not None else None, len(A), hal.ptr(out)))
    assert (out[len(A)] == SENTINEL).all(), "halo_field_op copied back more than n rows"
    return out[: len(A)]


@pytest.mark.parametrize("fname,fid", [("fp", 0), ("fq", 1)])
def test_field_ops_edge_cross_product(hal, fname, fid):
    """Every pairing of the edge patterns, and the pairs whose patterns add up to p - 1, p and p + 1, with
    the patterns as values, as ark words and as internal integers (the sums then hold in that integer)."""
    m = P.FIELDS[fname]
    s = field_edge_set(m)
    patterns = [(x, y) for x in s for y in s]                              # a = b on the diagonal
    patterns += [(x, (t - x) % m) for x in s for t in (m - 1, m, m + 1)]   # a + b = p - 1, p, p + 1
    pairs = [(scaled(x, sh, m), scaled(y, sh, m)) for sh in SCALES.values() for x, y in patterns]
    # the scaling is what it claims: the ark words / the internal integer of x are the pattern X
    X = s[9]
    assert P.to_mont(scaled(X, 256, m), m) == X and P.to_mont(scaled(X, 261, m), m) * 32 % m == X
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    A, B = fe(a, m), fe(b, m)
    for op, fn in OPS.items():
        got = _field_op(hal, fid, op, A, B)
        exp = fe([fn(x, y, m) for x, y in pairs], m)
        bad = [(hex(a[i]), hex(b[i])) for i in range(len(pairs)) if not np.array_equal(got[i], exp[i])]
        assert not bad, (op, bad[:5])


@pytest.mark.parametrize("fname,fid", [("fp", 0), ("fq", 1)])
def test_field_inverse_structured_inputs(hal, fname, fid):
    """fe_inv's binary GCD starts from the integer X of the internal form, X = x 2^261 mod p, and is steered
    by the bit lengths of its operands and by 62-bit approximations of them.  The structured integers --
    powers of two and their neighbours, p - 2^k, everything below 64, values of 61-63 bits, and p minus each
    of them -- are therefore fed as x = X 2^-261 mod p, so that the GCD meets X itself; the same integers
    are also fed literally (there the GCD sees x 2^261 mod p, an unstructured value) together with 2000
    random values.  Every inverse is checked against pow(x, -1, p) and through x x^-1 = 1 (op 0)."""
    m = P.FIELDS[fname]
    rng = random.Random(100 + fid)
    st = []
    for k in range(255):
        st += [1 << k, (1 << k) - 1, m - (1 << k)]
    st += list(range(64))
    for bits in (61, 62, 63):
        st += [1 << (bits - 1), (1 << bits) - 1, (1 << (bits - 1)) + 1, (1 << bits) - 2]
        st += [rng.randrange(1 << (bits - 1), 1 << bits) for _ in range(8)]
    assert all(0 <= x < m for x in st)
    st += [(-x) % m for x in st]
    xs = [scaled(X, 261, m) for X in st]      # the GCD starts from X
    assert all(P.to_mont(x, m) * 32 % m == X for x, X in zip(xs[:800:7], st[:800:7]))  # ark words X 2^-5
    xs += st                                  # the literal values
    xs += [rng.randrange(m) for _ in range(2000)]
    X = fe(xs, m)
    assert (X[-2000:, :3].max(axis=0) >> np.uint64(63)).all()  # all 64 bits of the random words in play
    inv = _field_op(hal, fid, 4, X, None)
    exp = fe([pow(x, -1, m) if x else 0 for x in xs], m)
    bad = [hex(xs[i]) for i in range(len(xs)) if not np.array_equal(inv[i], exp[i])]
    assert not bad, bad[:5]
    prod = _field_op(hal, fid, 0, X, np.ascontiguousarray(inv))
    one, zero = fe([1], m)[0], fe([0], m)[0]
    assert all(np.array_equal(prod[i], one if xs[i] else zero) for i in range(len(xs)))


def test_invalid_arguments(hal):
    L = hal.load()
    x = np.zeros((4, 4), dtype=np.uint64)
    assert L.halo_field_op(7, 0, hal.ptr(x), hal.ptr(x), 4, hal.ptr(x)) == 1
    assert L.halo_ntt(0, None, 3, 0) == 1
