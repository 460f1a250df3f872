"""The host field arithmetic (halo_amd/csrc/host_mont.hpp) against Python big integers.

Every point the library returns to a caller goes through HostMont::inv: the packed XYZZ -> WrappedPoint
conversions (one point, and up to 16 with one inversion by Montgomery's trick) and the scalar inverse
of the IPA's challenges.  A stand-alone program (tests/host_mont_dump.cpp, built here by the host C++
compiler: the header is free of HIP) prints their outputs for both fields; every output word must
equal the big-integer value.  The inputs sit at the edges the GPU tests never reach: coordinates in
[p, 2p), the identity anywhere in a batch, a batch whose running product stays one.

A packed coordinate is an integer below 2p congruent to v 2^261, the same factor in every coordinate,
so x = X / ZZ and y = Y / ZZZ; the outputs are the ark (Montgomery, R = 2^256) words x R and y R mod p.
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# FpCfg and FqCfg of consts.hpp: each is the base field of one curve and the scalar field of the other
FIELDS = {"fp": 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,
          "fq": 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001}
R = 1 << 256
M64 = (1 << 64) - 1


def words(v, n=4):
    return [(v >> (64 * i)) & M64 for i in range(n)]


def expect_point(p, pt):
    """(X, Y, ZZ, ZZZ), raw words in [0, 2p) -> the 8 words of the WrappedPoint."""
    X, Y, ZZ, ZZZ = (c % p for c in pt)
    if ZZ == 0:
        return [0] * 8
    return words(X * pow(ZZ, -1, p) * R % p) + words(Y * pow(ZZZ, -1, p) * R % p)


def random_point(rng, p):
    """Any four words below 2p with ZZ, ZZZ != 0 mod p (the conversion does not assume ZZ^3 = ZZZ^2)."""
    while True:
        pt = tuple(rng.randrange(2 * p) for _ in range(4))
        if pt[2] % p and pt[3] % p:
            return pt


def identity(rng, p, zz):
    return (rng.randrange(2 * p), rng.randrange(2 * p), zz, rng.randrange(2 * p))


def w1_line(f, pt):
    return "w1 %s %064x %064x %064x %064x\n" % ((f,) + tuple(pt))


def w2_line(f, pts):
    return "w2 %s %d %s\n" % (f, len(pts), " ".join("%064x" % c for pt in pts for c in pt))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip("no host C++ compiler (c++, g++ or clang++) to build tests/host_mont_dump.cpp")
    exe = str(tmp_path_factory.mktemp("host_mont") / "host_mont_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_mont_dump.cpp"), "-o", exe], check=True)

    def raw(lines):
        out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True)
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got

    def run(lines):
        return [[int(x, 16) for x in l.split()] for l in raw(lines)]

    run.raw = raw
    return run


def single_points(f):
    p = FIELDS[f]
    rng = random.Random(0x5EED0 ^ (p & 0xFFFF))
    pts = [identity(rng, p, 0), identity(rng, p, p)]        # ZZ = 0 and ZZ = p: the identity
    pts += [(2 * p - 1,) * 4, (1,) * 4, (p + 1,) * 4]
    pts += [random_point(rng, p) for _ in range(200)]
    return pts


def batches(f):
    p = FIELDS[f]
    rng = random.Random(0xBA7C4 ^ (p & 0xFFFF))
    out = []
    for k in (1, 2, 3, 16):
        out.append([random_point(rng, p) for _ in range(k)])
        for pos in sorted({0, k // 2, k - 1}):               # the identity first, in the middle, last
            b = [random_point(rng, p) for _ in range(k)]
            b[pos] = identity(rng, p, (0, p)[pos & 1])
            out.append(b)
        out.append([identity(rng, p, (0, p)[i & 1]) for i in range(k)])  # the running product stays one
        if k >= 2:                                            # two equal points
            b = [random_point(rng, p) for _ in range(k)]
            b[k - 1] = b[0]
            out.append(b)
    out.append([(2 * p - 1,) * 4, (1,) * 4, (p + 1,) * 4])   # the single-point edges as one batch
    return out


def inverse_inputs(f):
    p = FIELDS[f]
    rng = random.Random(0x1A7E5 ^ (p & 0xFFFF))
    out = [1, p - 1, 2, (p + 1) // 2, p + 5]                  # p + 5: reduced once on entry
    while len(out) < 205:
        a = rng.randrange(R)
        if a % p:
            out.append(a)
    return out


@pytest.mark.parametrize("f", sorted(FIELDS))
def test_xyzz_to_wrapped(dump, f):
    p = FIELDS[f]
    pts = single_points(f)
    got = dump([w1_line(f, pt) for pt in pts])
    assert got[0] == [0] * 8 and got[1] == [0] * 8
    for pt, g in zip(pts, got):
        assert g == expect_point(p, pt), [hex(c) for c in pt]


@pytest.mark.parametrize("f", sorted(FIELDS))
def test_xyzz_to_wrapped_batch(dump, f):
    p = FIELDS[f]
    bs = batches(f)
    assert all(1 <= len(b) <= 16 for b in bs)                 # the arrays are sized for 16 (points.hpp)
    got = dump([w2_line(f, b) for b in bs])
    one = iter(dump([w1_line(f, pt) for b in bs for pt in b]))
    for b, g in zip(bs, got):
        assert len(g) == 8 * len(b)
        for i, pt in enumerate(b):
            gi = g[8 * i:8 * i + 8]
            assert gi == next(one), (len(b), i)               # the single-point function on the same input
            assert gi == expect_point(p, pt), (len(b), i, [hex(c) for c in pt])


@pytest.mark.parametrize("f", sorted(FIELDS))
def test_scalar_inverse(dump, f):
    p = FIELDS[f]
    assert dump(["inv %s %064x\n" % (f, a) for a in (0, p)]) == [[0], [0]]
    ins = inverse_inputs(f)
    got = dump(["inv %s %064x\n" % (f, a) for a in ins])
    for a, g in zip(ins, got):
        # a = x R: the output is x^-1 R = a^-1 R^2 mod p
        assert g == [1] + words(pow(a, -1, p) * R * R % p), hex(a)


# ---- host_scalar.hpp: the one below-the-modulus predicate, check_rho and HostScalar ------------------
HALO_OK, HALO_EINVAL = 0, 1


def edge_values(p):
    """Where a limb-wise comparison with p can go wrong: the ends of the range, p and its neighbours, the
    values that equal p in three limbs and differ by one in the lowest (p - 1, p + 1) or in the top one."""
    top = 1 << 192
    return [0, 1, p - 1, p, p + 1, (1 << 255) - 1, R - 1, p - top, p + top, p - top + 1, p + top - 1]


@pytest.mark.parametrize("f", sorted(FIELDS))
def test_scalar_below(dump, f):
    p = FIELDS[f]
    vals = edge_values(p)
    got = dump(["below %s 1 %064x\n" % (f, a) for a in vals])
    for a, g in zip(vals, got):
        assert g == [int(a < p), int(a < p)], hex(a)
    # the span form: all of the values, none of them (true), and the ones below p only
    low = [a for a in vals if a < p]
    span = lambda xs: "below %s %d %s\n" % (f, len(xs), " ".join("%064x" % a for a in xs))
    got = dump([span(vals), span([]), span(low), span(low + [p]), span([p] + low)])
    assert got[0] == [sum(int(a < p) << i for i, a in enumerate(vals)), 0]
    assert got[1] == [0, 1]
    assert got[2] == [(1 << len(low)) - 1, 1]
    assert got[3][1] == 0 and got[4][1] == 0


@pytest.mark.parametrize("f", sorted(FIELDS))
def test_check_rho(dump, f):
    p = FIELDS[f]
    rho = lambda xs: "rho %s %d %s\n" % (f, len(xs), " ".join("%064x" % a for a in xs))
    got = dump.raw([rho([1, p - 1, 5]), "rho %s -1\n" % f, rho([]), rho([1, 0, p]), rho([p - 1, 2, p]), rho([R - 1]),
                    rho([p + 1, 0])])
    assert got[0] == "%d|" % HALO_OK and got[1] == "%d|" % HALO_OK and got[2] == "%d|" % HALO_OK
    assert got[3] == "%d|the_call: rho[1] is zero" % HALO_EINVAL
    assert got[4] == "%d|the_call: rho[2] is not below the modulus" % HALO_EINVAL
    assert got[5] == "%d|the_call: rho[0] is not below the modulus" % HALO_EINVAL
    assert got[6] == "%d|the_call: rho[0] is not below the modulus" % HALO_EINVAL    # the first fault is reported


@pytest.mark.parametrize("f", sorted(FIELDS))
def test_host_scalar_arith(dump, f):
    """HostScalar takes inputs below the modulus: the edge values that are, in every pair."""
    p = FIELDS[f]
    rng = random.Random(0xA517 ^ (p & 0xFFFF))
    vals = [a for a in edge_values(p) if a < p] + [(p - 1) // 2, (p + 1) // 2] + [rng.randrange(p) for _ in range(6)]
    pairs = [(a, b) for a in vals for b in vals]
    got = dump(["arith %s %064x %064x\n" % (f, a, b) for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert g == words((a + b) % p) + words((a - b) % p) + words(-a % p), (hex(a), hex(b))
