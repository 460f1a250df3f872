"""The signed-window recoding core (halo_amd/csrc/digits_core.hpp) against a big-integer recoding.

A stand-alone program (tests/digits_core_dump.cpp, built here by the host C++ compiler: the header is
free of HIP) prints the sort entries of a list of integers for the constant widths 16 and 17 and for
the run-time path (its plain loop and its 16-times-unrolled form) with c in {13, 15, 16, 17, 18, 20}.
The core takes the scalar already folded to min(s, p - s) and the flip bit, so the fold is done here,
as the device wrapper (digits.hpp) does it: s is replaced by p - s when p - s < s.  Every entry is
compared with the Python recoding, the digits are checked to sum to the folded integer, and with the
flip applied to -+s modulo p; where a width has a constant and a run-time instantiation, the outputs
must be identical.
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two scalar fields (Pallas / Vesta): 2^254 + a 126-bit tail
MODULI = (0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001,
          0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001)
NONE = 0xFFFFFFFF
WIDTHS = (13, 15, 16, 17, 18, 20)


def windows(c):
    return (255 + c - 1) // c


def fold(s, p):
    """(min(s, p - s), flip): the device wrapper's rule, p - s < s."""
    return (p - s, 1) if p - s < s else (s, 0)


def signed_digits(t, c, W):
    """d_w in [-(2^(c-1) - 1), 2^(c-1)] with sum d_w 2^(c w) = t."""
    out = []
    for _ in range(W):
        d = t & ((1 << c) - 1)
        if d > 1 << (c - 1):
            d -= 1 << c
        out.append(d)
        t = (t - d) >> c
    assert t == 0, "W windows do not hold the integer"
    return out


def entries(digits, flip):
    return [NONE if d == 0 else (abs(d) - 1) | ((int(d < 0) ^ flip) << 31) for d in digits]


def from_digits(ds, c):
    return sum(d << (c * w) for w, d in enumerate(ds))


def scalars(p):
    rng = random.Random(20240517 ^ (p & 0xFFFF))
    out = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2, 2, p - 2]
    out += [rng.randrange(p) for _ in range(200)]
    out += [rng.randrange(1 << 64) for _ in range(8)]           # zero digits in the top windows
    out += [rng.randrange(1 << 200) for _ in range(8)]
    out.append((1 << 253) - 1)                                    # every window all ones: the carry runs to the top
    out.append(p - ((1 << 253) - 1))                              # ... and the same after the fold
    for c in WIDTHS:
        W = windows(c)
        half = 1 << (c - 1)
        out.append((1 << (c * (W - 1))) - 1)                      # all ones below the top window
        # a digit of magnitude exactly 2^(c-1): straight, and made by a carry (half - 1 after a negative digit)
        for w in (0, 1, W // 2, W - 2):
            out.append(half << (c * w))
            out.append(((half - 1) << (c * (w + 1))) | ((half + 1) << (c * w)))
        out.append(from_digits([half] * (W - 1), c))              # +2^(c-1) in every window but the top
        out.append(from_digits([half - 1, half] * ((W - 1) // 2), c))
        # chosen digits with zeros in the top window(s) and in the middle
        ds = [rng.randrange(-(half - 1), half + 1) for _ in range(W - 2)]
        ds[len(ds) // 2] = 0
        ds[-1] = rng.randrange(1, half)
        out.append(from_digits(ds, c))
    return [s % p for s in out]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("digits_core") / "digits_core_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "digits_core_dump.cpp"), "-o", exe], check=True)

    def run(mode, c, W, cases):
        lines = "".join("%s %d %d %d %064x\n" % (mode, c, W, flip, t) for t, flip in cases)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True)
        got = [[int(x, 16) for x in l.split()] for l in out.stdout.splitlines()]
        assert len(got) == len(cases)
        return got

    return run


@pytest.fixture(scope="module")
def cases():
    return [(p, s, *fold(s, p)) for p in MODULI for s in scalars(p)]


def _check(got, cases, c, W):
    for (p, s, t, flip), g in zip(cases, got):
        assert 2 * t <= p - 1 and t == (p - s if flip else s)
        ds = signed_digits(t, c, W)
        assert g == entries(ds, flip), (hex(s), c)
        # decode what the program printed: sum of the digits = t, and with the flip applied = s or s - p
        dec, signed = [], []
        for e in g:
            d = 0 if e == NONE else ((e & 0x7FFFFFFF) + 1) * (-1 if (e >> 31) ^ flip else 1)
            dec.append(d)
            signed.append(0 if e == NONE else ((e & 0x7FFFFFFF) + 1) * (-1 if e >> 31 else 1))
        assert from_digits(dec, c) == t
        assert from_digits(signed, c) % p == s % p
        assert all(abs(d) <= 1 << (c - 1) for d in dec)


@pytest.mark.parametrize("c", WIDTHS)
def test_runtime_width(dump, cases, c):
    W = windows(c)
    folded = [(t, flip) for _, _, t, flip in cases]
    got = dump("rt", c, W, folded)
    _check(got, cases, c, W)
    if W <= 16:  # the unrolled form of the fused scatter (W <= 16 windows)
        assert dump("rtu", c, W, folded) == got


@pytest.mark.parametrize("c", (16, 17))
def test_constant_width(dump, cases, c):
    W = windows(c)
    folded = [(t, flip) for _, _, t, flip in cases]
    got = dump("c%d" % c, c, W, folded)
    _check(got, cases, c, W)
    assert got == dump("rt", c, W, folded)
    assert got == dump("rtu", c, W, folded)


def test_fewer_windows_than_unrolled(dump):
    """The unrolled run-time loop produces exactly W entries: the windows from W on are skipped."""
    t = (1 << 100) - 12345
    for W in (1, 7, 8):
        got = dump("rtu", 13, W, [(t, 0)])[0]
        assert got == dump("rt", 13, W, [(t, 0)])[0] and len(got) == W
        assert got == entries(signed_digits(t, 13, 20)[:W], 0)
