"""The scalar recoding in two steps (halo_amd/csrc/digits_core.hpp digits_fold / digits_unfold) against
the one-step recoding and Python integers.

The fused first sort pass converts and folds a scalar once: the histogram kernel stores the folded
canonical integer min(s, p - s) < 2^254 with the fold's sign in bit 255 (32 B), and the scatter cuts its
windows from those words.  A stand-alone program (tests/digits_two_step_dump.cpp, host C++ only) takes
ark Montgomery scalars and prints, for each, the entries of the one-step recoding, the stored words and
the entries cut from the stored words after a trip through memory.  Asserted for c in {13, 16, 17, 19},
with the constant-width instantiations at 16 and 17 and the run-time ones (plain loop; unrolled where
W <= 16) at every width:
  * the stored words are min(s, p - s) | flip << 255, flip set exactly when p - s < s;
  * the two-step entries equal the one-step entries;
  * the digits they encode sum to +-s: sum_w d_w 2^(c w) = s (mod p), every |d_w| <= 2^(c - 1).
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two scalar fields as consts.hpp names them (FpCfg: Pallas' scalars, FqCfg: Vesta's)
MODULI = {"fp": 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,
          "fq": 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001}
NONE = 0xFFFFFFFF
WIDTHS = (13, 16, 17, 19)


def windows(c):
    return (255 + c - 1) // c


def modes(c):
    out = ["rt"]
    if windows(c) <= 16:
        out.append("rtu")
    if c in (16, 17):
        out.append("c%d" % c)
    return out


def scalars(p):
    rng = random.Random(0x2057E9 ^ (p & 0xFFFF))
    out = [0, 1, 2, (p - 1) // 2, (p + 1) // 2, p - 1, ((1 << 254) - 1) % p]
    out += [rng.randrange(p) for _ in range(300)]
    return out


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("digits_two_step") / "digits_two_step_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "digits_two_step_dump.cpp"), "-o", exe], check=True)

    def run(field, mode, c, ss):
        p = MODULI[field]
        R = (1 << 256) % p
        lines = "".join("%s %s %d %d %064x\n" % (field, mode, c, windows(c), s * R % p) for s in ss)
        out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True)
        got = [[int(x, 16) for x in l.split()] for l in out.stdout.splitlines()]
        assert len(got) == 3 * len(ss)
        return [got[3 * i:3 * i + 3] for i in range(len(ss))]

    return run


def decode(entries):
    return [0 if e == NONE else ((e & 0x7FFFFFFF) + 1) * (-1 if e >> 31 else 1) for e in entries]


@pytest.mark.parametrize("field", sorted(MODULI))
@pytest.mark.parametrize("c", WIDTHS)
def test_two_step_equals_one_step(dump, field, c):
    p = MODULI[field]
    ss = scalars(p)
    W = windows(c)
    first = None
    for mode in modes(c):
        got = dump(field, mode, c, ss)
        for s, (one, stored, two) in zip(ss, got):
            flip = int(p - s < s)
            t = p - s if flip else s
            assert 2 * t <= p - 1 and t < 1 << 254
            assert sum(w << (32 * q) for q, w in enumerate(stored)) == t | (flip << 255), hex(s)
            assert two == one and len(two) == W, (hex(s), mode)
            ds = decode(two)
            assert all(abs(d) <= 1 << (c - 1) for d in ds)
            assert (sum(d << (c * w) for w, d in enumerate(ds)) - s) % p == 0, (hex(s), mode)
            # the sign bits before the flip encode the folded integer itself
            assert sum(d << (c * w) for w, d in enumerate(ds)) == (-t if flip else t)
        if first is None:
            first = got
        else:  # the instantiations of one width agree
            assert got == first, mode
