"""The host walk over serialized pcdl Instances (halo_amd/csrc/wire_plan.hpp) and the Python restatement of the wire
format (tests/wire_ref.py), on the CPU.

tests/wire_plan_dump.cpp is built by the host C++ compiler (the header is free of HIP), once plainly and once with
-fsanitize=address,undefined; both programs run stand-alone over the same cases and walk each case in a heap block
of exactly its length, so a read past the buffer is a sanitizer report and a non-zero exit.

The fixture tests/golden/wire_qs_head.bin holds 18 Pallas instances serialized by the reference (n = 4 .. 1024, two
of each, all hiding); wire_qs_head.npz what tests/wire_ref.py decodes from them (tests/golden/make_wire.py).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pasta as P
import wire_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, TRUNCATED, LENGTH_PREFIX, ROUNDS, NOT_POW2, TAG, OPTION_PAIR, TOO_MANY, TRAILING = range(9)


@pytest.fixture(scope="module")
def head():
    return open(os.path.join(GOLDEN, "wire_qs_head.bin"), "rb").read()


@pytest.fixture(scope="module")
def expect():
    return np.load(os.path.join(GOLDEN, "wire_qs_head.npz"))


def build(tmp, name, extra):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", *extra, "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wire_plan_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def walk(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wire_plan")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    exe = build(tmp, "wire_plan_dump_" + request.param, extra)

    def run(cases):
        """cases: (bytes, vec_prefix, max_k) -> the program's answers"""
        text = "".join("%s %d %d\n" % (b.hex() or "-", int(vec), max_k) for b, vec, max_k in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        got = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(got) == len(cases)
        return got

    return run


def u64(x):
    return int(x).to_bytes(8, "little")


# offsets inside the n = 4 hiding instance (lg = 2): C 0, d 33, z 41, v 73, |Ls| 105, Ls 113, |Rs| 179, Rs 187,
# U 253, c 286, tag 318, C_bar 319, tag 352, w_prime 353, end 385
D_AT, LS_LEN, RS_LEN, TAG_CBAR, TAG_W, END = 33, 105, 179, 318, 352, 385


def patched(b, at, new):
    return b[:at] + new + b[at + len(new):]


def test_fixture_walks_to_the_recorded_layout(walk, head, expect):
    got = walk([(head, False, 18), (u64(18) + head, True, 18), (head, False, 64)])
    for g, shift in zip(got, (0, 8, 0)):
        assert g["status"] == OK and g["k"] == 18
        assert [i[0] - shift for i in g["instances"]] == expect["offsets"].tolist()
        assert [i[1] - shift for i in g["instances"]] == expect["ends"].tolist()
        assert [i[2] for i in g["instances"]] == expect["d"].tolist()
        assert [i[3] for i in g["instances"]] == expect["hiding"].tolist()
        assert g["instances"][-1][1] - shift == len(head)  # the walk ends at the last byte


def test_every_truncation_is_refused(walk, head):
    one = head[:END]
    assert walk([(one, False, 1)])[0]["status"] == OK
    # every proper prefix with at least one byte is an instance that ends early ...
    got = walk([(one[:n], False, 4) for n in range(1, END)])
    assert [g["status"] for g in got] == [TRUNCATED] * (END - 1)
    assert all(g["k"] == 0 and g["bad"] == 0 for g in got)
    # ... also behind one whole instance, where the second is the one named
    got = walk([(one + one[:n], False, 4) for n in (1, 40, 112, 300, 384)])
    assert [(g["status"], g["k"], g["bad"]) for g in got] == [(TRUNCATED, 1, 1)] * 5
    # no bytes at all is an empty list without a prefix; as a Vec of one instance all 385 lengths are refused
    assert walk([(b"", False, 4)])[0] == {"status": OK, "message": "ok", "k": 0, "bad": 0, "instances": []}
    got = walk([(u64(1) + one[:n], True, 4) for n in range(END)])
    assert all(g["status"] in (TRUNCATED, LENGTH_PREFIX) and g["k"] == 0 for g in got)
    assert [g["status"] for g in got[188:]] == [TRUNCATED] * (END - 188)  # 188 bytes: the shortest instance
    assert walk([(u64(1)[:5], True, 4)])[0]["status"] == TRUNCATED


def test_malformed_structure_is_refused_with_its_status(walk, head):
    one = head[:END]
    cases = [
        (patched(one, LS_LEN, u64(2**64 - 1)), LENGTH_PREFIX),
        (patched(one, LS_LEN, u64(len(one))), LENGTH_PREFIX),
        (patched(one, RS_LEN, u64(2**64 - 1)), LENGTH_PREFIX),
        (patched(one, RS_LEN, u64(2**61)), LENGTH_PREFIX),       # 33 * 2^61 wraps a 64-bit product
        (patched(one, RS_LEN, u64(3)), ROUNDS),                   # Ls != Rs
        (patched(one, RS_LEN, u64(1)), ROUNDS),
        (patched(one, LS_LEN, u64(1)), ROUNDS),                   # differs from lg(d + 1)
        (patched(one, TAG_CBAR, b"\2"), TAG),
        (patched(one, TAG_W, b"\2"), TAG),
        (patched(one, TAG_W, b"\xff"), TAG),
        (patched(one, TAG_W, b"\0"), OPTION_PAIR),                # a lone C_bar
        (one[:TAG_CBAR] + b"\0\1" + bytes(32), OPTION_PAIR),      # a lone w_prime
        (patched(one, D_AT, u64(4)), NOT_POW2),
        (patched(one, D_AT, u64(2**64 - 1)), NOT_POW2),           # d + 1 wraps to 0
        (patched(one, D_AT, u64(7)), ROUNDS),                     # a power of two that the two lengths do not match
    ]
    got = walk([(b, False, 4) for b, _ in cases])
    assert [g["status"] for g in got] == [s for _, s in cases]
    assert all(g["k"] == 0 for g in got)
    messages = {g["status"]: g["message"] for g in got}
    assert len(set(messages.values())) == len(messages)  # a message of its own for each status


def test_vec_prefix_and_capacity(walk, head):
    two = head[:2 * END]
    got = walk([(u64(2) + two, True, 2), (u64(1) + two, True, 2), (u64(3) + two, True, 4), (u64(2**64 - 1) + two, True, 4),
                (u64(len(two)) + two, True, 4), (two, False, 1), (u64(2) + two, True, 1), (u64(0), True, 0)])
    assert [(g["status"], g["k"]) for g in got] == [(OK, 2), (TRAILING, 1), (TRUNCATED, 2), (LENGTH_PREFIX, 0),
                                                     (LENGTH_PREFIX, 0), (TOO_MANY, 1), (TOO_MANY, 1), (OK, 0)]


# ---------------------------------------------------------------------------------------------
# tests/wire_ref.py against the reference's bytes and against itself
# ---------------------------------------------------------------------------------------------
def test_wire_ref_reproduces_the_fixture(head, expect):
    cv = P.PALLAS
    qs = W.decode_instances(cv, head)
    assert len(qs) == 18 and W.encode_instances(cv, qs) == head
    assert W.decode_instances(cv, u64(18) + head, vec=True) == qs
    flags = set()
    for q in qs:
        for pt in [q["C"], q["U"], q["C_bar"], *q["Ls"], *q["Rs"]]:
            assert P.on_curve(cv, pt)
            flags.add(W.encode_point(cv, pt)[32])
    assert flags == {0x00, 0x80}
    for i, q in enumerate(qs):
        a, b = expect["rounds"][i], expect["rounds"][i + 1]
        assert [W.wrapped(cv, p) for p in q["Ls"]] == expect["Ls"][a:b].tolist()
        assert W.ark_scalar(q["c"], cv.scalar) == expect["c"][i].tolist()
        assert W.instance_size(len(q["Ls"]), True) == expect["ends"][i] - expect["offsets"][i]


def test_wire_ref_roots_and_refusals():
    for p in (P.FP_MODULUS, P.FQ_MODULUS):
        assert W.sqrt(0, p) == 0 and W.sqrt(1, p) == 1 and W.sqrt(4, p) == 2 and W.sqrt(5, p) is None
        for a in (2, 3, 7, 12345678901234567890, p - 1, p - 4):
            r = W.sqrt(a, p)
            assert (r is None) == (not W.is_square(a, p))
            if r is not None:
                assert r * r % p == a and r <= p - r
    for cv in (P.PALLAS, P.VESTA):
        g = cv.generator
        for pt in (g, P.neg(cv, g), P.INF, P.mul(cv, 12345, g)):
            assert W.decode_point(cv, W.encode_point(cv, pt)) == pt
        x = (cv.base - 1).to_bytes(32, "little")
        for rec in (x + b"\xc0", x + b"\x01", x + b"\x20", (7).to_bytes(32, "little") + b"\x40",
                    cv.base.to_bytes(32, "little") + b"\0", (2**255 - 1).to_bytes(32, "little") + b"\0", bytes(33)):
            assert not W.point_valid(cv, rec)
        with pytest.raises(W.WireError):
            W.decode_scalar(cv.scalar.to_bytes(32, "little"), cv.scalar)
