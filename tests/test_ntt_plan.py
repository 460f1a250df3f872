"""The host-side decisions of a device NTT as halo_amd/csrc/ntt_plan.hpp plans them: the pass split and its cache
key, the zero-tail pruning of pass 0, each pass's launch geometry, buffers and tables, and the refusals.

A stand-alone program (tests/ntt_plan_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
answers single questions and sweeps every log n in 0..30 x ntt_big_max_log in {0, 16, 17, 20, 22, 99} x
ntt_even_split x in place or not x both directions x every prune request 0..log n, counting the plans that break a
property:

  radix       log n = 0 has no pass, else 1..4; every radix in [1, 11]; log_ns is the sum of the earlier radices and
              the radices sum to log n;
  block       radices up to 8 on 1024-element blocks, 9..11 on 2048 (the ranges NttSwz was searched for), ne / 4
              threads and 36 B of LDS per element;
  geometry    t grid_x = N / R, the block's t R positions fit ne, `full` says whether they fill it, and a block holds
              as many columns as fit unless the pass has fewer;
  tables      per-pass tables exist up to 2^24 and then for every pass but the first, 2^(log_r + log_ns) entries each;
  key         a radix fits the key's 5 bits and the key is the radices, 5 bits each;
  prune       only pass 0 of a forward transform prunes; the granted prune is ntt_pass0_prune's, at most the request,
              0 or in [ntt_g0, log_r), and on the wide blocks log_r - prune is even;
  chain       each pass reads what the one before wrote, the first reads IN, the last writes OUT;
  tmp2        TMP2 is only ever pass 0's destination, and only in place; needs_tmp2 says so;
  alias       no pass has one buffer as source and destination (IN and OUT are one buffer in place) unless the plan
              has one pass, and then grid_x = 1;
  out_scaled  exactly on the last pass of a transform with tables and more than one pass;
  read_end    N >> the granted prune, or N;
  ark, two_level  the first pass reads ark words and the last writes them; lo_bits = ceil(log n / 2), nlo nhi = N.

The literal tables below were worked out by hand from ntt_radices, ntt_split_key, ntt_pass0_prune, get_twiddles and
ntt_device as they stood in ntt.hip before the plan existed.  Two of them:
  log n = 25, even split: four passes of 8 with 7 bits to spare; taking 2 from the back three times gives 8, 6, 6, 6
              and 1 is left, which the last pass gives up: [8, 6, 6, 5].
  radix 9, prune request 4: 9 - 4 is odd and the block is wide, so 3; 3 >= G0 = 1 and 3 < 9: granted 3.
log n = 0 had the one "radix" 0 there and was copied before any pass ran; the plan has no pass for it.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo_amd", "csrc")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ntt_plan") / "ntt_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "ntt_plan_dump.cpp"),
                    "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


@pytest.fixture(scope="module")
def swept(dump):
    return dump(["sweep"])[0]


def test_every_plan_keeps_the_properties(swept):
    got = dict(swept)
    got.pop("seen")
    # sum over log n of (log n + 1) prune requests x 6 x 2 x 2 x 2
    assert got.pop("plans") == sum(l + 1 for l in range(31)) * 6 * 2 * 2 * 2
    assert got == {k: 0 for k in ("radix", "block", "geometry", "tables", "key", "prune", "chain", "tmp2", "alias",
                                  "out_scaled", "read_end", "ark", "two_level")}


def split(dump, logn, big=22, even=0):
    return dump(["split %d %d %d" % (logn, big, even)])[0]["radices"]


DEFAULT_SPLITS = {9: [5, 4], 13: [7, 6], 16: [8, 8], 17: [9, 8], 20: [10, 10], 21: [11, 10], 22: [11, 11], 23: [8, 8, 7],
                  24: [8, 8, 8], 25: [7, 6, 6, 6], 30: [8, 8, 7, 7]}
TUNED_SPLITS = [
    (9, 22, 1, [6, 3]), (13, 22, 1, [8, 5]), (25, 22, 1, [8, 6, 6, 5]),
    (17, 16, 0, [6, 6, 5]), (22, 16, 0, [8, 7, 7]),
    (17, 16, 1, [6, 6, 5]), (19, 16, 1, [8, 6, 5]), (22, 16, 1, [8, 8, 6]),
    (21, 20, 0, [7, 7, 7]),
]


def test_default_splits(dump):
    assert split(dump, 0) == []
    for logn in range(1, 9):
        assert split(dump, logn) == [logn]
    for logn, rad in DEFAULT_SPLITS.items():
        assert split(dump, logn) == rad, logn


@pytest.mark.parametrize("logn,big,even,rad", TUNED_SPLITS)
def test_tuned_splits(dump, logn, big, even, rad):
    assert split(dump, logn, big, even) == rad


def test_big_max_log_above_22_acts_as_22(dump):
    for logn in range(31):
        for even in (0, 1):
            assert split(dump, logn, 99, even) == split(dump, logn, 22, even) == split(dump, logn, 23, even), logn
    assert split(dump, 23, 99) == [8, 8, 7]


def test_split_key(dump):
    assert dump(["split 23 22 0"])[0]["key"] == (8 << 10) | (8 << 5) | 7
    assert dump(["split 30 22 0"])[0]["key"] == (8 << 15) | (8 << 10) | (7 << 5) | 7
    # two tunings that give one split share its tables; two splits of one size do not
    assert dump(["split 17 16 0"])[0]["key"] == dump(["split 17 16 1"])[0]["key"] != dump(["split 17 22 0"])[0]["key"]


PRUNE = {8: {1: 0, 2: 2, 3: 3, 7: 7, 8: 0}, 3: {2: 2, 3: 0}, 9: {1: 1, 2: 1, 4: 3}, 10: {1: 0, 3: 2, 9: 8, 10: 0},
         11: {2: 1, 3: 3, 10: 9, 11: 0}}


def test_prune_granted(dump):
    for lr, cases in PRUNE.items():
        for req, granted in cases.items():
            assert dump(["prune %d %d" % (lr, req)])[0]["granted"] == granted, (lr, req)
        assert dump(["prune %d 0" % lr])[0]["granted"] == 0


def plan(dump, logn, inverse=0, in_place=0, prune=0, big=22, even=0):
    return dump(["plan %d %d %d %d %d %d" % (logn, inverse, in_place, prune, big, even)])[0]


# (log n, pass) -> the fields the parent's pass loop and get_twiddles gave
GEOMETRY = [
    (3, 0, dict(log_r=3, ne=1024, t=1, grid_x=1, full=0, lds_bytes=36864, dst="OUT", table_entries=0)),
    (9, 0, dict(log_r=5, ne=1024, t=16, grid_x=1, full=0, dst="TMP", table_entries=0)),
    (9, 1, dict(log_r=4, ne=1024, t=32, grid_x=1, dst="OUT", table_entries=512)),
    (17, 0, dict(log_r=9, ne=2048, t=4, grid_x=64, full=1, lds_bytes=73728, threads=512, table_entries=0)),
    (17, 1, dict(log_r=8, ne=1024, t=4, grid_x=128, threads=256, table_entries=131072)),
    (20, 0, dict(log_r=10, ne=2048, t=2, grid_x=512, table_entries=0)),
    (20, 1, dict(log_r=10, ne=2048, t=2, grid_x=512, table_entries=1 << 20)),
    (22, 0, dict(log_r=11, ne=2048, t=1, grid_x=2048, table_entries=0)),
    (22, 1, dict(log_r=11, ne=2048, t=1, grid_x=2048, table_entries=1 << 22)),
    (24, 0, dict(log_r=8, grid_x=16384, dst="OUT", table_entries=0)),
    (24, 1, dict(log_r=8, grid_x=16384, dst="TMP", table_entries=65536)),
    (24, 2, dict(log_r=8, grid_x=16384, dst="OUT", table_entries=1 << 24)),
]


@pytest.mark.parametrize("logn,p,want", GEOMETRY, ids=["%d-%d" % c[:2] for c in GEOMETRY])
def test_geometry_roles_and_tables(dump, logn, p, want):
    got = plan(dump, logn)["pass"][p]
    assert {k: got[k] for k in want} == want


def test_no_tables_above_2p24(dump):
    got = plan(dump, 25)
    assert not got["tables"] and [q["dst"] for q in got["pass"]] == ["TMP", "OUT", "TMP", "OUT"]
    assert all(not q["table"] and q["table_entries"] == 0 and not q["out_scaled"] for q in got["pass"])
    assert plan(dump, 24)["tables"] and [q["out_scaled"] for q in plan(dump, 24)["pass"]] == [0, 0, 1]


def test_in_place_with_three_passes_goes_through_tmp2(dump):
    for logn, big in ((23, 22), (24, 22), (17, 16), (22, 16)):
        got = plan(dump, logn, in_place=1, big=big)
        assert got["needs_tmp2"] and [(q["src"], q["dst"]) for q in got["pass"]] == [("IN", "TMP2"), ("TMP2", "TMP"),
                                                                                    ("TMP", "OUT")], logn
        # out of place the same passes need no second scratch
        got = plan(dump, logn, big=big)
        assert not got["needs_tmp2"] and [q["dst"] for q in got["pass"]] == ["OUT", "TMP", "OUT"]
    for logn in (9, 17, 22, 25, 30):  # an even pass count ends on OUT without it
        assert not plan(dump, logn, in_place=1)["needs_tmp2"], logn
    one = plan(dump, 8, in_place=1)  # one workgroup reads and writes the caller's buffer
    assert one["npass"] == 1 and one["pass"][0]["grid_x"] == 1 and (one["pass"][0]["src"], one["pass"][0]["dst"]) == ("IN", "OUT")


def test_prune_in_the_plan(dump):
    # the prover's shape: 2^20 coefficients on the 2^23 domain, three stages of zeros
    got = plan(dump, 23, in_place=1, prune=3)
    assert got["pass"][0]["prune"] == 3 and got["read_end"] == 1 << 20 and [q["prune"] for q in got["pass"][1:]] == [0, 0]
    # radix 9 cuts a request of 2 to 1; radix 6 grants it
    assert plan(dump, 17, in_place=1, prune=2)["pass"][0]["prune"] == 1
    assert plan(dump, 17, in_place=1, prune=2)["read_end"] == 1 << 16
    assert plan(dump, 17, in_place=1, prune=2, big=16)["pass"][0]["prune"] == 2
    # the inverse transform never prunes; a request the radix cannot grant reads everything
    assert plan(dump, 23, inverse=1, prune=3)["pass"][0]["prune"] == 0 and plan(dump, 23, inverse=1, prune=3)["read_end"] == 1 << 23
    assert plan(dump, 20, prune=1)["pass"][0]["prune"] == 0 and plan(dump, 20, prune=1)["read_end"] == 1 << 20


def model_g0(ne, r):
    """tools/ntt_model.py's own line for the first group's stage count, evaluated as it stands there."""
    src = open(os.path.join(ROOT, "tools", "ntt_model.py")).read()
    (expr,) = re.findall(r"^\s*G0 = (.+)$", src, re.M)
    return eval(expr, {"min": min}, {"NE": ne, "r": r})


def test_g0_is_the_model_s_and_the_kernel_s(dump, swept):
    seen = [tuple(s) for s in swept["seen"]]
    assert sorted(seen) == [(1024, r) for r in range(1, 9)] + [(2048, r) for r in (9, 10, 11)]
    pairs = sorted(set(seen) | {(ne, r) for ne in (1024, 2048) for r in range(1, 12)})
    got = dump(["g0 %d %d" % p for p in pairs])
    assert [g["g0"] for g in got] == [model_g0(*p) for p in pairs]
    assert [model_g0(1024, r) for r in (1, 2, 3, 8)] == [1, 2, 2, 2] and [model_g0(2048, r) for r in (9, 10, 11)] == [1, 2, 1]
    # k_ntt_pass keeps the expression in its own text (the call moved two bytes of every instantiation): the same
    # expression as the header's, up to the case of NE and the suffix of a literal
    norm = lambda e: re.sub(r"\b(\d+)u\b", r"\1", e.replace("NE", "ne")).replace(" ", "")
    (kernel,) = re.findall(r"const uint32_t G0 = (.+);", open(os.path.join(CSRC, "ntt.hip")).read())
    (header,) = re.findall(r"ntt_g0\(int ne, unsigned r\) \{ return (.+); \}", open(os.path.join(CSRC, "ntt_plan.hpp")).read())
    assert norm(kernel) == norm(header)


def test_check_edges(dump):
    got = dump(["check 30 1", "check 31 1", "check 30 65535", "check 30 65536", "check 30 0", "check 31 0", "check 0 1",
                "check 4294967295 65536"])
    assert [g["check"] for g in got] == ["ok", "log_too_large", "ok", "batch_too_large", "empty", "log_too_large", "ok",
                                         "log_too_large"]
