"""The scratch carving of the batched verifier calls (halo_amd/csrc/scratch_layout.hpp) on the CPU.

ScratchLayout hands out 256-byte-aligned offsets into one device buffer and HostParts lays the arrays of a
host call out the same way for upload_parts (runtime.cpp).  A stand-alone program
(tests/scratch_layout_dump.cpp, built here by the host C++ compiler: the header is free of HIP) prints the
offsets; they are checked for the properties every user relies on and against three layouts worked out by
hand from the arithmetic the units had before the shared header (commit 7459456), so the header is checked
against that arithmetic and not against itself:

  fs_device (pcdl_fs.hip:236-238 there), k = 3, lg = 4 (t = 10), hiding, no xis_out:
      o_sc = align(3 * 10 * 64 = 1920) = 2048, o_sum = 2048 + align(960) = 3072, o_xis = 3072 + align(384) = 3584,
      o_cp = 3584 + align(3 * 5 * 32 = 480) = 4096, o_bad = 4096 + align(192) = 4352, total = 4352 + align(3) = 4608
  decide_combined (decider.hip:260-261 there), k = 5:
      o_U = align(160) = 256, o_P = 256 + align(320) = 768, then four steps of 256: o_neg = 1024, o_sum = 1280,
      o_comb = 1536, o_valid = 1792; total = 1792 without bisect, 1792 + align(5) = 2048 with it
  plonk_device (plonk_verify.hip:638-647 there), k = 2, lg = 6, full (ipp = 4, nx = 2), npi = 0 (m = 1), no
  chal_out / sides_out / asdl_out, R_TERMS = 43, RO_TERMS = 4; the aligned sizes in order:
      5632 2816 512 256 | 256 256 512 256 256 1792 | 256 512 256 256 256 | 512 256 256 | 256 256 256 256 |
      3072 3072 512 256 | 512 1536 256 256: o_comb = 25600, and the buffer is 25856 bytes
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [0, 1, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, (1 << 31) + 1, (1 << 40) + 255]


def align(n):
    return (n + 255) // 256 * 256


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if not cxx or not shutil.which(cxx):
        pytest.skip("no host C++ compiler (c++, g++ or clang++) to build tests/scratch_layout_dump.cpp")
    exe = str(tmp_path_factory.mktemp("scratch_layout") / "scratch_layout_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "scratch_layout_dump.cpp"), "-o", exe], check=True)

    def run(mode, rows):
        lines = ["%s %d %s\n" % (mode, len(r), " ".join(map(str, r))) for r in rows]
        out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True)
        got = [[int(x) for x in l.split()] for l in out.stdout.splitlines()]
        assert len(got) == len(rows)
        return got

    return run


def sweeps():
    """Every size alone, every ordered pair, and all of them in both orders."""
    return [[a] for a in SIZES] + [[a, b] for a in SIZES for b in SIZES] + [SIZES, SIZES[::-1], []]


def test_layout_properties(dump):
    rows = sweeps()
    for sizes, got in zip(rows, dump("layout", rows)):
        offs, total = got[:-1], got[-1]
        assert len(offs) == len(sizes)
        assert all(o % 256 == 0 for o in offs), sizes
        assert total == sum(align(b) for b in sizes), sizes          # so a zero-byte part consumes nothing
        end = 0
        for b, o in zip(sizes, offs):                                # in order, and no part overlaps the one before
            assert o == end, sizes
            end = o + align(b)
            assert o + b <= end


def test_host_parts(dump):
    rows = sweeps()
    for sizes, lay, got in zip(rows, dump("layout", rows), dump("parts", rows)):
        assert got[-1] == lay[-1], sizes
        for b, o, at in zip(sizes, lay[:-1], got[:-1]):
            assert at == (o if b else -1), sizes                     # an absent row, else the layout's offset


def test_parent_literals(dump):
    """The three layouts of the module docstring, by the parent's arithmetic."""
    k, lg, t = 3, 4, 10
    fs = [k * t * 64, k * t * 32, k * 128, k * (lg + 1) * 32, k * 64, k]
    k = 5
    comb = [[k * 32, k * 64, 64, 64, 128, 1, k if bisect else 0] for bisect in (True, False)]
    k, lg, ipp, nx, m, r_terms, ro_terms = 2, 6, 4, 2, 1, 43, 4
    plonk = [k * r_terms * 64, k * r_terms * 32, k * ro_terms * 64, k * ro_terms * 32, k * 128, k * 128, ipp * k * 64,
             ipp * k * 32, ipp * k * 32, ipp * k * (lg + 1) * 32, k * m * 32, 3 * k * 64, 3 * k * 32, k * 64, k * 128,
             k * 5 * 32, k * 2 * 32, k * 2 * 32, k, k, ipp * k, k, 4 * nx * lg * 64, 4 * nx * lg * 64, 4 * nx * 64,
             4 * nx * 32, nx * (lg + 1) * 32, 3 * nx * (lg + 1) * 32, nx, nx, 1]
    got = dump("layout", [fs, comb[0], comb[1], plonk])
    assert got[0] == [0, 2048, 3072, 3584, 4096, 4352, 4608]
    assert got[1] == [0, 256, 768, 1024, 1280, 1536, 1792, 2048]
    assert got[2] == [0, 256, 768, 1024, 1280, 1536, 1792, 1792]
    assert got[3][-2] == 25600 and got[3][-1] == 25856
