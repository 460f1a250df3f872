"""k_acc's cursor over the sorted entries (halo_amd/csrc/acc_entries.hpp) on the host.

A stand-alone program (tests/acc_entries_walk.cpp, built here by the host C++ compiler with the address
and undefined-behaviour sanitizers: the header is free of HIP) walks every chunk the way acc_chunk does
(beg = t K, end = min(count, beg + K)) for K = 1 .. 17, 30, 60, 64 and every count 0 .. 3 K + 5, and checks
that the cursor hands out exactly keys[e] and vals[e] for every e in [beg, end), and loads one 16-byte group
per array at the chunk's start and at every multiple of four after it and nowhere else.  Its arrays
have exactly acc_entries_bytes(count) bytes, the reservation of the sorted arrays' owners (sort.hip
msm_radix_sort, msm.hip msm_shared_batch_t) at the tightest E = count, so a group that reached past the
reservation would be the sanitizer's report.  The control runs the same walk over arrays of the earlier
reservation, max(count, 1) * 4 bytes, and expects that report.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = list(range(1, 18)) + [30, 60, 64]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("acc_entries") / "acc_entries_walk")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "acc_entries_walk.cpp"), "-o", exe], check=True)

    def run(args):
        return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)

    return run


def model(K):
    """(chunks, entries, loads per array) over the counts 0 .. 3 K + 5."""
    chunks = entries = loads = 0
    for cnt in range(3 * K + 6):
        for beg in range(0, cnt, K):
            end = min(cnt, beg + K)
            chunks += 1
            entries += end - beg
            loads += 1 + sum(1 for e in range(beg + 1, end) if e % 4 == 0)
    return chunks, entries, loads


def test_cursor_returns_every_entry_and_reloads_at_multiples_of_four(walk):
    r = walk(KS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(KS)
    for K, line in zip(KS, lines):
        chunks, entries, loads = model(K)
        assert line == "K %d counts %d chunks %d entries %d loads %d" % (K, 3 * K + 6, chunks, entries, loads)
        # a quarter of the loads of one per entry, up to one more per chunk (the start inside a group)
        assert entries / 4 <= loads <= entries / 4 + chunks


def test_groups_stay_inside_the_reservation_only_since_it_is_whole_groups(walk):
    """The earlier reservation cuts the last group whenever the count is no multiple of four: the sanitizer
    stops the walk at count 1."""
    r = walk(["old", 1])
    assert r.returncode != 0
    assert "AddressSanitizer: heap-buffer-overflow" in r.stderr, r.stderr[-4000:]
