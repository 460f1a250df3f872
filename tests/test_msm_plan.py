"""The MSM launch plan (halo_amd/csrc/msm_plan.hpp) against literals.

A stand-alone program (tests/msm_plan_dump.cpp, built here by the host C++ compiler: the header
is free of HIP) prints the plan for a list of shapes; every field is compared with a literal.  The
literals restate the formulas of the four drivers as they stood in msm.hip before the plan existed
(commit 86685ec), worked out by hand from these lines of that file:

  msm_windows 356, msm_shifted_window_bits 361-371, msm_window_bits 373-377, msm_chunk_len 391-397;
  msm_device_t 514-557 (nn = max(n, 1), GLV NP = 2 nn, W = ceil(129 / c), B, SW, SN, NB, L, H, NT,
    key_bits, E, K, nchunks, ng1, ng2, the partials layout with max(nchunks, 1) slots, the
    reservations) and its fusion rule 573: headline, glv_1000, n0 / n1 (both kinds of bases), msm_2^24;
  msm_srs_pairs_t 798-821 and its fusion rule 848: the pair_* shapes;
  msm_shared_batch_t 1143-1176: batch_unshifted (c = 5, W = 51, B = 16, TS = 16) and batch_shifted
    (c_s = 17: two sub-digit windows of 2^8 buckets, TS = 15 x 16);
  msm_chunk_len's switch at E = 16 x 256 CUs x 1024 lanes (393): switch_below / switch_above (K is 16
    on both sides: ceil(E / resident) below, the floor of 16 above), and msm_2^24 well above (K = 64);
  the E = 0 plan: the max(nchunks, 1) guard of 548-552 alone.
The window sums hold SW windows and then the hiding terms (1 for msm_device_t, SW for the pairs, none
elsewhere: 557, 710, 817, 1169; msm_device_t reserved W + 1 where SW + 1 are used).
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("c W SW B L logL H logH NT key_bits K SN NB E nchunks ng1 ng2 off_first off_last off_g1 off_g2 "
          "digits_bytes bstart_bytes partials_bytes bucket_sums_bytes rows_bytes cols_bytes terms_bytes").split()


def _exp(text):
    vals = [int(v) for v in text.split()]
    assert len(vals) == len(FIELDS)
    return dict(zip(FIELDS, vals))


# name: (the driver refuses E >= 2^32, expected fields in FIELDS order)
SHAPES = {
    # one window-shifted output, n = 2^20, c = 17
    "headline": (False, _exp("17 15 1 65536 256 8 256 8 17 16 16 15728640 65536 15728640 983040 15360 240 "
                             "0 8847360 17694720 17832969 62914560 262148 285362208 8388608 32768 32768 2176")),
    # P = 2 outputs of half = 2^12 scalars
    "pair_c15": (True, _exp("15 17 2 16384 256 8 64 6 15 15 3 69632 32768 139264 46422 725 11 "
                            "0 417798 835596 842130 557056 131076 13475808 4194304 16384 65536 3840")),
    "pair_c16": (True, _exp("16 16 2 32768 256 8 128 7 16 16 2 65536 65536 131072 65536 1024 16 "
                            "0 589824 1179648 1188873 524288 262148 19024416 8388608 32768 65536 4096")),
    "pair_c17": (True, _exp("17 15 2 65536 256 8 256 8 17 17 1 61440 131072 122880 122880 1920 30 "
                            "0 1105920 2211840 2229129 491520 524292 35670528 16777216 65536 65536 4352")),
    # P = 4 (two sessions): 18-bit keys
    "pair4_c17": (True, _exp("17 15 4 65536 256 8 256 8 17 18 1 61440 262144 245760 245760 3840 60 "
                             "0 2211840 4423680 4458249 983040 1048580 71340768 33554432 131072 131072 8704")),
    # GLV over n = 1000 caller bases: NP = 2000, c = msm_window_bits(2000) = 7, W = SW = ceil(129 / 7)
    "glv_1000": (False, _exp("7 19 19 64 64 6 1 0 7 11 6 2000 1216 38000 6334 98 1 "
                             "0 57006 114012 114903 152000 4868 1838736 155648 2432 155648 17024")),
    # shared batch, T = 16 scalars, len = 1024 outputs
    "batch_unshifted": (True, _exp("5 51 52224 16 16 4 1 0 5 20 4 16 835584 835584 208896 3264 51 "
                                   "0 1880064 3760128 3789513 3342336 3342340 60639696 106954752 6684672 106954752 "
                                   "33423360")),
    "batch_shifted": (True, _exp("8 2 2048 256 256 8 1 0 9 19 2 240 524288 491520 245760 3840 60 "
                                 "0 2211840 4423680 4458249 1966080 2097156 71340768 67108864 262144 67108864 2359296")),
    # n = 0 and n = 1 give the same plan (nn = max(n, 1)); nchunks < 64, so no groups
    "n0_n1_glv": (False, _exp("6 22 22 32 32 5 1 0 6 10 1 2 704 44 44 0 0 "
                              "0 396 792 801 176 2820 12960 90112 2816 90112 16896")),
    "n0_n1_shifted": (False, _exp("17 15 1 65536 256 8 256 8 17 16 1 15 65536 15 15 0 0 "
                                  "0 135 270 279 60 262148 4608 8388608 32768 32768 2176")),
    "switch_below": (False, _exp("17 15 1 65536 256 8 256 8 17 16 16 4194304 65536 4194304 262144 4096 64 "
                                 "0 2359296 4718592 4755465 16777216 262148 76096800 8388608 32768 32768 2176")),
    "switch_above": (False, _exp("17 15 1 65536 256 8 256 8 17 16 16 4194305 65536 4194305 262145 4096 64 "
                                 "0 2359305 4718610 4755483 16777220 262148 76097088 8388608 32768 32768 2176")),
    "msm_2^24": (False, _exp("17 15 1 65536 256 8 256 8 17 16 64 251658240 65536 251658240 3932160 61440 960 "
                             "0 35389440 70778880 71331849 1006632960 262148 1141447968 8388608 32768 32768 2176")),
    "E0": (False, _exp("17 15 1 65536 256 8 256 8 17 16 1 0 65536 0 0 0 0 "
                       "0 9 18 27 0 262148 576 8388608 32768 32768 2176")),
}

# (P, n, W, B, key_bits) -> fused first pass
FUSE = [
    ((1, 1 << 20, 15, 65536, 16), True),    # headline
    ((1, 1 << 20, 14, 1 << 18, 18), True),  # c = 19: 573 has no key_bits term
    ((1, (1 << 27) - 1, 15, 65536, 16), True),
    ((1, 1 << 27, 15, 65536, 16), False),   # n < 2^31 / 16
    ((1, 4096, 17, 16384, 14), False),      # W > 16
    ((2, 4096, 17, 16384, 15), False),      # pair_c15: W > 16
    ((2, 4096, 16, 32768, 16), True),       # pair_c16
    ((2, 4096, 15, 65536, 17), True),       # pair_c17
    ((4, 4096, 15, 65536, 18), False),      # pair4_c17: key_bits > 17
    ((2, 4096, 16, 128, 9), False),         # B % 256: unreachable from the driver (W <= 16 forces c >= 16)
    ((2, 4096, 16, 256, 9), True),
]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "msm_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


def test_plans_match_the_drivers_formulas(dump):
    names = list(SHAPES)
    cmds = []
    for n in names:
        e = SHAPES[n][1]
        cmds.append("plan %d %d %d %d %d 256 %d %d" % (e["E"], e["NB"], e["SW"], e["B"], e["c"], e["W"], e["SN"]))
    for n, got in zip(names, dump(cmds)):
        refuses, e = SHAPES[n]
        for f in FIELDS:
            assert got[f] == e[f], (n, f, got[f], e[f])
        assert got["window_sums_bytes"] == [e["SW"] * 128, (e["SW"] + 1) * 128, 2 * e["SW"] * 128], n
        # the partials regions: as many entries as their writers index, disjoint, inside the buffer
        slots = max(e["nchunks"], 1)
        regions = [(got["off_first"], slots), (got["off_last"], slots), (got["off_g1"], e["ng1"] + 1),
                   (got["off_g2"], e["ng2"] + 1)]
        end = 0
        for off, count in regions:
            assert off >= end, (n, regions)
            end = off + 9 * count
        assert end * 16 <= got["partials_bytes"], n
        if refuses:
            assert got["E"] < 1 << 32 and got["NB"] < 1 << 32, n


def test_fusion_rule(dump):
    got = dump(["fuse %d %d %d %d %d" % a for a, _ in FUSE])
    assert [g["fuse"] for g in got] == [want for _, want in FUSE]


def test_window_choices(dump):
    got = dump(["bits 2000", "bits %d" % (1 << 20), "bits %d" % (1 << 16), "bits 0", "bits 1", "windows 17",
                "windows 15", "windows 8", "windows 5"])
    assert got[0]["window_bits"] == 7
    assert got[1] == {"window_bits": 16, "shifted_window_bits": 17}
    assert got[2] == {"window_bits": 12, "shifted_window_bits": 15}
    assert got[3]["window_bits"] == 6 and got[4]["window_bits"] == 6
    assert [g["windows"] for g in got[5:]] == [15, 17, 32, 51]
