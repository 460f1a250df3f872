"""The path of an IPA session as halo_amd/csrc/ipa_plan.hpp plans it: the form of G, what every round launches and
what every fold does, for given (n, SRS, tunings).

A stand-alone program (tests/ipa_plan_dump.cpp, built here by the host C++ compiler: the header is free of HIP)
sweeps n over every power of two from 2 to 2^24, G explicit or the SRS prefix, an SRS of n and of 2n points, the
window-shifted copies resident or not, the tuning sets the GPU tests pin (the defaults; ipa_srs_tail_n = 0 and = n,
ipa_weighted = 0, ipa_tail = 0, ipa_mat_n = 0, ipa_pair_max = 0 one at a time; ipa_weighted = 0 with
ipa_srs_tail_n = 0, the "fold" modes of tests/test_gpu_prover.py), a session advanced alone and in lockstep, and
drives round and fold alternately until m = 0, and folds only (pcdl.rs test_u_check).  It keeps its own account of
what was written into gs and counts the steps that break a property:

  rounds         exactly lg n rounds and folds, a round leaves m alone and a fold halves it;
  tail_left      Tail is never left or entered twice, and a round's kind matches its form;
  weighted_cond  Weighted occurs only without explicit G and with the shifted copies resident;
  explicit_g     a session with explicit G is Folded throughout, folds G, never fetches and never uses the SRS table;
  gs_read        an MSM over gs, a G fold and an own tail table find G written into gs (after the step's fetch, which
                 only the unfolded prefix allows), affine for the first two and in the layout the table build is told;
                 the plan's own gs_current / gs_xyzz agree with that account;
  srs_table      the SRS table is chosen only while G0 is the unfolded prefix and n0 <= min(srs_tab_n, srs.n);
  mat            G is materialised at most once, at the first round with 2m <= ipa_mat_n, and no weighted round
                 runs at such a length;
  deferred       a fold is deferred in Tail and nowhere else;
  wlen           wlen 2m = n0 in Weighted and Tail (wlen = n0 once m = 0).

The literal traces below were worked out by hand from ipa_setup and ipa_round_launch as they stood before the plan
existed (constants: IPA_TAIL_N = 2048, TAIL_FUSE_N = 256, srs_tab_n = 8192; defaults: ipa_tail = ipa_weighted = 1,
ipa_srs_tail_n = 4096, ipa_mat_n = 2048, ipa_pair_max = 2^19).  The default at n = 2^14 over a shifted SRS:
  setup     allow_tail = 1; tail_from_srs = (2^14 <= min(4096, 8192, 2^14)) = 0; weighted = shifted and n > 2048 and
            not tail_from_srs and ipa_weighted = 1, which clears allow_tail.  gs is not filled (need_gs = 0).
  rounds 1-3  2m = 16384, 8192, 4096 > ipa_mat_n: weighted rounds; n0 / 2 = 8192 terms per side <= ipa_pair_max, so
            L and R are one pair MSM.  Each fold is the weight fold (wlen 1 -> 2 -> 4 -> 8).
  round 4   2m = 2048 <= ipa_mat_n: allow_tail is read again (1), to_tail = (2048 <= IPA_TAIL_N) = 1, so G is
            materialised as XYZZ; weighted = 0.  Then not tail and allow_tail and 2m <= IPA_TAIL_N: the tail is entered;
            gs_srs_prefix = 0, so the session builds its own table from the XYZZ gs, n0 = 2048 > TAIL_FUSE_N: the
            split tail round.
  rounds 5-14  tail rounds over the same table (n0 stays 2048): eleven tail rounds in all, every fold deferred.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULTS = dict(tail=1, weighted=1, srs_tail_n=4096, mat_n=2048, pair_max=1 << 19)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ipa_plan") / "ipa_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "halo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ipa_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
        return [json.loads(l) for l in out.stdout.splitlines()]

    return run


def test_every_path_keeps_the_properties(dump):
    got = dump(["sweep"])[0]
    # 24 sizes x explicit or not x two SRS lengths x shifted or not x 8 tuning sets x solo or not x rounds or folds only
    assert got.pop("runs") == 24 * 2 * 2 * 2 * 8 * 2 * 2
    assert got == {"rounds": 0, "tail_left": 0, "weighted_cond": 0, "explicit_g": 0, "gs_read": 0, "srs_table": 0,
                   "mat": 0, "deferred": 0, "wlen": 0}


def trace(dump, logn, shifted=1, explicit=0, srs_n=None, solo=1, **knobs):
    t = dict(DEFAULTS, **knobs)
    n = 1 << logn
    line = "trace %d %d %d %d 8192 %d %d %d %d %d %d" % (n, explicit, srs_n or n, shifted, t["tail"], t["weighted"],
                                                        t["srs_tail_n"], t["mat_n"], t["pair_max"], solo)
    got = dump([line])[0]
    assert got.pop("violations") == 0
    return got


# the modes of tests/test_gpu_prover.py::test_ipa_open_tail_switch_vs_c_restatement, with its knobs
def mode_knobs(mode, n):
    knobs = {"weighted": 1 if mode.startswith("weighted") else 0, "srs_tail_n": n if mode == "srs_tail" else 0}
    if mode == "weighted_to_end":
        knobs["mat_n"] = 0
    if mode == "weighted_fold_after":
        knobs["tail"] = 0
    return knobs


OWN = "tail_own>tail_split"
MAT = "mat_xyzz>tail_own>tail_split"
MODE_TRACES = [
    # G is copied at setup, folded until 2m = 2048, then the session's own table; every tail fold is deferred
    ("fold", 12, "srs_prefix+copy_gs", ["lr_msm", OWN] + ["tail_split"] * 10, ["g"] + ["deferred"] * 11, "tail"),
    ("fold", 13, "srs_prefix+copy_gs", ["lr_msm"] * 2 + [OWN] + ["tail_split"] * 10, ["g"] * 2 + ["deferred"] * 11, "tail"),
    # round 1 on the shifted SRS ranges, round 2 over the folded gs
    ("fold_srs_round0", 13, "srs_prefix+copy_gs", ["lr_srs_ranges", "lr_msm", OWN] + ["tail_split"] * 10,
     ["g"] * 2 + ["deferred"] * 11, "tail"),
    # weighted rounds while 2m > ipa_mat_n = 2048, then G as XYZZ and the own table
    ("weighted", 12, "weighted", ["weighted_pair", MAT] + ["tail_split"] * 10, ["weights"] + ["deferred"] * 11, "tail"),
    ("weighted", 13, "weighted", ["weighted_pair"] * 2 + [MAT] + ["tail_split"] * 10, ["weights"] * 2 + ["deferred"] * 11,
     "tail"),
    ("weighted", 14, "weighted", ["weighted_pair"] * 3 + [MAT] + ["tail_split"] * 10, ["weights"] * 3 + ["deferred"] * 11,
     "tail"),
    ("weighted", 15, "weighted", ["weighted_pair"] * 4 + [MAT] + ["tail_split"] * 10, ["weights"] * 4 + ["deferred"] * 11,
     "tail"),
    # ipa_mat_n = 0: never materialised
    ("weighted_to_end", 13, "weighted", ["weighted_pair"] * 13, ["weights"] * 13, "weighted"),
    # ipa_tail = 0: G materialised affine at 2m = 2048 and folded from there
    ("weighted_fold_after", 12, "weighted", ["weighted_pair", "mat_affine>lr_msm"] + ["lr_msm"] * 10,
     ["weights"] + ["g"] * 11, "folded"),
    # ipa_srs_tail_n = n: the SRS's table from round 1, gs never filled
    ("srs_tail", 12, "srs_prefix", ["tail_srs>tail_split"] + ["tail_split"] * 11, ["deferred"] * 12, "tail"),
    ("srs_tail", 13, "srs_prefix", ["tail_srs>tail_split"] + ["tail_split"] * 12, ["deferred"] * 13, "tail"),
]


@pytest.mark.parametrize("mode,logn,begin,rounds,folds,end", MODE_TRACES, ids=["%s-%d" % c[:2] for c in MODE_TRACES])
def test_pinned_modes_take_their_paths(dump, mode, logn, begin, rounds, folds, end):
    got = trace(dump, logn, shifted=0 if mode == "fold" else 1, **mode_knobs(mode, 1 << logn))
    assert got == {"begin": begin, "rounds": rounds, "folds": folds, "end": end}


def test_default_paths(dump):
    # 2^12 <= ipa_srs_tail_n: the SRS's table from round 1
    assert trace(dump, 12) == {"begin": "srs_prefix", "rounds": ["tail_srs>tail_split"] + ["tail_split"] * 11,
                               "folds": ["deferred"] * 12, "end": "tail"}
    # 2^14: the derivation in this file's docstring
    assert trace(dump, 14) == {"begin": "weighted", "rounds": ["weighted_pair"] * 3 + [MAT] + ["tail_split"] * 10,
                               "folds": ["weights"] * 3 + ["deferred"] * 11, "end": "tail"}
    # 2^20: 2^19 terms per side are still a pair MSM; nine weighted rounds down to 2m = 4096
    assert trace(dump, 20) == {"begin": "weighted", "rounds": ["weighted_pair"] * 9 + [MAT] + ["tail_split"] * 10,
                               "folds": ["weights"] * 9 + ["deferred"] * 11, "end": "tail"}


def test_other_paths(dump):
    # n0 <= TAIL_FUSE_N: the fused tail round
    assert trace(dump, 8)["rounds"] == ["tail_srs>tail_fused"] + ["tail_fused"] * 7
    # above ipa_pair_max: two MSMs, on two streams when the session advances alone
    assert trace(dump, 13, pair_max=0, solo=1)["rounds"][:2] == ["weighted_two_streams"] * 2
    assert trace(dump, 13, pair_max=0, solo=0)["rounds"][:2] == ["weighted_one_stream"] * 2
    # no shifted copies: no weighted rounds, plain MSMs over the copied prefix
    assert trace(dump, 13, shifted=0)["rounds"][:3] == ["lr_msm", "lr_msm", OWN]
    # the SRS table is off for the tail start (ipa_srs_tail_n = 0) but serves a session of n <= IPA_TAIL_N
    assert trace(dump, 11, srs_tail_n=0) == {"begin": "srs_prefix", "rounds": ["tail_srs>tail_split"] + ["tail_split"] * 10,
                                             "folds": ["deferred"] * 11, "end": "tail"}
    # explicit G: folded every round, whatever the tunings
    assert trace(dump, 13, explicit=1) == {"begin": "folded+copy_gs", "rounds": ["lr_msm"] * 13, "folds": ["g"] * 13,
                                           "end": "folded"}
