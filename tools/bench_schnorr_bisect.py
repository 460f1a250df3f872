"""Measures the descent below a rejected combined Schnorr batch (halo_amd/csrc/schnorr_bisect.hip) on Pallas with
10-element messages, inputs built as tools/bench_schnorr.py builds them (64 distinct signatures from the CPU
restatement, tiled to the batch size; a wrong item is a valid one with the low bit of s flipped).

    python tools/bench_schnorr_bisect.py [--sizes 40000,1048576] [--runs 10] [--warmup 2] [--out FILE]
                                         [--pass-items C] [--leaf L] [--skip-crossover]

Two parts, each of `warmup` dropped rounds and `runs` kept ones; the median is reported beside the minimum and maximum.

  crossover   for m = 2^10 .. 2^18: one pass over the left half (m items) of a node of 2 m items against the ladder
              over m items, both inside ONE halo_schnorr_verify_bisect_dev call per round: a batch of 2 m items, resident,
              whose last item is wrong, under schnorr_bisect_leaf = m, schnorr_bisect_pass_items = 1, so that the root
              takes one pass (node scalars, comb, MSM, split) and its failing right half, m items, goes to the ladder.
              Device events of the library's profile scopes (halo_profile_*): pass = sig_bisect_pass + sig_split, ladder =
              sig_bisect_ladder.  The level's host wait (the flags' download) is not in the pass; the whole call is timed
              beside it by device events.  c is the smallest power of two m from which pass <= ladder holds (medians) at
              every larger m measured (crossover_c; crossover_first_m is the first m at which it holds at all: below
              the crossover both sit on their latency floors and trade places), L = 2 c.
  rejected    halo_schnorr_verify_combined on host arrays (host clock: the uploads, the combined pass, the resolution,
              the verdicts' download) with the tuning key schnorr_bisect = 0 and 1 alternated within every round, at
              each size, with b = 1, 16, 1024 wrong items spread evenly and with every second item wrong, under
              schnorr_bisect_pass_items = c and schnorr_bisect_leaf = L: --pass-items / --leaf, else the crossover's,
              else (--skip-crossover) the library's defaults.
Every verdict is checked.  Prints one JSON line and writes it to --out (default profiles/schnorr_bisect_bench.json).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from bench_schnorr import MSG_LEN, signatures  # noqa: E402
from bench_schnorr_combined import dev, event_ms, rand_rho, tile_host, wall_ms  # noqa: E402
from halo_amd import _lib as H  # noqa: E402
from halo_amd import schnorr  # noqa: E402

PASS_SCOPES = ("sig_bisect_pass", "sig_split")
LADDER_SCOPE = "sig_bisect_ladder"


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def read_scope(L, name):
    cnt, ms = ctypes.c_size_t(0), ctypes.c_double(0.0)
    H.check(L.halo_profile_read(name.encode(), ctypes.byref(cnt), ctypes.byref(ms)))
    return cnt.value, ms.value


def crossover(L, base, sp, runs, warmup):
    pk, R, s, msgs = base
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = {}
    for lg in range(10, 19):
        m = 1 << lg
        n = 2 * m
        h_s = tile_host(s, n)
        h_s[n - 1, 0] ^= np.uint64(1)
        d_pk, d_R, d_s, d_m, d_rho = dev(tile_host(pk, n)), dev(tile_host(R, n)), dev(h_s), dev(tile_host(msgs, n)), dev(rand_rho(n, n))
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_comb = torch.zeros(1, dtype=torch.uint8, device="cuda")
        want = np.ones(n, dtype=np.uint8)
        want[n - 1] = 0

        def call():
            H.check(L.halo_schnorr_verify_bisect_dev(H.PALLAS, dp(d_pk), dp(d_R), dp(d_s), dp(d_m), MSG_LEN, n, dp(d_rho), dp(d_ok),
                                                     dp(d_comb), sp))

        ms = {"pass": [], "ladder": [], "call": []}
        with H.tuning(schnorr_bisect_leaf=m, schnorr_bisect_pass_items=1):
            for rnd in range(warmup + runs):
                d_ok.fill_(7)
                H.check(L.halo_profile_reset())
                H.check(L.halo_profile_enable(1))
                t_call = event_ms(call)
                got = d_ok.cpu().numpy()
                assert np.array_equal(got, want) and int(d_comb.cpu()[0]) == 0, f"crossover m = {m}: verdicts"
                t_pass = 0.0
                for name in PASS_SCOPES:
                    cnt, t = read_scope(L, name)
                    assert cnt == 1, (name, cnt)
                    t_pass += t
                cnt, t_ladder = read_scope(L, LADDER_SCOPE)
                assert cnt == 1, (LADDER_SCOPE, cnt)
                H.check(L.halo_profile_enable(0))
                H.check(L.halo_profile_reset())
                if rnd >= warmup:
                    ms["pass"].append(t_pass)
                    ms["ladder"].append(t_ladder)
                    ms["call"].append(t_call)
        out[str(m)] = {"pass": stats(ms["pass"]), "ladder": stats(ms["ladder"]), "call": stats(ms["call"]), "msm_terms": 2 * m,
                       "ladder_ns_per_item": round(float(np.median(ms["ladder"])) * 1e6 / m, 1)}
        del d_pk, d_R, d_s, d_m, d_rho, d_ok, d_comb
    holds = [(int(m), out[m]["pass"]["ms_median"] <= out[m]["ladder"]["ms_median"]) for m in out]
    first = next((m for m, h in holds if h), None)
    # the crossover proper: from there on the pass stays below the ladder at every larger m measured.  Below it both
    # sit on their latency floors (one wave's ladder, the MSM's tail), where the comparison is noise and the ladder is
    # far from linear in its items, which is what the budget rule's c assumes.
    stable = next((m for j, (m, _) in enumerate(holds) if all(h for _, h in holds[j:])), None)
    return out, first, stable


def rejected(L, base, n, c, leaf, runs, warmup):
    pk, R, s, msgs = base
    h_pk, h_R, h_s, h_m = tile_host(pk, n), tile_host(R, n), tile_host(s, n), tile_host(msgs, n)
    h_rho = rand_rho(n, n)
    h_ok = np.zeros(n, dtype=np.uint8)
    h_comb = np.zeros(1, dtype=np.uint8)
    out = {}
    cases = [("b1", np.array([n // 3])), ("b16", np.arange(16) * (n // 16) + n // 32), ("b1024", np.arange(1024) * (n // 1024) + n // 2048),
             ("every_second", np.arange(0, n, 2))]
    for name, wrong in cases:
        h_bad = h_s.copy()
        h_bad[wrong, 0] ^= np.uint64(1)  # another scalar below the modulus
        want = np.ones(n, dtype=np.uint8)
        want[wrong] = 0
        ins = (H.ptr(h_pk), H.ptr(h_R), H.ptr(h_bad), H.ptr(h_m), MSG_LEN, n)

        def call():
            H.check(L.halo_schnorr_verify_combined(H.PALLAS, *ins, H.ptr(h_rho), H.ptr(h_ok), H.ptr(h_comb)))

        ms = {0: [], 1: []}
        with H.tuning(schnorr_bisect_leaf=leaf, schnorr_bisect_pass_items=c):
            for rnd in range(warmup + runs):
                for key in (0, 1):
                    h_ok[:] = 7
                    with H.tuning(schnorr_bisect=key):
                        t = wall_ms(call)
                    assert np.array_equal(h_ok, want) and int(h_comb[0]) == 0, f"{name} key {key}: verdicts"
                    if rnd >= warmup:
                        ms[key].append(t)
        e = {"wrong": int(len(wrong)), "key0": stats(ms[0]), "key1": stats(ms[1])}
        e["key1_over_key0"] = round(e["key1"]["ms_median"] / e["key0"]["ms_median"], 3)
        out[name] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40000,1048576")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pass-items", type=int)
    ap.add_argument("--leaf", type=int)
    ap.add_argument("--skip-crossover", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schnorr_bisect_bench.json"))
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    base = signatures(64)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"workload": "schnorr_verify_bisect", "curve": "pallas", "msg_len": MSG_LEN, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0),
           "library_defaults": {"schnorr_bisect_pass_items": H.get_tuning("schnorr_bisect_pass_items"),
                                "schnorr_bisect_leaf": H.get_tuning("schnorr_bisect_leaf")}}
    c = None
    if not a.skip_crossover:
        res["crossover"], first, c = crossover(L, base, sp, a.runs, a.warmup)
        res["crossover_first_m"] = first
        res["crossover_c"] = c
    c = a.pass_items or c or H.get_tuning("schnorr_bisect_pass_items")
    leaf = a.leaf or 2 * c
    res["rejected_keys"] = {"schnorr_bisect_pass_items": c, "schnorr_bisect_leaf": leaf}
    res["rejected"] = {str(n): rejected(L, base, n, c, leaf, a.runs, a.warmup) for n in [int(x) for x in a.sizes.split(",")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
