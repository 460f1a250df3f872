"""Times the combined Schnorr batch (halo_schnorr_verify_combined_dev: one MSM of 2 k + 1 terms under random weights)
against the exact call (halo_schnorr_verify_batch_dev: k ladders) on Pallas with 10-element messages, inputs built as
tools/bench_schnorr.py builds them (64 distinct signatures from the CPU restatement, tiled to the batch size).

    python tools/bench_schnorr_combined.py [--sizes 40000,1048576] [--runs 10] [--warmup 2] [--out FILE]

Modes, alternated within every round so that drift hits all of them alike (a round = each mode once; the first
`warmup` rounds are dropped, the median of the other `runs` is reported beside their minimum and maximum):
  a  exact            halo_schnorr_verify_batch_dev, inputs resident, device events
  b  combined_rho     halo_schnorr_verify_combined_dev with the caller's weights, inputs resident, device events
  c  combined_fs      ... with derived weights (d_rho NULL), inputs resident, device events
  d  host_one_wrong   halo_schnorr_verify_combined on host arrays with one wrong signature: the uploads, the combined
                      pass, the exact ladder over the e already on the device, the verdicts' download; host clock
  e  host_exact       halo_schnorr_verify_batch on the same host arrays (what d's uploads alone cost shows here)
After the timed rounds, b and c run under the library's profile scopes (halo_profile_*) in a pass of their own: the
split into hashing, liveness, derivation (leaves, levels, weights), preparation, MSM and finish, in ms per call.
Every verdict is checked.  Prints one JSON line and writes it to --out (default profiles/schnorr_combined_bench.json).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from bench_schnorr import MSG_LEN, signatures  # noqa: E402
from halo_amd import _lib as H  # noqa: E402
from halo_amd import schnorr  # noqa: E402

SCOPES = ["sig_hash", "sig_live", "sig_rho", "sig_leaves", "rho_level", "sig_weights", "sig_prepare", "sig_sum", "sig_msm",
          "sig_finish"]


def tile_host(a, n):
    reps = (n + len(a) - 1) // len(a)
    return np.ascontiguousarray(np.tile(a, (reps, 1))[:n])


def dev(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def rand_rho(k, seed):
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)  # below 2^254: below the modulus
    return a


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms, n):
    med = float(np.median(ms))
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "sigs_per_s": round(n / med * 1e3)}


def profile_split(L, fn, calls=3):
    """ms per call under each scope (a stage's span includes the launches timed inside it)."""
    H.check(L.halo_profile_reset())
    H.check(L.halo_profile_enable(1))
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = {}
    for name in SCOPES:
        cnt, ms = ctypes.c_size_t(0), ctypes.c_double(0.0)
        if L.halo_profile_read(name.encode(), ctypes.byref(cnt), ctypes.byref(ms)) == 0 and cnt.value:
            out[name] = {"ms_per_call": round(ms.value / calls, 4), "launches_per_call": cnt.value / calls}
    H.check(L.halo_profile_enable(0))
    H.check(L.halo_profile_reset())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40000,1048576")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schnorr_combined_bench.json"))
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    pk, R, s, msgs = signatures(64)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    res = {"workload": "schnorr_verify_combined", "curve": "pallas", "msg_len": MSG_LEN, "runs": a.runs, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in [int(x) for x in a.sizes.split(",")]:
        h_pk, h_R, h_s, h_m = tile_host(pk, n), tile_host(R, n), tile_host(s, n), tile_host(msgs, n)
        h_rho = rand_rho(n, n)
        d_pk, d_R, d_s, d_m, d_rho = dev(h_pk), dev(h_R), dev(h_s), dev(h_m), dev(h_rho)
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_comb = torch.zeros(1, dtype=torch.uint8, device="cuda")
        wrong = n // 3
        h_s_bad = h_s.copy()
        h_s_bad[wrong, 0] ^= np.uint64(1)  # another scalar below the modulus: one wrong signature
        h_ok = np.zeros(n, dtype=np.uint8)
        h_comb = np.zeros(1, dtype=np.uint8)
        ins = (dp(d_pk), dp(d_R), dp(d_s), dp(d_m), MSG_LEN, n)
        host_ins = (H.ptr(h_pk), H.ptr(h_R), H.ptr(h_s_bad), H.ptr(h_m), MSG_LEN, n)

        def exact():
            H.check(L.halo_schnorr_verify_batch_dev(H.PALLAS, *ins, dp(d_ok), sp))

        def combined_rho():
            H.check(L.halo_schnorr_verify_combined_dev(H.PALLAS, *ins, dp(d_rho), dp(d_ok), dp(d_comb), sp))

        def combined_fs():
            H.check(L.halo_schnorr_verify_combined_dev(H.PALLAS, *ins, None, dp(d_ok), dp(d_comb), sp))

        def host_one_wrong():
            H.check(L.halo_schnorr_verify_combined(H.PALLAS, *host_ins, H.ptr(h_rho), H.ptr(h_ok), H.ptr(h_comb)))

        def host_exact():
            H.check(L.halo_schnorr_verify_batch(H.PALLAS, *host_ins, H.ptr(h_ok)))

        modes = [("exact", exact, event_ms), ("combined_rho", combined_rho, event_ms), ("combined_fs", combined_fs, event_ms),
                 ("host_one_wrong", host_one_wrong, wall_ms), ("host_exact", host_exact, wall_ms)]
        # every verdict, once, before anything is timed
        for name, fn, _ in modes[:3]:
            d_ok.zero_()
            d_comb.zero_()
            fn()
            torch.cuda.synchronize()
            assert bool((d_ok == 1).all()), f"{name}: a valid signature was rejected"
            assert name == "exact" or int(d_comb.cpu()[0]) == 1, name
        want = np.ones(n, dtype=np.uint8)
        want[wrong] = 0
        for name, fn, _ in modes[3:]:
            h_ok[:] = 7
            h_comb[:] = 7
            fn()
            assert np.array_equal(h_ok, want), f"{name}: verdicts"
            assert name == "host_exact" or int(h_comb[0]) == 0, name
        ms = {name: [] for name, _, _ in modes}
        for rnd in range(a.warmup + a.runs):
            for name, fn, clock in modes:
                t = clock(fn)
                if rnd >= a.warmup:
                    ms[name].append(t)
        entry = {name: summary(v, n) for name, v in ms.items()}
        for name in ("combined_rho", "combined_fs"):
            entry[name]["vs_exact"] = round(entry["exact"]["ms_median"] / entry[name]["ms_median"], 3)
        entry["msm_terms"] = 2 * n + 1
        entry["profile_combined_rho"] = profile_split(L, combined_rho)
        entry["profile_combined_fs"] = profile_split(L, combined_fs)
        res["sizes"][str(n)] = entry
        del d_pk, d_R, d_s, d_m, d_rho, d_ok, d_comb
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
