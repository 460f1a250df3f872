"""Times the Fiat-Shamir sponge handles (halo_sponge_*, halo_amd.sponge) and the prover's PLONK transcript on them,
Pallas, in one session.  DESIGN §4.12 records the numbers.

    python tools/bench_sponge.py [--reps 10] [--ks 1,64,4096] [--naive-lgs 10,16] [--out profiles/sponge_bench.json]

The PLONK prover transcript as calls -- absorb_g of 16, two challenges, absorb_g of 1, one challenge, absorb_g of 16,
two challenges: 34 permutations per sponge -- on a SpongeBatch of k, medians of --reps after warm-ups:
  * the host-array forms (wall time: each call copies in, runs and waits);
  * the _dev forms (event time on the stream, and wall time with one wait at the end);
  * the kernels' own time and the permutation count from the library's profiling hooks;
  * for k = 1, the same transcript through the Python restatement (tests/plonk_ref.SpongeAdapter), and that the two
    give the same five challenges.
naive_prover under transcripts at n = 2^lg on DeviceBackend(device_transcripts=True, device_acc=True) with device_plonk
off (the PLONK sponge is the restatement's, in Python) and on, alternated, --reps runs each after a warm-up: the medians,
each one's spread (max - min) and whether on is not slower than off by more than that spread.
Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from halo_amd import _lib as H  # noqa: E402
from halo_amd import group, prover, schnorr, sponge  # noqa: E402

from bench_pcdl_check import dev, timed, wall  # noqa: E402

SCHEDULE = ((16, 2), (1, 1), (16, 2))  # points absorbed, challenges drawn


def transcript_host(s, pts):
    out, at = [], 0
    for count, draws in SCHEDULE:
        s.absorb_g(pts[:, at:at + count])
        at += count
        out.append(s.challenge(draws))
    return np.concatenate(out, axis=1)


def transcript_dev(s, d_pts):
    out = []
    for j, (_, draws) in enumerate(SCHEDULE):
        s.absorb_g_dev(d_pts[j])
        out.append(s.challenge_dev(draws))
    return out


def profile(L, fn, launches):
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    L.halo_profile_enable(0)
    out = {}
    for name in ("sponge_absorb", "sponge_challenge", "sponge_permutations"):
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        H.check(L.halo_profile_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        out[name] = {"count_per_call": n.value / launches, "kernel_ms_per_call": round(ms.value / launches, 4)}
    L.halo_profile_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", default="1,64,4096")
    ap.add_argument("--naive-lgs", default="10,16")
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = a.reps
    H.ensure_device(0)
    L = H.load()
    cname = "pallas"
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    tr = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, tr[f"poseidon_{f}_mds"], tr[f"poseidon_{f}_rc"])
    base = g[f"ref_srs_{cname}_b00_first64"]
    S, Hh = g[f"ref_sh_{cname}"]
    rng = np.random.default_rng(21)
    res = {"workload": "sponge", "curve": cname, "reps": reps, "device": torch.cuda.get_device_name(0),
           "transcript": "absorb_g 16, 2 challenges, absorb_g 1, 1 challenge, absorb_g 16, 2 challenges", "k": {}}

    for k in [int(x) for x in a.ks.split(",") if x]:
        pts = np.ascontiguousarray(base[rng.integers(0, 64, size=(k, 33))])
        d_pts = [dev(np.ascontiguousarray(pts[:, lo:hi])) for lo, hi in ((0, 16), (16, 17), (17, 33))]

        def host():
            with sponge.SpongeBatch(cname, "PLONK", k) as s:
                return transcript_host(s, pts)

        def on_dev():
            with sponge.SpongeBatch(cname, "PLONK", k) as s:
                return transcript_dev(s, d_pts)

        # the handle's own cost (new: one launch and a wait; free: hipFree) is in both; measured alone too
        def handle_only():
            sponge.SpongeBatch(cname, "PLONK", k).close()

        s = sponge.SpongeBatch(cname, "PLONK", k)

        def calls_only():  # one long-lived handle (the transcripts follow one another): seven _dev calls, one wait
            out = transcript_dev(s, d_pts)
            torch.cuda.synchronize()
            return out

        def fresh_dev():
            on_dev()
            torch.cuda.synchronize()

        e = {"host_forms": wall(host, reps), "dev_forms_wall": wall(fresh_dev, reps),
             "dev_forms_calls_only_event": timed(lambda: transcript_dev(s, d_pts), reps),
             "dev_forms_calls_only_wall": wall(calls_only, reps), "handle_new_free_wall": wall(handle_only, reps),
             "kernels": profile(L, fresh_dev, 3)}
        got_h, got_d = host(), torch.cat(on_dev(), dim=1).cpu().numpy().view(np.uint64)
        assert np.array_equal(got_h, got_d), "host and _dev forms differ"
        if k == 1:
            import plonk_ref as R

            def restated():
                t, out, at = R.SpongeAdapter(cname, "PLONK"), [], 0
                for count, draws in SCHEDULE:
                    t.absorb_g(pts[0, at:at + count])
                    at += count
                    out += [t.challenge() for _ in range(draws)]
                return np.stack(out)

            e["python_restatement"] = wall(restated, reps)
            assert np.array_equal(restated(), got_h[0]), "the device sponge differs from the restatement"
        s.close()
        res["k"][str(k)] = e

    nt = None
    for lg in [int(x) for x in a.naive_lgs.split(",") if x]:
        import plonk_ref as R
        nt = R.new_transcript(cname)
        n = 1 << lg
        group.PublicParams.upload(cname, base, S, Hh, precompute_windows=False)  # installs (S, H)
        group.PublicParams.synthesize(cname, n, 7, precompute_windows=True)
        Bs = {flag: prover.DeviceBackend(cname, device_transcripts=True, device_acc=True, device_plonk=flag) for flag in (False, True)}
        wit = prover.synthetic_witness(Bs[False], n, seed=1)
        p0 = Bs[False].random_vec(n, np.random.default_rng(2))
        acc_prev = Bs[False].acc_prove([Bs[False].instance_open(p0, n - 1, 12345, nt)], n - 1, nt)
        runs = {False: [], True: []}
        outs = {}
        for rep in range(reps + 1):  # the first pair warms up
            for flag in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[flag] = prover.naive_prover(Bs[flag], wit, n, None, acc_prev=acc_prev, transcript=nt)
                torch.cuda.synchronize()
                if rep:
                    runs[flag].append((time.perf_counter() - t0) * 1e3)
        assert all(np.array_equal(x, y) for x, y in zip(outs[True]["C_ts"], outs[False]["C_ts"])) and \
            outs[True]["vs"] == outs[False]["vs"], "device_plonk changes the proof"
        off, on = runs[False], runs[True]
        spread = max(max(off) - min(off), max(on) - min(on))
        res["naive_prover_lg%d" % lg] = {
            "device_plonk_off_ms_median": round(float(np.median(off)), 3), "device_plonk_on_ms_median": round(float(np.median(on)), 3),
            "off_ms_min_max": [round(min(off), 3), round(max(off), 3)], "on_ms_min_max": [round(min(on), 3), round(max(on), 3)],
            "spread_ms": round(spread, 3), "on_not_slower_within_spread": bool(np.median(on) <= np.median(off) + spread)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
