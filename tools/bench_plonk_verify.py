"""Times PlonkProof::verify_succinct on the device (halo_plonk_verify_succinct_batch) on Pallas over a synthesized
SRS, at lg n = 16 (the IVC circuits' rows) and 20 for k = 1, 64 and 4096 proofs, and in the same run
halo_pcdl_succinct_check_fs_batch alone over the same 3 k instances: the part the library had before, so the
Plonk-specific stages are the difference.  DESIGN §4.8 records the numbers.

    python tools/bench_plonk_verify.py [--reps 10] [--ks 1,64,4096] [--lgs 16,20] [--out FILE]

Per lg n and k:
  * the wall time of the host-array call (median of --reps >= 10 after 2 warm-ups) and of
    halo_pcdl_succinct_check_fs_batch over the 3 k instances;
  * the event-timed median of the _dev call (inputs resident);
  * the per-stage split: each kernel's own time from the library's profiling hooks, mean over the launches.
The proofs are synthetic -- random scalars over tiled SRS points -- so every verdict is a rejection; no
kernel's path depends on the verdict, so the work is that of an accepting batch.  Prints one JSON line (and
writes it to --out).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from halo_amd import _lib as H  # noqa: E402
from halo_amd import group, schnorr  # noqa: E402

from bench_pcdl_check import dev, scalars, timed, wall  # noqa: E402

STAGES = ("plonk_points", "plonk_challenges", "plonk_identity", "pcdl_challenges", "pcdl_terms", "asdl_challenges",
          "asdl_terms", "lincomb_terms", "lincomb_sum")
NPI = 4


def stage_ms(L, fn, launches):
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    L.halo_profile_enable(0)
    out = {}
    for name in STAGES:
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        H.check(L.halo_profile_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        if n.value:
            out[name + "_ms_per_call"] = round(ms.value / launches, 4)
    L.halo_profile_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", default="1,64,4096")
    ap.add_argument("--lgs", default="16,20")
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(a.reps, 10)
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    tr = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, tr[f"poseidon_{f}_mds"], tr[f"poseidon_{f}_rc"])
    base = g["ref_srs_pallas_b00_first64"]
    S, Hh = g["ref_sh_pallas"]
    lgs = [int(x) for x in a.lgs.split(",")]
    group.PublicParams.upload("pallas", base, S, Hh, precompute_windows=False)  # installs (S, H)
    group.PublicParams.synthesize("pallas", 1 << max(lgs), 7, precompute_windows=False)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.default_rng(13)
    tile = lambda n, off=0: np.ascontiguousarray(np.tile(base, ((n + off + 63) // 64, 1))[off:n + off])  # noqa: E731
    res = {"workload": "plonk_verify_succinct", "curve": "pallas", "reps": reps, "public_inputs": NPI,
           "device": torch.cuda.get_device_name(0), "lg_n": {}}
    for lg in lgs:
        rows = 1 << lg
        out_lg = {}
        for k in [int(x) for x in a.ks.split(",")]:
            ins = [tile(10), scalars(rng, k * NPI), tile(k * 16, 1), tile(k, 2), tile(k * 16, 3), scalars(rng, k * 78),
                   tile(k * 3 * lg, 4), tile(k * 3 * lg, 5), tile(k * 3, 6), scalars(rng, k * 3), tile(k, 7), scalars(rng, k),
                   scalars(rng, k), tile(k, 8), scalars(rng, k), scalars(rng, k), scalars(rng, 9)]
            verdict = np.zeros(k, dtype=np.uint8)
            d_in = [dev(x) for x in ins]
            d_verdict = torch.zeros(k, dtype=torch.uint8, device="cuda")
            # the same 3 k instances for the succinct check alone: C, z, v of its own, the proofs' Ls, Rs, U, c
            fs_in = [tile(3 * k, 9), scalars(rng, 3 * k), scalars(rng, 3 * k), ins[6], ins[7], ins[8], ins[9]]
            ok = np.zeros(3 * k, dtype=np.uint8)

            def plonk_host():
                p = [H.ptr(x) for x in ins]
                H.check(L.halo_plonk_verify_succinct_batch(H.PALLAS, rows, k, p[0], p[1], NPI, *p[2:], H.ptr(verdict), None,
                                                           None, None))

            def plonk_dev():
                p = [dp(t) for t in d_in]
                H.check(L.halo_plonk_verify_succinct_batch_dev(H.PALLAS, rows, k, p[0], p[1], NPI, *p[2:], dp(d_verdict), None,
                                                               None, None, sp))

            def fs_host():
                H.check(L.halo_pcdl_succinct_check_fs_batch(H.PALLAS, rows - 1, 3 * k, *[H.ptr(x) for x in fs_in], None, None,
                                                            None, None, None, H.ptr(ok)))

            launches = reps if k <= 64 else max(3, reps // 3)
            entry = {"plonk_host": wall(plonk_host, reps), "pcdl_fs_host_3k_instances": wall(fs_host, reps),
                     "plonk_dev": timed(plonk_dev, reps), "stages": stage_ms(L, plonk_dev, launches)}
            entry["plonk_specific_wall_ms"] = round(entry["plonk_host"]["wall_ms_median"] -
                                                    entry["pcdl_fs_host_3k_instances"]["wall_ms_median"], 4)
            entry["verdicts_all_reject"] = bool((verdict != 0).all())
            out_lg[str(k)] = entry
            del d_in, d_verdict
        res["lg_n"][str(lg)] = out_lg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
