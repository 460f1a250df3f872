"""Times pcdl::open in one call with its transcript on the device (halo_pcdl_open_fs_dev_multi / halo_pcdl_open_fs)
on Pallas over a synthesized SRS, for plain openings at n = 2^10, 2^16 and 2^20 and k = 1 and 2 openings side by
side, beside the two host-driven loops the repository had.  DESIGN §4.10 records the numbers.

    python tools/bench_pcdl_open_fs.py [--reps 10] [--lgs 10,16,20] [--prover-lg 16] [--out FILE]

All in one session on one device, wall time of the whole call (each ends with the proof on the host):
  (a) the new call: open_device_many over k device-resident polynomials (every opening's chain enqueued before any
      is waited for), with the sponge's lane layout pinned to 3 and to 1, and for k = 1 also the host-array call;
      the transcript kernel's own time per round from the library's profiling hooks (open_fs_round);
  (b) the host-driven lockstep loop with stand-in challenges (prover.ipa_open_many, the benchmarked prover's path:
      one host trip per round, a sponge that costs nearly nothing) -- the floor of a host-driven opening;
  (c) the host-driven loop under the restated Poseidon sponge (pcdl.open_without_eval with oracle/poseidon.py), until
      now the only way to a reference-valid proof from Python; k = 2 is two calls in a row (no lockstep form exists);
and naive_prover under transcripts at n = 2^prover-lg on DeviceBackend with and without device_transcripts (a
synthetic witness: the work is that of a satisfiable one).  (a) and (c) give the same proof, which is asserted.
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
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import pasta as P  # noqa: E402
import poseidon  # noqa: E402
from halo_amd import _lib as H  # noqa: E402
from halo_amd import group, pcdl, prover, schnorr  # noqa: E402

from bench_pcdl_check import dev, scalars, wall  # noqa: E402

LABELS = {"PCDL": poseidon.PCDL, "ASDL": poseidon.ASDL, "PLONK": poseidon.PLONK}


class OracleSponge:
    """oracle/poseidon.py behind the reference's Sponge interface, over WrappedPoints / ark scalars."""

    def __init__(self, cname, label="PCDL"):
        self.c = P.CURVES[cname]
        self.s = poseidon.Sponge(cname, LABELS[label])

    def absorb_g(self, pts):
        self.s.absorb_g([P.wrapped_to_point(self.c, [int(x) for x in q]) for q in pts])

    def absorb_fr(self, xs):
        self.s.absorb_fr([P.from_mont(P.limbs_to_int(x), self.c.scalar) for x in xs])

    def challenge(self):
        return np.array(P.int_to_limbs(P.to_mont(self.s.challenge(), self.c.scalar)), dtype=np.uint64)


def round_kernel_ms(L, fn, calls, rounds):
    """The transcript kernel's own time per round (mean over `calls` calls of `rounds` rounds in all)."""
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    L.halo_profile_enable(0)
    n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
    H.check(L.halo_profile_read(b"open_fs_round", ctypes.byref(n), ctypes.byref(ms)))
    L.halo_profile_reset()
    return round(ms.value / max(n.value, 1), 5), n.value == calls * rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lgs", default="10,16,20")
    ap.add_argument("--prover-lg", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    cname = "pallas"
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    tr = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, tr[f"poseidon_{f}_mds"], tr[f"poseidon_{f}_rc"])
    S, Hh = g[f"ref_sh_{cname}"]
    lgs = [int(x) for x in a.lgs.split(",")]
    group.PublicParams.upload(cname, g[f"ref_srs_{cname}_b00_first64"], S, Hh, precompute_windows=False)  # installs (S, H)
    group.PublicParams.synthesize(cname, 1 << max(lgs + [a.prover_lg]), 7, precompute_windows=True)
    rng = np.random.default_rng(14)
    res = {"workload": "pcdl_open_fs", "curve": cname, "reps": a.reps, "device": torch.cuda.get_device_name(0), "lg_n": {}}
    B = prover.DeviceBackend(cname)
    for lg in lgs:
        n, d = 1 << lg, (1 << lg) - 1
        ps = [scalars(rng, n) for _ in range(2)]
        zs = scalars(rng, 2)
        d_ps = [dev(p).reshape(n, 4) for p in ps]
        Cs = np.stack([pcdl.commit(p, d, curve=cname) for p in ps])
        reps = a.reps if lg <= 16 else max(3, a.reps // 2)
        out_lg = {}
        for k in (1, 2):
            e = {}
            for lanes in (3, 1):
                with H.tuning(poseidon_lanes=lanes):
                    fn = lambda: pcdl.open_device_many(d_ps[:k], Cs[:k], d, zs[:k], curve=cname)  # noqa: E731
                    e[f"a_device_transcript_lanes{lanes}"] = wall(fn, reps)
                    per_round, counted = round_kernel_ms(L, fn, 3, k * lg)
                    e[f"a_round_kernel_ms_lanes{lanes}"] = per_round if counted else None
            if k == 1:
                e["a_host_arrays"] = wall(lambda: pcdl.open_device(ps[0], Cs[0], d, zs[0], curve=cname), reps)
            items = [(d_ps[i], B.to_int(zs[i]), 0) for i in range(k)]
            e["b_host_loop_stand_in"] = wall(lambda: prover.ipa_open_many(B, items, d), reps)
            c_reps = 3 if lg >= 16 else reps

            def host_sponge():
                return [pcdl.open(ps[i], Cs[i], d, zs[i], transcript=OracleSponge(cname), curve=cname) for i in range(k)]

            e["c_host_loop_poseidon"] = wall(host_sponge, c_reps, warmup=1)
            got = pcdl.open_device_many(d_ps[:k], Cs[:k], d, zs[:k], curve=cname)
            for x, y in zip(got, host_sponge()):
                assert all(np.array_equal(np.stack(x[f]), np.stack(y[f])) for f in ("Ls", "Rs", "U", "c", "v")), "proofs differ"
            out_lg[str(k)] = e
        res["lg_n"][str(lg)] = out_lg
        del d_ps
    # the prover under transcripts, with and without the PCDL sponges on the device
    n = 1 << a.prover_lg
    pr = {}
    for devt in (False, True):
        Bt = prover.DeviceBackend(cname, device_transcripts=devt)
        wit = prover.synthetic_witness(Bt, n, seed=1)
        nt = lambda label: OracleSponge(cname, label)  # noqa: E731
        p0 = Bt.random_vec(n, np.random.default_rng(2))
        acc_prev = Bt.acc_prove([Bt.instance_open(p0, n - 1, 12345, nt)], n - 1, nt)
        runs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = prover.naive_prover(Bt, wit, n, None, acc_prev=acc_prev, transcript=nt)
            torch.cuda.synchronize()
            runs.append(((time.perf_counter() - t0) * 1e3, out["times"]["r5_open"] * 1e3, out["times"]["r5_acc"] * 1e3))
        best = min(runs[1:])
        pr["device_transcripts" if devt else "host_sponges"] = {
            "total_ms": round(best[0], 3), "r5_open_ms": round(best[1], 3), "r5_acc_ms": round(best[2], 3)}
    res["naive_prover_lg%d" % a.prover_lg] = pr
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
