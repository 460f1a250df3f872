"""Times the accumulation scheme in one call each (halo_acc_prover, halo_acc_verifier_batch and its _dev form) on
Pallas over a synthesized SRS.  DESIGN §4.11 records the numbers.

    python tools/bench_acc.py [--reps 20] [--prover-lgs 10,16,20] [--ms 1,3] [--ks 1,64,4096] [--verifier-lgs 16,20]
                              [--naive-lg 16] [--no-plonk] [--out profiles/acc_bench.json]

Prover, per lg n and m (valid instances made with pcdl.open_device_many; medians of --reps after warm-ups):
  * the wall time of the whole halo_acc_prover call (acc.prover_device);
  * its stages: each kernel's own time from the library's profiling hooks, summed per call (PCDL sponges, ASDL sponge,
    terms, the linear combinations, the h-combine, the opening's transcript kernel), and the wall time of the opening
    alone (pcdl.open_device_many over the same h on the device);
  * today's route in the same session: acc.prover(..., device_transcripts=True) under the restated Poseidon sponge.
    Both give the same accumulator, which is asserted.
Verifier, per lg n and k with m = 3 (synthetic instances -- random scalars over tiled SRS points -- so every verdict is
INSTANCE; no kernel's path depends on the verdict):
  * the event-timed median of the _dev call and the wall time of the host-array call;
  * the ASDL sponge and the terms kernels alone, and the ASDL sponge per permutation
    (ceil((1 + 2 m (lg n + 1) + 2 m) / 2) absorb permutations and two squeezes on Pallas).
naive_prover under transcripts at n = 2^naive-lg (0: skipped) on DeviceBackend(device_transcripts=True) with and
without device_acc (a synthetic witness: the work is that of a satisfiable one), best of the warm repetitions.
Unless --no-plonk: tools/bench_plonk_verify.py is run as a child in the same session for the same k and lg n, and its
asdl_challenges / asdl_terms stages are kept beside them.  Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from halo_amd import _lib as H  # noqa: E402
from halo_amd import acc, group, pcdl, prover, schnorr  # noqa: E402

from bench_pcdl_check import dev, scalars, timed, wall  # noqa: E402
from bench_pcdl_open_fs import OracleSponge  # noqa: E402

STAGES = ("pcdl_challenges", "pcdl_terms", "acc_challenges", "acc_terms", "lincomb_terms", "lincomb_sum", "acc_hpoly_combine",
          "open_fs_round")


def stage_ms(L, fn, launches):
    """Each named kernel's own time, summed over its launches in one call (mean over `launches` calls)."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prover-lgs", default="10,16,20")
    ap.add_argument("--ms", default="1,3")
    ap.add_argument("--ks", default="1,64,4096")
    ap.add_argument("--verifier-lgs", default="16,20")
    ap.add_argument("--naive-lg", type=int, default=16)
    ap.add_argument("--no-plonk", action="store_true")
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
    p_lgs = [int(x) for x in a.prover_lgs.split(",") if x]
    v_lgs = [int(x) for x in a.verifier_lgs.split(",") if x]
    ms = [int(x) for x in a.ms.split(",")]
    ks = [int(x) for x in a.ks.split(",")]
    rng = np.random.default_rng(15)
    nt = lambda label: OracleSponge(cname, label)  # noqa: E731
    res = {"workload": "acc", "curve": cname, "reps": reps, "device": torch.cuda.get_device_name(0), "prover": {}, "verifier": {}}

    # ---- the prover: the SRS is synthesized per lg n (an opening reads Gs[0 .. n))
    for lg in p_lgs:
        n, d = 1 << lg, (1 << lg) - 1
        group.PublicParams.upload(cname, base, S, Hh, precompute_windows=False)  # installs (S, H)
        group.PublicParams.synthesize(cname, n, 7, precompute_windows=True)
        mmax = max(ms)
        polys = [scalars(rng, n) for _ in range(mmax)]
        zs = scalars(rng, mmax)
        d_ps = [dev(p).reshape(n, 4) for p in polys]
        Cs = np.stack([pcdl.commit(p, d, curve=cname) for p in polys])
        pis = pcdl.open_device_many(d_ps, Cs, d, zs, curve=cname)
        insts = [pcdl.Instance(Cs[i], d, zs[i], pis[i]["v"], pis[i]) for i in range(mmax)]
        del d_ps
        out_lg = {}
        for m in ms:
            qs = insts[:m]
            new = lambda: acc.prover_device(qs, curve=cname)  # noqa: E731
            old = lambda: acc.prover(qs, nt, curve=cname, device_transcripts=True)  # noqa: E731
            e = {"halo_acc_prover": wall(new, reps), "stages": stage_ms(L, new, 3),
                 "today_device_transcripts_host_asdl": wall(old, reps if lg < 20 else max(5, reps // 4))}
            x, y = new(), old()
            assert np.array_equal(x.C, y.C) and np.array_equal(x.z, y.z) and np.array_equal(x.v, y.v), "accumulators differ"
            assert all(np.array_equal(np.stack(x.pi[f]), np.stack(y.pi[f])) for f in ("Ls", "Rs", "U", "c")), "proofs differ"
            # the opening alone: the same h, resident, through the entry point whose chain the prover shares
            _, _, _, hs, alphas = acc.common_subroutine_device(qs, curve=cname)
            d_h = dev(pcdl.HPoly.combine(hs, alphas)).reshape(-1, 4)
            e["opening_alone"] = wall(lambda: pcdl.open_device_many([d_h], x.C[None], d, x.z[None], curve=cname), reps)
            out_lg[str(m)] = e
            del d_h
        res["prover"][str(lg)] = out_lg

    # ---- the verifier, m = 3
    if v_lgs:
        group.PublicParams.upload(cname, base, S, Hh, precompute_windows=False)
        group.PublicParams.synthesize(cname, 1 << max(v_lgs), 7, precompute_windows=False)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    tile = lambda n, off=0: np.ascontiguousarray(np.tile(base, ((n + off + 63) // 64, 1))[off:n + off])  # noqa: E731
    m = 3
    for lg in v_lgs:
        d = (1 << lg) - 1
        out_lg = {}
        for k in ks:
            km = k * m
            ins = [tile(km, 9), scalars(rng, km), scalars(rng, km), tile(km * lg, 4), tile(km * lg, 5), tile(km, 6),
                   scalars(rng, km), None, None, None, tile(k, 8), scalars(rng, k), scalars(rng, k)]
            verdict = np.zeros(k, dtype=np.uint8)
            d_in = [dev(x) if x is not None else None for x in ins]
            d_verdict = torch.zeros(k, dtype=torch.uint8, device="cuda")

            def host():
                H.check(L.halo_acc_verifier_batch(H.PALLAS, d, k, m, *[H.ptr(x) for x in ins], H.ptr(verdict), None, None, None,
                                                  None))

            def on_dev():
                H.check(L.halo_acc_verifier_batch_dev(H.PALLAS, d, k, m, *[dp(t) if t is not None else None for t in d_in],
                                                      dp(d_verdict), None, None, None, None, sp))

            launches = reps if k <= 64 else max(3, reps // 3)
            e = {"verifier_host": wall(host, reps), "verifier_dev": timed(on_dev, reps), "stages": stage_ms(L, on_dev, launches)}
            perms = (1 + 2 * m * (lg + 1) + 2 * m + 1) // 2 + 2
            e["asdl_permutations"] = perms
            e["asdl_ms_per_permutation"] = round(e["stages"]["acc_challenges_ms_per_call"] / perms, 5)
            e["verdicts_all_instance"] = bool((verdict == acc.INSTANCE).all())
            out_lg[str(k)] = e
            del d_in, d_verdict
        res["verifier"][str(lg)] = out_lg

    # ---- naive_prover under transcripts: acc::prover's ASDL sponge in the caller's Python, and on the device
    if a.naive_lg:
        n = 1 << a.naive_lg
        group.PublicParams.upload(cname, base, S, Hh, precompute_windows=False)
        group.PublicParams.synthesize(cname, n, 7, precompute_windows=True)
        pr = {}
        for dev_acc in (False, True):
            Bt = prover.DeviceBackend(cname, device_transcripts=True, device_acc=dev_acc)
            wit = prover.synthetic_witness(Bt, n, seed=1)
            p0 = Bt.random_vec(n, np.random.default_rng(2))
            acc_prev = Bt.acc_prove([Bt.instance_open(p0, n - 1, 12345, nt)], n - 1, nt)
            runs = []
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = prover.naive_prover(Bt, wit, n, None, acc_prev=acc_prev, transcript=nt)
                torch.cuda.synchronize()
                runs.append(((time.perf_counter() - t0) * 1e3, out["times"]["r5_open"] * 1e3, out["times"]["r5_acc"] * 1e3))
            best = min(runs[1:])
            pr["device_acc" if dev_acc else "host_asdl"] = {
                "total_ms": round(best[0], 3), "r5_open_ms": round(best[1], 3), "r5_acc_ms": round(best[2], 3)}
        res["naive_prover_lg%d" % a.naive_lg] = pr

    # ---- the Plonk verifier's asdl stages (the same kernels with m = 3 inside its chain), as a child in this session
    if not a.no_plonk and v_lgs:
        child = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_plonk_verify.py"), "--reps", str(max(reps, 10)),
                                "--ks", a.ks, "--lgs", a.verifier_lgs], capture_output=True, text=True, check=True,
                               timeout=600)  # a hung child ends the job
        pv = json.loads(child.stdout.strip().splitlines()[-1])
        res["plonk_verify_stages"] = {
            lg: {k: {s: e["stages"].get(s) for s in ("asdl_challenges_ms_per_call", "asdl_terms_ms_per_call")} |
                 {"plonk_dev_event_ms_median": e["plonk_dev"]["event_ms_median"]} for k, e in by_k.items()}
            for lg, by_k in pv["lg_n"].items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
