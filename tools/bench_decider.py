"""Times the batched decider (halo_pcdl_decide_batch and its _dev form, halo_amd/csrc/decider.hip) on Pallas over a
synthesized SRS with its window-shifted copies, at lg n = 16 and 20 for k = 1, 64 and 4096 instances, beside the
route the parent commit offers: a loop of halo_pcdl_decider_commit with the comparison in numpy, measured in the
same session.  DESIGN §4.9 records the numbers.

    python tools/bench_decider.py [--reps 20] [--ks 1,64,4096] [--lgs 16,20] [--out profiles/decider_bench.json]
                                  [--budget-ms 4000] [--loop-max 256] [--modes combined]
    python tools/bench_decider.py --ks 64,4096 --out profiles/decider_bisect_bench.json --alternations 3 \
                                  --modes combined,combined_one_bad,bisect_one_bad,bisect_all_bad,one_bad_alternated
    python tools/bench_decider.py --ks 64,4096 --out profiles/decider_rho_bench.json --modes combined,derived,derived_alternated

Per lg n and k:
  * exact mode and combined mode (all valid): the event-timed median of the _dev call (inputs resident) and the
    wall time of the host-array call;
  * combined mode with one bad instance: the host-array call, which falls back to exact mode (wall time);
  * the stages from the library's profiling hooks, per call: "hpoly_rows", "hpoly_combine" (kernel times) and
    "decide_msm" (the span of the MSMs on the stream), with the number of "decide_msm" stages;
  * the parent's loop (wall time);
  * "bisect_one_bad": the same one-bad host call with the tuning key decide_bisect = 1 (the batch is bisected on the
    device instead of rerun in exact mode), with its stages; "bisect_all_bad" (k <= 64): every U wrong, bisected,
    beside exact mode on the same batch;
  * "one_bad_alternated": the two one-bad routes (key off, key on) alternated --alternations times, each a median,
    and whether their ranges are apart.
  * "derived" (k > 1): combined mode under the weights the device derives from the batch (tuning key decide_rho_fs = 1,
    rho NULL): the _dev call, the host-array call, the stages with "decide_rho" (the span of the derivation) and its
    kernels "rho_leaves", "rho_level" (ceil(lg k) launches), "rho_weights", and halo_pcdl_decide_rho_dev on its own;
    "derived_alternated": the _dev call with the caller's rho and with derived weights alternated --alternations
    times, each a median.
A library without a key (HALO_LIB pointing at an older build) can run every mode that does not set it.
Medians of --reps calls after warm-up; a call that takes longer than --budget-ms is repeated fewer times (at
least twice; the count is recorded).  The parent's loop over more than --loop-max instances is measured over
--loop-max of them and scaled, which the entry says.  The xi rows are random; min(k, 64) of them are distinct and
their commitments (from halo_pcdl_decider_commit, once) make every instance valid.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

import torch  # noqa: E402

from halo_amd import _lib as H  # noqa: E402
from halo_amd import group, pcdl, schnorr  # noqa: E402

from bench_pcdl_check import dev, scalars  # noqa: E402

STAGES = ("hpoly_rows", "hpoly_combine", "hpoly_segments", "lincomb_terms", "decide_msm", "decide_rho", "rho_leaves",
          "rho_level", "rho_weights")


def median_ms(fn, reps, budget_ms, events):
    """(median ms, min ms, calls measured): one warm-up call sizes the repetitions."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    n = reps if first * reps <= budget_ms else max(2, int(budget_ms / max(first, 1e-3)))
    n = min(n, reps)
    if first * 3 <= budget_ms:
        fn()
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        else:
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "calls": n}


def stages(L, fn):
    """The stage times of one call (halo_profile_*)."""
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    L.halo_profile_enable(0)
    out = {}
    for name in STAGES:
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        H.check(L.halo_profile_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        out[name] = {"launches": n.value, "ms": round(ms.value, 4)}
    L.halo_profile_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="1,64,4096")
    ap.add_argument("--lgs", default="16,20")
    ap.add_argument("--budget-ms", type=float, default=4000.0)
    ap.add_argument("--loop-max", type=int, default=256)
    ap.add_argument("--modes", default="exact,combined,combined_one_bad,parent_loop",
                    help="what to measure (an A/B of one stage needs only its mode)")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    modes = set(a.modes.split(","))
    H.ensure_device(0)
    L = H.load()
    lgs = [int(x) for x in a.lgs.split(",")]
    group.PublicParams.synthesize("pallas", 1 << max(lgs), 7, precompute_windows=True)
    if modes & {"derived", "derived_alternated"}:
        tr = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
        for f in ("fp", "fq"):
            schnorr.set_poseidon_params(f, tr[f"poseidon_{f}_mds"], tr[f"poseidon_{f}_rc"])
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    rng = np.random.default_rng(14)
    res = {"workload": "pcdl_decide_batch", "curve": "pallas", "reps": a.reps, "budget_ms": a.budget_ms,
           "device": torch.cuda.get_device_name(0), "srs": 1 << max(lgs),
           "decide_group_scalars": H.get_tuning("decide_group_scalars"), "msm_multi_max": H.get_tuning("msm_multi_max"),
           "lg_n": {}}
    for lg in lgs:
        d, row = (1 << lg) - 1, lg + 1
        distinct = 64
        xi_d = scalars(rng, distinct * row).reshape(distinct, row, 4)
        U_d = np.stack([pcdl.decider_commit(xi_d[i], d, curve="pallas") for i in range(distinct)])
        out_lg = {}
        for k in [int(x) for x in a.ks.split(",")]:
            idx = np.arange(k) % distinct
            xis, U = np.ascontiguousarray(xi_d[idx]), np.ascontiguousarray(U_d[idx])
            rho = scalars(rng, k)
            rho[:, 0] |= np.uint64(1)
            bad = U.copy()
            bad[k // 2] = U_d[(idx[k // 2] + 1) % distinct]  # a valid point, another instance's commitment
            all_bad = np.ascontiguousarray(U_d[(idx + 1) % distinct])
            one_bad = [0 if i == k // 2 else 1 for i in range(k)]
            ok = np.zeros(k, dtype=np.uint8)
            d_x, d_U, d_rho = dev(xis), dev(U), dev(rho)
            d_ok = torch.zeros(k, dtype=torch.uint8, device="cuda")
            d_c = torch.zeros(1, dtype=torch.uint8, device="cuda")

            def dev_call(with_rho):
                H.check(L.halo_pcdl_decide_batch_dev(H.PALLAS, d, k, dp(d_x), dp(d_U), None, dp(d_rho) if with_rho else None,
                                                     dp(d_ok), dp(d_c), sp))

            def host_call(with_rho, points):
                H.check(L.halo_pcdl_decide_batch(H.PALLAS, d, k, H.ptr(xis), H.ptr(points), None,
                                                 H.ptr(rho) if with_rho else None, H.ptr(ok)))

            m = min(k, a.loop_max)

            def parent_loop():
                return [np.array_equal(pcdl.decider_commit(xis[i], d, curve="pallas"), U[i]) for i in range(m)]

            entry = {}
            if "exact" in modes:
                entry["exact"] = {"dev_event": median_ms(lambda: dev_call(False), a.reps, a.budget_ms, True),
                                  "host_wall": median_ms(lambda: host_call(False, U), a.reps, a.budget_ms, False),
                                  "stages": stages(L, lambda: dev_call(False))}
                assert ok.tolist() == [1] * k and d_ok.cpu().numpy().tolist() == [1] * k
            if "combined" in modes:
                entry["combined"] = {"dev_event": median_ms(lambda: dev_call(True), a.reps, a.budget_ms, True),
                                     "host_wall": median_ms(lambda: host_call(True, U), a.reps, a.budget_ms, False),
                                     "stages": stages(L, lambda: dev_call(True))}
                assert ok.tolist() == [1] * k and (k == 1 or int(d_c.cpu()[0]) == 1)
            if "derived" in modes and k > 1:
                d_w = torch.zeros((k, 4), dtype=torch.int64, device="cuda")

                def rho_call():
                    H.check(L.halo_pcdl_decide_rho_dev(H.PALLAS, d, k, dp(d_x), dp(d_U), None, dp(d_w), sp))

                with H.deriving(True):
                    entry["derived"] = {"dev_event": median_ms(lambda: dev_call(False), a.reps, a.budget_ms, True),
                                        "host_wall": median_ms(lambda: host_call(False, U), a.reps, a.budget_ms, False),
                                        "stages": stages(L, lambda: dev_call(False))}
                assert ok.tolist() == [1] * k and int(d_c.cpu()[0]) == 1
                entry["derived"]["decide_rho_dev_event"] = median_ms(rho_call, a.reps, a.budget_ms, True)
                assert np.array_equal(d_w.cpu().numpy().view(np.uint64), pcdl.decide_rho(xis, U, d, curve="pallas"))
            if "derived_alternated" in modes and k > 1:
                runs = {"caller_rho": [], "derived": []}
                for _ in range(a.alternations):
                    for name, key in (("caller_rho", 0), ("derived", 1)):
                        with H.tuning(decide_rho_fs=key):
                            runs[name].append(median_ms(lambda: dev_call(key == 0), a.reps, a.budget_ms, True)["ms_median"])
                        assert int(d_c.cpu()[0]) == 1
                entry["derived_alternated"] = runs
            if "combined_one_bad" in modes:
                entry["combined_one_bad"] = {"host_wall": median_ms(lambda: host_call(True, bad), a.reps, a.budget_ms, False),
                                             "stages": stages(L, lambda: host_call(True, bad))}
                assert ok.tolist() == one_bad
            if "bisect_one_bad" in modes and k > 1:
                with H.tuning(decide_bisect=1):
                    entry["bisect_one_bad"] = {"host_wall": median_ms(lambda: host_call(True, bad), a.reps, a.budget_ms, False),
                                               "stages": stages(L, lambda: host_call(True, bad))}
                assert ok.tolist() == one_bad
            if "bisect_all_bad" in modes and 1 < k <= 64:
                with H.tuning(decide_bisect=1):
                    entry["bisect_all_bad"] = {"host_wall": median_ms(lambda: host_call(True, all_bad), a.reps, a.budget_ms, False),
                                               "stages": stages(L, lambda: host_call(True, all_bad))}
                assert ok.tolist() == [0] * k
                entry["exact_all_bad"] = {"host_wall": median_ms(lambda: host_call(False, all_bad), a.reps, a.budget_ms, False)}
                assert ok.tolist() == [0] * k
            if "one_bad_alternated" in modes and k > 1:
                runs = {"exact_rerun": [], "bisect": []}
                for _ in range(a.alternations):
                    for name, key in (("exact_rerun", 0), ("bisect", 1)):
                        with H.tuning(decide_bisect=key):
                            runs[name].append(median_ms(lambda: host_call(True, bad), a.reps, a.budget_ms, False)["ms_median"])
                        assert ok.tolist() == one_bad
                runs["apart"] = max(runs["bisect"]) < min(runs["exact_rerun"])
                entry["one_bad_alternated"] = runs
            if "parent_loop" in modes:
                loop = median_ms(parent_loop, a.reps, a.budget_ms, False)
                assert all(parent_loop())
                if m < k:
                    loop = {"ms_median": round(loop["ms_median"] * k / m, 4), "ms_min": round(loop["ms_min"] * k / m, 4),
                            "calls": loop["calls"], "scaled_from_instances": m}
                entry["parent_loop_wall"] = loop
            out_lg[str(k)] = entry
            del d_x, d_U, d_rho, d_ok, d_c
        res["lg_n"][str(lg)] = out_lg
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
