"""Times the PCDL verifier's device path at lg n = 20 (t = 2 lg n + 2 = 42 terms per instance) on Pallas over
a synthesized SRS, for k = 1, 3, 64 and 4096 instances, and the two comparisons DESIGN §4.7 records:

  (a) the batched linear combination (halo_point_lincomb_batch, host arrays) against the only other device
      route to the same arithmetic: halo_curve_op op 2 over the k t terms, then halo_point_sum_rows_dev;
  (b) the term kernel's time per term at 2^16 terms (halo_profile_read "lincomb_terms") -- to be set
      against the ladder share per signature of k_schnorr_verify at 2^16 signatures (verification minus
      hashing, tools/bench_schnorr.py --sizes 65536, run in the same session).

    python tools/bench_pcdl_check.py [--launches 20] [--ks 1,3,64,4096] [--out FILE]

Per k: event-timed medians of halo_point_lincomb_batch_dev (inputs resident), the kernels' own times from
the library's profiling hooks, wall times of the host-array calls, and for k = 1 and 3 the wall time of
pcdl.succinct_check_many (host transcript included; a stand-in sponge, so the verdict is a rejection:
the work is the same).  The timed points are 64 SRS points tiled and the scalars are random, which is all
the ladder's cost depends on.  Prints one JSON line (and writes it to --out).
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

from halo_amd import _lib as H  # noqa: E402
from halo_amd import group, pcdl  # noqa: E402

LG_N = 20
T = 2 * LG_N + 2


def scalars(rng, n):
    a = rng.integers(0, 2**64 - 1, size=(n, 4), dtype=np.uint64, endpoint=True)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)  # below the modulus
    return np.ascontiguousarray(a)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def timed(fn, launches, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"event_ms_median": round(float(np.median(ms)), 4), "event_ms_min": round(min(ms), 4),
            "event_ms_max": round(max(ms), 4)}


def wall(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms_median": round(float(np.median(ts)), 4), "wall_ms_min": round(min(ts), 4)}


def kernel_ms(L, fn, launches):
    """Mean of each kernel's own time over `launches` calls (halo_profile_*)."""
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    L.halo_profile_enable(0)
    out = {}
    for name in ("lincomb_terms", "lincomb_sum"):
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        H.check(L.halo_profile_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        out[name + "_ms_mean"] = round(ms.value / max(n.value, 1), 4)
    L.halo_profile_reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--ks", default="1,3,64,4096")
    ap.add_argument("--out")
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    base = g["ref_srs_pallas_b00_first64"]
    S, Hh = g["ref_sh_pallas"]
    group.PublicParams.upload("pallas", base, S, Hh, precompute_windows=False)  # installs (S, H)
    group.PublicParams.synthesize("pallas", 1 << LG_N, 7, precompute_windows=False)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.default_rng(11)
    res = {"workload": "pcdl_succinct_check", "curve": "pallas", "lg_n": LG_N, "terms_per_instance": T,
           "launches": a.launches, "device": torch.cuda.get_device_name(0), "k": {}}

    def lincomb_case(k, t):
        n = k * t
        pts = np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1))[:n])
        sc = scalars(rng, n)
        add = np.ascontiguousarray(np.tile(base[::-1], ((k + 63) // 64, 1))[:k])
        return pts, sc, add

    for k in [int(x) for x in a.ks.split(",")]:
        pts, sc, add = lincomb_case(k, T)
        n = k * T
        d_pts, d_sc, d_add = dev(pts), dev(sc), dev(add)
        d_out = torch.zeros(k * 16, dtype=torch.int64, device="cuda")
        d_id = torch.zeros(k, dtype=torch.uint8, device="cuda")
        out = np.zeros((k, 8), dtype=np.uint64)

        def lincomb_dev():
            H.check(L.halo_point_lincomb_batch_dev(H.PALLAS, dp(d_add), dp(d_pts), dp(d_sc), k, T, dp(d_out), dp(d_id), sp))

        def lincomb_host():
            H.check(L.halo_point_lincomb_batch(H.PALLAS, H.ptr(add), H.ptr(pts), H.ptr(sc), k, T, H.ptr(out)))

        # route (a): one scalar multiplication per term through halo_curve_op, then the row sums
        terms = np.zeros((n, 8), dtype=np.uint64)
        d_rows = torch.zeros(k * 8, dtype=torch.int64, device="cuda")

        def old_route():
            H.check(L.halo_curve_op(H.PALLAS, 2, H.ptr(pts), None, H.ptr(sc), n, H.ptr(terms)))
            d_terms = dev(terms)
            H.check(L.halo_point_sum_rows_dev(H.PALLAS, dp(d_terms), k, T, dp(d_rows), sp))
            torch.cuda.synchronize()

        reps = max(3, min(a.launches, 20 if k <= 64 else 5))
        entry = {"terms": n, "term_waves": (n + 15) // 16,
                 "lincomb_dev": timed(lincomb_dev, a.launches), "lincomb_kernels": kernel_ms(L, lincomb_dev, a.launches),
                 "lincomb_host": wall(lincomb_host, reps), "curve_op_then_sum_rows": wall(old_route, reps)}
        # the two routes agree up to the addend, which the old route has no slot for
        lincomb_host()
        got = out.copy()
        H.check(L.halo_point_lincomb_batch(H.PALLAS, None, H.ptr(pts), H.ptr(sc), k, T, H.ptr(out)))
        old_route()
        rows = np.ascontiguousarray(d_rows.cpu().numpy().view(np.uint64)).reshape(k, 8)
        assert np.array_equal(rows, out), "the two routes disagree"
        assert not np.array_equal(got, out)
        entry["new_over_old"] = round(entry["lincomb_host"]["wall_ms_median"] / entry["curve_op_then_sum_rows"]["wall_ms_median"], 4)
        # the whole check call: host scalar work, copies, the two launches
        Cp, U = add, np.ascontiguousarray(pts[:k])
        z, v, c = scalars(rng, k), scalars(rng, k), scalars(rng, k)
        xis = scalars(rng, k * (LG_N + 1))
        xis[:, 0] |= np.uint64(1)  # nonzero
        Ls, Rs = np.ascontiguousarray(pts[: k * LG_N]), np.ascontiguousarray(pts[k * LG_N: 2 * k * LG_N])
        ok = np.zeros(k, dtype=np.uint8)

        def check_call():
            H.check(L.halo_pcdl_succinct_check_batch(H.PALLAS, (1 << LG_N) - 1, k, H.ptr(Cp), H.ptr(z), H.ptr(v), H.ptr(xis),
                                                     H.ptr(Ls), H.ptr(Rs), H.ptr(U), H.ptr(c), H.ptr(ok)))

        entry["succinct_check_batch"] = wall(check_call, reps)
        if k <= 3:  # the latency of a check from Python, the caller's (stand-in) transcript included
            insts = [pcdl.Instance(Cp[i], (1 << LG_N) - 1, z[i], v[i],
                                   {"Ls": Ls[i * LG_N: (i + 1) * LG_N], "Rs": Rs[i * LG_N: (i + 1) * LG_N], "U": U[i], "c": c[i],
                                    "C_bar": None, "w_prime": None}) for i in range(k)]

            def py_check():
                try:
                    pcdl.succinct_check_many(insts, [pcdl.StandInTranscript("pallas") for _ in range(k)], "pallas")
                except pcdl.CheckFailed:
                    pass

            entry["python_succinct_check"] = wall(py_check, reps)
        res["k"][str(k)] = entry
        del d_pts, d_sc, d_add, d_out, d_id, d_rows
    # (b) 2^16 terms, one per item: the term kernel alone
    k = 1 << 16
    pts, sc, _ = lincomb_case(k, 1)
    d_pts, d_sc = dev(pts), dev(sc)
    d_out = torch.zeros(k * 16, dtype=torch.int64, device="cuda")

    def terms_only():
        H.check(L.halo_point_lincomb_batch_dev(H.PALLAS, None, dp(d_pts), dp(d_sc), k, 1, dp(d_out), None, sp))

    e = {"terms": k, "lincomb_dev": timed(terms_only, a.launches), "lincomb_kernels": kernel_ms(L, terms_only, a.launches)}
    e["ns_per_term"] = round(e["lincomb_kernels"]["lincomb_terms_ms_mean"] * 1e6 / k, 2)
    res["terms_65536"] = e
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
