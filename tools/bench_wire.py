"""Times the wire format on the device (halo_amd/csrc/wire.hip) on Pallas over a synthesized SRS: what decoding
serialized instances costs beside the verifier that consumes them, and the square root alone.  DESIGN §4.13 and
README record the numbers.

    python tools/bench_wire.py [--reps 10] [--ks 1,64,4096] [--lgs 16,20] [--sqrt-only] [--out profiles/wire_bench.json]

Instance decode, per lg n and k, for hiding instances (44 points each at lg n = 20):
  (a) check_from_arrays   halo_pcdl_check_fs_batch_dev over decoded device arrays: the path that existed before the
                          wire format, and the yardstick;
  (b) check_from_bytes    halo_pcdl_instances_decode_dev and then the same call, from device bytes, on one stream;
  (c) decode_alone        halo_pcdl_instances_decode_dev alone.
Device-event times, medians of --reps after 2 warm-ups; (a) and (b) alternate inside one loop so that both see the
same machine.  decode_over_check = (c) / (a) is the figure the expectation "a root (~840 multiplications) is cheaper
than the ladder term the same point feeds" stands or falls by.  The instances are well-formed bytes over valid
points (the 64 reference SRS points, compressed by the library) and random scalars: every verdict is a rejection,
and no kernel's path depends on the verdict.  rho is given, so the decider is the combined one.

Standalone roots: halo_fe_sqrt_batch_dev over 2^20 random elements of Fq, roots per second from the event time.
Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from halo_amd import _lib as H  # noqa: E402
from halo_amd import group, schnorr, wire  # noqa: E402

from bench_pcdl_check import dev, scalars, timed  # noqa: E402


def instance_bytes(rng, recs, k, lg):
    """k hiding instances of lg rounds as one uint8 array: points drawn from the 64 records, random scalars."""
    d = (1 << lg) - 1
    size = 121 + 66 * lg + 65 + 2 + 65
    buf = np.zeros((k, size), dtype=np.uint8)
    pick = lambda j: recs[(np.arange(k) * 7 + j) % len(recs)]  # noqa: E731

    def scalar_bytes():
        s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F  # below the modulus
        return s

    u64 = lambda x: np.frombuffer(int(x).to_bytes(8, "little"), dtype=np.uint8)  # noqa: E731
    buf[:, 0:33] = pick(0)
    buf[:, 33:41] = u64(d)
    buf[:, 41:73], buf[:, 73:105] = scalar_bytes(), scalar_bytes()
    ls, rs = 113, 121 + 33 * lg
    buf[:, 105:113], buf[:, rs - 8:rs] = u64(lg), u64(lg)
    for j in range(lg):
        buf[:, ls + 33 * j: ls + 33 * j + 33] = pick(1 + j)
        buf[:, rs + 33 * j: rs + 33 * j + 33] = pick(1 + lg + j)
    u = rs + 33 * lg
    buf[:, u:u + 33] = pick(2 * lg + 1)
    buf[:, u + 33:u + 65] = scalar_bytes()
    buf[:, u + 65] = 1
    buf[:, u + 66:u + 99] = pick(2 * lg + 2)
    buf[:, u + 99] = 1
    buf[:, u + 100:u + 132] = scalar_bytes()
    assert u + 132 == size
    return buf.reshape(-1), np.arange(k, dtype=np.uint64) * np.uint64(size)


def alternating(fa, fb, reps, warmup=2):
    """Device-event medians of two calls timed in turn in one loop."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = []
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e0, e1, e2 in evs:
        e0.record()
        fa()
        e1.record()
        fb()
        e2.record()
    torch.cuda.synchronize()
    for which in (0, 1):
        ms = [e[which].elapsed_time(e[which + 1]) for e in evs]
        out.append({"event_ms_median": round(float(np.median(ms)), 4), "event_ms_min": round(min(ms), 4),
                    "event_ms_max": round(max(ms), 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", default="1,64,4096")
    ap.add_argument("--lgs", default="16,20")
    ap.add_argument("--sqrt-log", type=int, default=20)
    ap.add_argument("--sqrt-only", action="store_true", help="the standalone roots alone (the workload of tools/pmc_wire.sh)")
    ap.add_argument("--out")
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden.npz"))
    tr = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, tr[f"poseidon_{f}_mds"], tr[f"poseidon_{f}_rc"])
    base = g["ref_srs_pallas_b00_first64"]
    S, Hh = g["ref_sh_pallas"]
    lgs = [] if a.sqrt_only else [int(x) for x in a.lgs.split(",")]
    group.PublicParams.upload("pallas", base, S, Hh, precompute_windows=False)  # installs (S, H)
    if lgs:
        group.PublicParams.synthesize("pallas", 1 << max(lgs), 7, precompute_windows=False)
    recs = np.frombuffer(wire.compress_points(base, "pallas"), dtype=np.uint8).reshape(64, 33)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(13)
    res = {"workload": "wire", "curve": "pallas", "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "measured_on_gpu": True, "lg_n": {}}

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    for lg in lgs:
        d = (1 << lg) - 1
        out_lg = {}
        for k in [int(x) for x in a.ks.split(",")]:
            buf, offsets = instance_bytes(rng, recs, k, lg)
            d_bytes, d_off = torch.from_numpy(buf).cuda(), dev(offsets)
            words = lambda m, w: torch.zeros((m, w), dtype=torch.int64, device="cuda")  # noqa: E731
            flags = lambda: torch.zeros(k, dtype=torch.uint8, device="cuda")  # noqa: E731
            arrays = [words(k, 8), words(k, 4), words(k, 4), words(k * lg, 8), words(k * lg, 8), words(k, 8), words(k, 4), flags(),
                      words(k, 8), words(k, 4)]
            ptrs = [t.data_ptr() for t in arrays]
            d_ok, d_code, d_comb, d_rho = flags(), flags(), flags(), dev(scalars(rng, k) | np.uint64(1))

            def decode():
                H.check(L.halo_pcdl_instances_decode_dev(H.PALLAS, d, k, d_bytes.data_ptr(), len(buf), d_off.data_ptr(), *ptrs,
                                                         d_ok.data_ptr(), sp))

            def check():
                H.check(L.halo_pcdl_check_fs_batch_dev(H.PALLAS, d, k, *ptrs, d_rho.data_ptr(), d_code.data_ptr(),
                                                       d_comb.data_ptr(), sp))

            def from_bytes():
                decode()
                check()

            decode()
            torch.cuda.synchronize()
            assert bool(d_ok.all()), "the benchmark's own bytes did not decode"
            ta, tb = alternating(check, from_bytes, a.reps)
            tc = timed(decode, a.reps, warmup=2)
            points = k * (2 * lg + 4)
            out_lg[str(k)] = {
                "bytes": int(len(buf)), "points": points, "check_from_arrays": ta, "check_from_bytes": tb, "decode_alone": tc,
                "decode_over_check": round(tc["event_ms_median"] / ta["event_ms_median"], 4),
                "bytes_over_arrays": round(tb["event_ms_median"] / ta["event_ms_median"], 4),
                "decode_points_per_s": round(points / (tc["event_ms_median"] * 1e-3), 1)}
            del d_bytes, arrays, d_rho
        res["lg_n"][str(lg)] = out_lg
        flush()  # a long run leaves what it has measured so far
    n = 1 << a.sqrt_log
    xs = dev(scalars(rng, n))
    d_out, d_sq = torch.zeros((n, 4), dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    t = timed(lambda: H.check(L.halo_fe_sqrt_batch_dev(H.FQ, xs.data_ptr(), n, d_out.data_ptr(), d_sq.data_ptr(), sp)), a.reps,
              warmup=2)
    res["sqrt"] = {"field": "fq", "elements": n, **t, "roots_per_s": round(n / (t["event_ms_median"] * 1e-3), 1),
                   "squares": int(d_sq.sum())}
    print(json.dumps(res))
    flush()


if __name__ == "__main__":
    main()
