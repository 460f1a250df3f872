"""Times the batched Schnorr verification (halo_schnorr_verify_batch_dev) and its hashing alone
(halo_schnorr_hash_batch_dev) on Pallas with 10-element messages, inputs resident on the device: the
reference's first benchmark (crates/plonk/src/main.rs:35-47, 40 000 x pk.verify; BASELINE.md: about
1300 signatures/s on its authors' CPU).

    python tools/bench_schnorr.py [--sizes 40000,1048576] [--launches 20] [--sweep] [--out FILE]

Per size and sponge layout (poseidon_lanes 1 and 3, alternated twice so the spread shows): warm-up, then
`launches` launches each bracketed by HIP events, and the wall time over the same batch of launches
(one synchronise before, one after).  64 distinct signatures made by the CPU restatement
(tests/schnorr_ref.py) are tiled to the batch size; every verdict is checked to be 1.  Prints one JSON
line (and writes it to --out).  --sweep adds hash-only timings at 2^15..2^19 (the layout threshold).
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

import pasta as P  # noqa: E402
import schnorr_ref as SR  # noqa: E402
from halo_amd import _lib as H  # noqa: E402
from halo_amd import schnorr  # noqa: E402

REFERENCE_SIGS_PER_S = 1300.0  # BASELINE.md:18 (the reference authors' CPU, all cores)
MSG_LEN = 10
SIMDS = 1024


def signatures(n_distinct: int):
    c = P.CURVES["pallas"]
    rng = np.random.default_rng(7)
    r = lambda m: int.from_bytes(rng.bytes(32), "little") % m  # noqa: E731
    items = []
    for _ in range(n_distinct):
        sk = r(c.scalar)
        msg = tuple(r(c.base) for _ in range(MSG_LEN))
        R, s = SR.sign("pallas", sk, r(c.scalar), msg)
        items.append((SR.public_key("pallas", sk), msg, R, s))
    assert all(SR.verify("pallas", *it) for it in items[:4])
    pk = SR.points("pallas", [it[0] for it in items])
    R = SR.points("pallas", [it[2] for it in items])
    s = SR.fe_rows([it[3] for it in items], c.scalar)
    msgs = np.array([SR.fe_rows(it[1], c.base) for it in items], dtype=np.uint64).reshape(n_distinct, MSG_LEN * 4)
    return pk, R, s, msgs


def tile(a, n):
    reps = (n + len(a) - 1) // len(a)
    return torch.from_numpy(np.ascontiguousarray(np.tile(a, (reps, 1))[:n]).view(np.int64)).cuda()


def timed(fn, launches: int, warmup: int = 3):
    """(per-launch event times in ms, wall ms per launch over the batch)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / launches
    return [a.elapsed_time(b) for a, b in ev], wall


def summary(ms, wall, n):
    med = float(np.median(ms))
    return {"event_ms_median": round(med, 4), "event_ms_min": round(min(ms), 4), "event_ms_max": round(max(ms), 4),
            "wall_ms_per_launch": round(wall, 4), "sigs_per_s": round(n / med * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40000,1048576")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    pk, R, s, msgs = signatures(64)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    res = {"workload": "schnorr_verify_batch", "curve": "pallas", "msg_len": MSG_LEN, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "reference_sigs_per_s": REFERENCE_SIGS_PER_S, "sizes": {}}
    sizes = [int(x) for x in a.sizes.split(",")]
    hash_only = [1 << e for e in range(15, 20)] if a.sweep else []
    for n in sizes + [x for x in hash_only if x not in sizes]:
        d_pk, d_R, d_s, d_m = tile(pk, n), tile(R, n), tile(s, n), tile(msgs, n)
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_e = torch.zeros((n, 4), dtype=torch.int64, device="cuda")

        def hash_():
            H.check(L.halo_schnorr_hash_batch_dev(H.PALLAS, dp(d_pk), dp(d_R), dp(d_m), MSG_LEN, n, dp(d_e), sp))

        def verify():
            H.check(L.halo_schnorr_verify_batch_dev(H.PALLAS, dp(d_pk), dp(d_R), dp(d_s), dp(d_m), MSG_LEN, n, dp(d_ok), sp))

        entry = {"waves": {"hash_1_lane": (n + 63) // 64, "hash_3_lanes": (n + 20) // 21, "ladder_quads": (n + 15) // 16,
                           "simds": SIMDS}}
        for rep in range(2):  # A B A B
            for lanes in (1, 3):
                with H.tuning(poseidon_lanes=lanes):
                    entry[f"hash_lanes{lanes}_run{rep}"] = summary(*timed(hash_, a.launches), n)
                    if n in sizes:
                        entry[f"verify_lanes{lanes}_run{rep}"] = summary(*timed(verify, a.launches), n)
        if n in sizes:
            verify()  # library default layout for this size
            torch.cuda.synchronize()
            assert bool((d_ok == 1).all()), "a valid signature was rejected"
            entry["hash_default"] = summary(*timed(hash_, a.launches), n)
            entry["verify_default"] = summary(*timed(verify, a.launches), n)
            entry["verify_default"]["vs_reference"] = round(entry["verify_default"]["sigs_per_s"] / REFERENCE_SIGS_PER_S)
        res["sizes"][str(n)] = entry
        del d_pk, d_R, d_s, d_m, d_ok, d_e
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
