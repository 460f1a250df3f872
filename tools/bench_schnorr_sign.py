"""Times batched Schnorr signing and key derivation on the generator's fixed-base comb (halo_generator_mul_batch_dev,
halo_schnorr_sign_batch_dev with and without pk) against the existing exact verifier (halo_schnorr_verify_batch_dev)
over the signatures just made, on Pallas with 10-element messages, inputs resident on the device.

    python tools/bench_schnorr_sign.py [--sizes 40000,1048576] [--launches 20] [--out profiles/schnorr_sign_bench.json]

Every key, nonce and message is distinct (random canonical limbs).  Per size: warm-up, then `launches` rounds; in each
round the five calls -- generator_mul, sign (pk derived), sign (pk given), hash alone, verify -- run one after the
other, each bracketed by HIP events, so they alternate in the same run and share whatever the clocks do.  Medians
are reported.  Every signature is checked to verify.  The table-build time is the first call of the process (k = 64)
less an identical second call.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from halo_amd import _lib as H  # noqa: E402
from halo_amd import schnorr  # noqa: E402

MSG_LEN = 10
OPS = ("generator_mul", "sign_derive_pk", "sign_given_pk", "hash", "verify")


def canonical(rng, *shape):
    """Random 4-limb values below 2^254, hence below both moduli: canonical ark limbs of distinct elements."""
    a = rng.integers(0, 2**64, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 62) - 1)
    return np.ascontiguousarray(a)


def cuda(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="40000,1048576")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schnorr_sign_bench.json"))
    a = ap.parse_args()
    H.ensure_device(0)
    L = H.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "transcript.npz"))
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rng = np.random.default_rng(113)

    # the table: first call of the process against an identical second one
    d_x = cuda(canonical(rng, 64))
    d_y = torch.zeros((64, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        H.check(L.halo_generator_mul_batch_dev(H.PALLAS, dp(d_x), 64, dp(d_y), sp))
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    res = {"workload": "schnorr_sign_batch", "curve": "pallas", "msg_len": MSG_LEN, "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "table": {"first_call_ms": round(t[0], 3), "second_call_ms": round(t[1], 3),
                                                              "build_ms": round(t[0] - min(t[1:]), 3)}, "sizes": {}}
    for n in [int(x) for x in a.sizes.split(",")]:
        d_sk, d_nonce, d_m = cuda(canonical(rng, n)), cuda(canonical(rng, n)), cuda(canonical(rng, n, MSG_LEN))
        d_pk = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        d_R = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        d_R2 = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        d_s = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        d_s2 = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        d_e = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        calls = {
            "generator_mul": lambda: L.halo_generator_mul_batch_dev(H.PALLAS, dp(d_sk), n, dp(d_pk), sp),
            "sign_derive_pk": lambda: L.halo_schnorr_sign_batch_dev(H.PALLAS, dp(d_sk), None, dp(d_nonce), dp(d_m), MSG_LEN, n,
                                                                    dp(d_R), dp(d_s), sp),
            "sign_given_pk": lambda: L.halo_schnorr_sign_batch_dev(H.PALLAS, dp(d_sk), dp(d_pk), dp(d_nonce), dp(d_m), MSG_LEN, n,
                                                                   dp(d_R2), dp(d_s2), sp),
            "hash": lambda: L.halo_schnorr_hash_batch_dev(H.PALLAS, dp(d_pk), dp(d_R), dp(d_m), MSG_LEN, n, dp(d_e), sp),
            "verify": lambda: L.halo_schnorr_verify_batch_dev(H.PALLAS, dp(d_pk), dp(d_R), dp(d_s), dp(d_m), MSG_LEN, n,
                                                              dp(d_ok), sp),
        }
        for _ in range(3):
            for op in OPS:
                H.check(calls[op]())
        torch.cuda.synchronize()
        assert bool((d_ok == 1).all()), "a signature made on the device was rejected"
        assert torch.equal(d_R, d_R2) and torch.equal(d_s, d_s2), "the two signing forms disagree"
        ev = {op: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
              for op in OPS}
        for i in range(a.launches):
            for op in OPS:
                ev[op][i][0].record()
                H.check(calls[op]())
                ev[op][i][1].record()
        torch.cuda.synchronize()
        entry = {}
        for op in OPS:
            ms = [x.elapsed_time(y) for x, y in ev[op]]
            med = float(np.median(ms))
            entry[op] = {"event_ms_median": round(med, 4), "event_ms_min": round(min(ms), 4), "event_ms_max": round(max(ms), 4),
                         "per_s": round(n / med * 1e3)}
        entry["sign_not_slower_than_verify"] = bool(entry["sign_derive_pk"]["event_ms_median"] <= entry["verify"]["event_ms_median"])
        entry["waves"] = {"comb_derive_pk": (2 * n + 63) // 64, "comb_given_pk": (n + 63) // 64, "verify_quads": (n + 15) // 16}
        res["sizes"][str(n)] = entry
        del d_sk, d_nonce, d_m, d_pk, d_R, d_R2, d_s, d_s2, d_e, d_ok
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
