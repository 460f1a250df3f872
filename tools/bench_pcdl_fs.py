"""Times pcdl::succinct_check from raw proofs (halo_pcdl_succinct_check_fs_batch, transcripts on the device) on
Pallas over a synthesized SRS, at lg n = 20 and 16 for k = 1, 64 and 4096 instances, beside the call it
builds on (halo_pcdl_succinct_check_batch, challenges given) and the only host sponge this repository has
(the Python restatement, oracle/poseidon.py).  DESIGN §4.7 records the numbers.

    python tools/bench_pcdl_fs.py [--launches 20] [--ks 1,2,4,8,16,64,4096] [--lgs 20,16] [--out FILE]

Per lg n and k, for a batch of plain instances and one of hiding instances:
  * the kernels' own times from the library's profiling hooks (pcdl_alpha, pcdl_challenges, pcdl_terms,
    lincomb_terms, lincomb_sum; means over the launches);
  * the event-timed median of the whole _dev call (inputs resident);
  * the wall time of the host-array call;
and, from the same session, the wall time of halo_pcdl_succinct_check_batch given precomputed challenges.
The instances are random scalars over tiled SRS points: every verdict is a rejection, and the work is that
of an accepting batch (no kernel's path depends on the verdict).  The host transcript is timed on one
instance per lg n and scaled by k; the crossover is the smallest measured k at which the device call
(challenges and check) takes less wall time than that plus halo_pcdl_succinct_check_batch.  The figure for
a native host sponge is an ESTIMATE from the multiplication count (NATIVE_NS_PER_MUL below), not a
measurement.  Prints one JSON line (and writes it to --out).
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
from halo_amd import group, schnorr  # noqa: E402

from bench_pcdl_check import dev, scalars, timed, wall  # noqa: E402

KERNELS = ("pcdl_alpha", "pcdl_challenges", "pcdl_terms", "lincomb_terms", "lincomb_sum")
MULS_PER_PERMUTATION = 55 * 21  # 55 rounds of three x^7 (4 each) and a 3 x 3 matrix
NATIVE_NS_PER_MUL = 25.0        # assumed cost of one 255-bit Montgomery multiplication on one CPU core (not measured)


def kernel_ms(L, fn, launches):
    """Per call: each kernel's own time summed over its launches in the call, mean over `launches` calls."""
    L.halo_profile_reset()
    L.halo_profile_enable(1)
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    L.halo_profile_enable(0)
    out = {}
    for name in KERNELS:
        n, ms = ctypes.c_size_t(0), ctypes.c_double(0)
        H.check(L.halo_profile_read(name.encode(), ctypes.byref(n), ctypes.byref(ms)))
        if n.value:
            out[name + "_ms_per_call"] = round(ms.value / launches, 4)
    L.halo_profile_reset()
    return out


class CountingSponge(poseidon.InnerSponge):
    permutations = 0

    def _permute(self):
        CountingSponge.permutations += 1
        super()._permute()


def host_transcript(lg, hiding, rng):
    """One instance's transcript with the Python restatement: (seconds, permutations)."""
    m, q = P.CURVES["pallas"].scalar, P.CURVES["pallas"].base
    ri = lambda mod: int.from_bytes(rng.bytes(32), "little") % mod  # noqa: E731
    pt = lambda: (ri(q), ri(q))  # noqa: E731  (the sponge absorbs coordinates; it never checks the curve)
    z, v = ri(m), ri(m)
    Ls, Rs = [pt() for _ in range(lg)], [pt() for _ in range(lg)]
    CountingSponge.permutations = 0
    t0 = time.perf_counter()
    t = poseidon.Sponge("pallas", poseidon.PCDL)
    t.inner = CountingSponge("fq")
    t.inner.absorb([poseidon.PCDL])
    if hiding:
        t.absorb_g([pt(), pt()])
        t.absorb_fr([z, v])
        t.challenge()
    t.absorb_g([pt()])
    t.absorb_fr([z, v])
    xi = t.challenge()
    for j in range(lg):
        t.absorb_fr([xi])
        t.absorb_g([Ls[j], Rs[j]])
        xi = t.challenge()
    return time.perf_counter() - t0, CountingSponge.permutations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--ks", default="1,2,4,8,16,64,4096")
    ap.add_argument("--lgs", default="20,16")
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
    lgs = [int(x) for x in a.lgs.split(",")]
    group.PublicParams.upload("pallas", base, S, Hh, precompute_windows=False)  # installs (S, H)
    group.PublicParams.synthesize("pallas", 1 << max(lgs), 7, precompute_windows=False)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    rng = np.random.default_rng(12)
    res = {"workload": "pcdl_succinct_check_fs", "curve": "pallas", "launches": a.launches,
           "device": torch.cuda.get_device_name(0), "muls_per_permutation": MULS_PER_PERMUTATION,
           "native_ns_per_mul_ASSUMED": NATIVE_NS_PER_MUL, "lg_n": {}}
    for lg in lgs:
        d = (1 << lg) - 1
        out_lg = {"k": {}, "host_transcript_python": {}}
        for hiding in (False, True):
            secs, perms = min(host_transcript(lg, hiding, rng) for _ in range(3))
            out_lg["host_transcript_python"]["hiding" if hiding else "plain"] = {
                "ms_per_instance": round(secs * 1e3, 3), "permutations": perms,
                "native_ms_per_instance_ESTIMATE": round(perms * MULS_PER_PERMUTATION * NATIVE_NS_PER_MUL * 1e-6, 4)}
        for k in [int(x) for x in a.ks.split(",")]:
            tile = lambda n: np.ascontiguousarray(np.tile(base, ((n + 63) // 64, 1))[:n])  # noqa: E731
            C, U, C_bar = tile(k), tile(k)[::-1].copy(), tile(k + 1)[1:].copy()
            Ls, Rs = tile(k * lg), tile(2 * k * lg)[k * lg:].copy()
            z, v, c, w_prime = scalars(rng, k), scalars(rng, k), scalars(rng, k), scalars(rng, k)
            hid = np.ones(k, dtype=np.uint8)
            xis, alphas, ok = np.zeros((k * (lg + 1), 4), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64), np.zeros(k, dtype=np.uint8)
            d_in = [dev(x) for x in (C, z, v, Ls, Rs, U, c)]
            d_hid = [torch.from_numpy(hid).cuda(), dev(C_bar), dev(w_prime)]
            d_xis = torch.zeros(k * (lg + 1) * 4, dtype=torch.int64, device="cuda")
            d_alpha = torch.zeros(k * 4, dtype=torch.int64, device="cuda")
            d_ok = torch.zeros(k, dtype=torch.uint8, device="cuda")
            reps = max(3, min(a.launches, 20 if k <= 64 else 5))
            entry = {}
            for hiding in (False, True):
                dh = d_hid if hiding else [None] * 3
                hh = [H.ptr(hid), H.ptr(C_bar), H.ptr(w_prime)] if hiding else [None] * 3

                def fs_dev():
                    H.check(L.halo_pcdl_succinct_check_fs_batch_dev(H.PALLAS, d, k, *[dp(t) for t in d_in], *[dp(t) for t in dh],
                                                                    dp(d_xis), dp(d_alpha), dp(d_ok), sp))

                def fs_host():
                    H.check(L.halo_pcdl_succinct_check_fs_batch(H.PALLAS, d, k, H.ptr(C), H.ptr(z), H.ptr(v), H.ptr(Ls), H.ptr(Rs),
                                                                H.ptr(U), H.ptr(c), *hh, H.ptr(xis), H.ptr(alphas), H.ptr(ok)))

                entry["hiding" if hiding else "plain"] = {"fs_dev": timed(fs_dev, a.launches),
                                                          "kernels": kernel_ms(L, fs_dev, a.launches),
                                                          "fs_host": wall(fs_host, reps)}
            # the call this one builds on, given the challenges the plain run just derived (never zero in practice)
            fs_host_plain = lambda: H.check(L.halo_pcdl_succinct_check_fs_batch(  # noqa: E731
                H.PALLAS, d, k, H.ptr(C), H.ptr(z), H.ptr(v), H.ptr(Ls), H.ptr(Rs), H.ptr(U), H.ptr(c), None, None, None,
                H.ptr(xis), None, H.ptr(ok)))
            fs_host_plain()
            ok_fs = ok.copy()

            def given_xis():
                H.check(L.halo_pcdl_succinct_check_batch(H.PALLAS, d, k, H.ptr(C), H.ptr(z), H.ptr(v), H.ptr(xis), H.ptr(Ls),
                                                         H.ptr(Rs), H.ptr(U), H.ptr(c), H.ptr(ok)))

            entry["succinct_check_batch_given_xis"] = wall(given_xis, reps)
            assert np.array_equal(ok, ok_fs), "the two calls disagree on the verdicts"
            py = out_lg["host_transcript_python"]["plain"]
            entry["host_python_transcripts_plus_check_ms"] = round(
                k * py["ms_per_instance"] + entry["succinct_check_batch_given_xis"]["wall_ms_median"], 3)
            entry["host_native_transcripts_plus_check_ms_ESTIMATE"] = round(
                k * py["native_ms_per_instance_ESTIMATE"] + entry["succinct_check_batch_given_xis"]["wall_ms_median"], 3)
            out_lg["k"][str(k)] = entry
            del d_in, d_hid, d_xis, d_alpha, d_ok
        ks = sorted(int(x) for x in out_lg["k"])
        fs = lambda k: out_lg["k"][str(k)]["plain"]["fs_host"]["wall_ms_median"]  # noqa: E731
        out_lg["crossover_k_vs_python_sponge"] = next(
            (k for k in ks if fs(k) < out_lg["k"][str(k)]["host_python_transcripts_plus_check_ms"]), None)
        out_lg["crossover_k_vs_native_sponge_ESTIMATE"] = next(
            (k for k in ks if fs(k) < out_lg["k"][str(k)]["host_native_transcripts_plus_check_ms_ESTIMATE"]), None)
        res["lg_n"][str(lg)] = out_lg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
