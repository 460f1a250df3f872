"""Writes tests/golden/plonk_proofs.npz: two-step proof chains of tests/plonk_ref.satisfiable_circuit made by
halo_amd.prover.naive_prover on the CPU backend under the reference's transcripts (proof 2's acc_prev is proof
1's acc_next; the first acc_prev is acc::prover of one fresh opening), with the restated verifier's challenges,
sides and accumulation challenges.  Chains: Pallas n = 8 and n = 64, Vesta n = 16.

Reads only tests/golden/golden.npz (the SRS recipe's first 64 points, S and H) and tests/golden/transcript.npz
(the Poseidon constants, through oracle/poseidon.py).  Run from the repository root:
    python tests/golden/make_plonk_proofs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import plonk_ref as R  # noqa: E402  (puts the repository root and oracle/ on the path)
import pasta as P  # noqa: E402

CHAINS = [("pallas", 8), ("pallas", 64), ("vesta", 16)]
FIELDS = [f for f in R.Rec._fields if f != "next_pi"]


def main():
    golden = np.load(os.path.join(HERE, "golden.npz"))
    out = {}
    for cname, n in CHAINS:
        srs = np.ascontiguousarray(golden[f"ref_srs_{cname}_b00_first64"])
        S, H = golden[f"ref_sh_{cname}"]
        C_qs, recs = R.prove_chain(cname, n, srs, S, H, steps=2, seed=n)
        key = f"{cname}_n{n}"
        m = P.CURVES[cname].scalar
        out[f"{key}_C_qs"] = C_qs
        for step, rec in enumerate(recs):
            code, rb = R.verify_succinct(cname, n, C_qs, H, rec)
            assert code == R.ACCEPT, (key, step, code)
            assert R.verify(cname, n, C_qs, H, rec, srs) == (R.ACCEPT, ""), (key, step)
            for f in FIELDS:
                out[f"{key}_{step}_{f}"] = getattr(rec, f)
            for j, name in enumerate(("Ls", "Rs", "U", "c")):
                out[f"{key}_{step}_next_pi_{name}"] = rec.next_pi[j]
            for name in ("challenges", "sides", "asdl"):
                out[f"{key}_{step}_{name}"] = np.stack([R.fe(x, m) for x in rb[name]])
            print(key, step, "accepted;", sum(1 for w in rec.C_ts if not w.any()), "identity C_ts")
    path = os.path.join(HERE, "plonk_proofs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
