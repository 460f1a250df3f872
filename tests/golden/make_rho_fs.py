#!/usr/bin/env python3
"""Regenerate tests/golden/rho_fs.npz (committed): the derived decider weights of tests/rho_ref.py on fixed batches,
so that a change of the definition shows as a diff of the fixture and a failing tests/test_rho_plan.py.

    python3 tests/golden/make_rho_fs.py

Per curve and case name (k, lg n, live mask or none) -- k1_lg0, k2_lg1, k3_lg3, k5_lg3, k5_lg3_live (1, 0, 1, 1, 0):
  {curve}_{case}_xis   (k, lg n + 1, 4)  ark scalars
  {curve}_{case}_U     (k, 8)            WrappedPoints: multiples of the generator, the second one the identity
  {curve}_{case}_live  (k,)              uint8, all ones where the case has no mask
  {curve}_{case}_rho   (k, 4)            rho_ref.weights of the above
The inputs are functions of the case alone (numpy's default_rng with a fixed seed).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import pasta as P  # noqa: E402
import rho_ref  # noqa: E402

CASES = {"k1_lg0": (1, 0, None), "k2_lg1": (2, 1, None), "k3_lg3": (3, 3, None), "k5_lg3": (5, 3, None),
         "k5_lg3_live": (5, 3, [1, 0, 1, 1, 0])}


def det_scalars(seed: int, k: int) -> np.ndarray:
    """k Montgomery-form scalars below 2^254 (tests/golden/make_transcript.py)."""
    a = np.random.default_rng(seed).integers(0, 2**64 - 1, size=(k, 4), dtype=np.uint64, endpoint=True)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return np.ascontiguousarray(a)


def inputs(cname: str, case: str):
    k, lg, live = CASES[case]
    cv = P.CURVES[cname]
    seed = 9000 + 10 * sorted(CASES).index(case) + (cname == "vesta")
    xis = det_scalars(seed, k * (lg + 1)).reshape(k, lg + 1, 4)
    pts = [None if i == 1 else P.mul_fast(cv, 3 + 7 * i + seed, cv.generator) for i in range(k)]
    U = np.array([P.point_to_wrapped(cv, p) for p in pts], dtype=np.uint64)
    return xis, U, np.array(live if live is not None else [1] * k, dtype=np.uint8), (1 << lg) - 1, live


def main():
    out = {}
    for cname in ("pallas", "vesta"):
        for case in CASES:
            xis, U, lv, d, live = inputs(cname, case)
            out[f"{cname}_{case}_xis"], out[f"{cname}_{case}_U"], out[f"{cname}_{case}_live"] = xis, U, lv
            out[f"{cname}_{case}_rho"] = rho_ref.weights(cname, xis, U, d, live)
    np.savez_compressed(os.path.join(HERE, "rho_fs.npz"), **out)


if __name__ == "__main__":
    main()
