"""Mirror of ``PlonkProof::verify_succinct`` / ``verify`` (crates/plonk/src/plonk/protocol.rs:357-502) on the
MI355X backend: batches of raw proofs of one circuit, every Fiat-Shamir transcript (PLONK, PCDL, ASDL) derived
on the device (halo_plonk_verify_succinct_batch, halo_amd/csrc/plonk_verify.hip); ``verify_batch`` adds the deciders
of the batch's accumulators in the same call (halo_plonk_verify_batch, halo_amd/csrc/decider.hip).

Points are WrappedPoints (8 u64), scalars ark Montgomery limbs (4 u64), as everywhere in halo_amd.  The proofs
do not hide (naive_prover and acc::prover open with w = None).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _lib as H
from . import pcdl
from .group import _curve
from .pcdl import CheckFailed, Instance
from .prover import Q_POLYS, R_POLYS, S_POLYS, T_POLYS, W_POLYS

N_EVALS = W_POLYS + R_POLYS + Q_POLYS + T_POLYS + 2 * S_POLYS + 2 + 3  # HALO_PLONK_EVALS

# halo_plonk_verdict_t
ACCEPT, IDENTITY, INSTANCE_0, INSTANCE_1, INSTANCE_2, C_BAR, Z, V, MALFORMED, DECIDER_SUCCINCT, DECIDER = range(11)
IDENTITY_MSG = "T(𝔷) ≠ (F_GC(𝔷) + α F_CC1(𝔷) + α² F_CC2(𝔷) + α³ F_PL1(𝔷) + α⁴ F_PL2(𝔷)) / Zₕ(𝔷)"
MESSAGES = {IDENTITY: IDENTITY_MSG, INSTANCE_0: pcdl.SUCCINCT_MSG, INSTANCE_1: pcdl.SUCCINCT_MSG,
            INSTANCE_2: pcdl.SUCCINCT_MSG, C_BAR: "C_bar' ≠ C_bar", Z: "z' = z", V: "h(z) = v",
            MALFORMED: "malformed proof: a point off the curve or a zero denominator at xi",
            DECIDER_SUCCINCT: pcdl.SUCCINCT_MSG, DECIDER: pcdl.DECIDER_MSG}


class PlonkProofEvals(NamedTuple):
    """protocol.rs:36-46; every field (len, 4) ark scalars, z and z_omega (4,)."""
    ws: np.ndarray
    rs: np.ndarray
    qs: np.ndarray
    ts: np.ndarray
    ids: np.ndarray
    sigmas: np.ndarray
    z: np.ndarray
    z_omega: np.ndarray
    w_omegas: np.ndarray

    def flat(self) -> np.ndarray:
        """The 78 evaluations in struct order, the layout of halo_plonk_verify_succinct_batch's vs."""
        return np.concatenate([H.fe_array(x) for x in self]).reshape(N_EVALS, 4)


class PlonkProofCommitments(NamedTuple):
    """protocol.rs:49-53."""
    ws: np.ndarray
    ts: np.ndarray
    z: np.ndarray


class PlonkProofEvalProofs(NamedTuple):
    """protocol.rs:30-33: the EvalProof dicts (Ls, Rs, U, c) of instance_1 and instance_2."""
    r: dict
    r_omega: dict


class PlonkProof(NamedTuple):
    """protocol.rs:56-61; acc_next is the accumulator's ``pcdl.Instance``."""
    vs: PlonkProofEvals
    Cs: PlonkProofCommitments
    pis: PlonkProofEvalProofs
    acc_next: Instance

    @classmethod
    def from_prover(cls, out: dict, curve="pallas") -> "PlonkProof":
        """The proof of ``naive_prover(..., transcript=new_transcript)``'s result.  The prover evaluates all
        16 w_omegas; the proof keeps the first 3 (protocol.rs:45,323)."""
        m = pcdl._SCALAR[_curve(curve)]

        def fe(xs):  # canonical integers -> ark Montgomery limbs
            return np.stack([pcdl._ark_limbs(x % m * (1 << 256) % m) for x in xs])

        v = out["vs"]
        cuts = np.cumsum([0, W_POLYS, R_POLYS, Q_POLYS, T_POLYS, S_POLYS, S_POLYS])
        ws, rs, qs, ts, ids, sigmas = (fe(v[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
        z_at = int(cuts[-1])
        vs = PlonkProofEvals(ws, rs, qs, ts, ids, sigmas, fe([v[z_at]])[0], fe([v[-1]])[0],
                             fe(v[z_at + 1:z_at + 4]))

        def pi(q):
            return {"Ls": H.point_array(np.stack(q["Ls"])), "Rs": H.point_array(np.stack(q["Rs"])),
                    "U": H.point_array(q["U"]).reshape(8), "c": fe([q["c"]])[0], "C_bar": None, "w_prime": None}

        a = out["acc"]
        d = len(a["Ls"])
        acc_next = Instance(H.point_array(a["C"]).reshape(8), (1 << d) - 1, fe([a["z"]])[0], fe([a["v"]])[0], pi(a))
        return cls(vs, PlonkProofCommitments(H.point_array(np.stack(out["C_ws"])), H.point_array(np.stack(out["C_ts"])),
                                             H.point_array(out["C_z"]).reshape(8)),
                   PlonkProofEvalProofs(pi(out["q_r"]), pi(out["q_r_omega"])), acc_next)


class PlonkCircuit(NamedTuple):
    """What verify_succinct reads of PlonkCircuit: rows (a power of two), the selector commitments C_qs (10, 8),
    public_input_count and the scalar Poseidon MDS matrix (P::SCALAR_POSEIDON_MDS, (9, 4) ark scalars)."""
    rows: int
    C_qs: np.ndarray
    public_input_count: int
    mds: np.ndarray


def _check_counts(circuit: PlonkCircuit, public_inputs) -> list[np.ndarray]:
    """The ensure of protocol.rs:368, for every proof of the batch, before any device call."""
    rows = []
    for x in public_inputs:
        a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64)).reshape(-1, 4)
        if len(a) != circuit.public_input_count:
            raise CheckFailed("public_inputs.public_inputs.len() == circuit.public_input_count")
        rows.append(a)
    return rows


def pack_batch(circuit: PlonkCircuit, public_inputs, acc_prevs, proofs) -> dict:
    """The arrays of one halo_plonk_verify_succinct_batch call, by argument name."""
    k = len(proofs)
    lg = circuit.rows.bit_length() - 1
    pub = _check_counts(circuit, public_inputs)
    if not (len(pub) == len(acc_prevs) == k):
        raise ValueError("one public input vector and one acc_prev per proof")
    prevs = [Instance(*a) for a in acc_prevs]
    nexts = [Instance(*p.acc_next) for p in proofs]

    def pts(rows, shape):
        return np.ascontiguousarray(np.stack([H.point_array(r).reshape(shape) for r in rows]) if k else np.zeros((0,) + shape, np.uint64))

    def fes(rows, shape):
        return np.ascontiguousarray(np.stack([H.fe_array(r).reshape(shape) for r in rows]) if k else np.zeros((0,) + shape, np.uint64))

    three = [[a.pi, p.pis.r, p.pis.r_omega] for a, p in zip(prevs, proofs)]
    for row in three:
        for pi in row:
            if len(H.point_array(pi["Ls"])) != lg or len(H.point_array(pi["Rs"])) != lg:
                raise ValueError(f"an evaluation proof has {len(pi['Ls'])} rounds, {circuit.rows} rows need {lg}")
    return {
        "C_qs": H.point_array(circuit.C_qs).reshape(Q_POLYS, 8),
        "public_inputs": fes(pub, (circuit.public_input_count, 4)) if circuit.public_input_count else None,
        "C_ws": pts([p.Cs.ws for p in proofs], (W_POLYS, 8)), "C_z": pts([p.Cs.z for p in proofs], (8,)),
        "C_ts": pts([p.Cs.ts for p in proofs], (T_POLYS, 8)),
        "vs": fes([PlonkProofEvals(*p.vs).flat() for p in proofs], (N_EVALS, 4)),
        "Ls": pts([np.stack([H.point_array(pi["Ls"]) for pi in row]) for row in three], (3, lg, 8)),
        "Rs": pts([np.stack([H.point_array(pi["Rs"]) for pi in row]) for row in three], (3, lg, 8)),
        "U": pts([np.stack([H.point_array(pi["U"]).reshape(8) for pi in row]) for row in three], (3, 8)),
        "c": fes([np.stack([H.fe_array(pi["c"], 1)[0] for pi in row]) for row in three], (3, 4)),
        "acc_prev_C": pts([a.C for a in prevs], (8,)), "acc_prev_z": fes([a.z for a in prevs], (4,)),
        "acc_prev_v": fes([a.v for a in prevs], (4,)),
        "acc_next_C": pts([a.C for a in nexts], (8,)), "acc_next_z": fes([a.z for a in nexts], (4,)),
        "acc_next_v": fes([a.v for a in nexts], (4,)),
        "mds": H.fe_array(circuit.mds, 9),
    }


ARG_ORDER = ("C_ws", "C_z", "C_ts", "vs", "Ls", "Rs", "U", "c", "acc_prev_C", "acc_prev_z", "acc_prev_v", "acc_next_C",
             "acc_next_z", "acc_next_v", "mds")


def verify_succinct_batch(circuit: PlonkCircuit, public_inputs, acc_prevs, proofs, curve="pallas", readbacks: bool = False):
    """verify_succinct of k proofs of one circuit in one device call.  public_inputs: k vectors of
    circuit.public_input_count scalars; acc_prevs: k ``pcdl.Instance`` (PlonkPublicInputs.acc_prev).  Returns the k
    verdict bytes (0 = accept, else halo_plonk_verdict_t); with readbacks also challenges (k, 5, 4) = beta, gamma,
    alpha, zeta, xi, sides (k, 2, 4) = f and t z_H, asdl (k, 2, 4) = the accumulation's alpha and z'."""
    a = pack_batch(circuit, public_inputs, acc_prevs, proofs)
    k = len(proofs)
    verdict = np.zeros(k, dtype=np.uint8)
    if k == 0:
        return (verdict, np.zeros((0, 5, 4), np.uint64), np.zeros((0, 2, 4), np.uint64),
                np.zeros((0, 2, 4), np.uint64)) if readbacks else verdict
    H.ensure_device()
    chal = np.zeros((k, 5, 4), dtype=np.uint64) if readbacks else None
    sides = np.zeros((k, 2, 4), dtype=np.uint64) if readbacks else None
    asdl = np.zeros((k, 2, 4), dtype=np.uint64) if readbacks else None
    H.check(H.load().halo_plonk_verify_succinct_batch(
        _curve(curve), circuit.rows, k, H.ptr(a["C_qs"]), H.ptr(a["public_inputs"]), circuit.public_input_count,
        *[H.ptr(a[name]) for name in ARG_ORDER], H.ptr(verdict), H.ptr(chal), H.ptr(sides), H.ptr(asdl)))
    return (verdict, chal, sides, asdl) if readbacks else verdict


def verify_batch(circuit: PlonkCircuit, public_inputs, acc_prevs, proofs, rhos=None, curve="pallas",
                 bisect: bool = False) -> np.ndarray:
    """PlonkProof::verify (protocol.rs:493-502) of k proofs of one circuit in one device call
    (halo_plonk_verify_batch): verify_succinct, then acc::decider of every acc_next, whose PCDL transcript runs
    beside the proof's three instances.  rhos None: one commitment per decider; rhos "fs": one random linear
    combination of the deciders and one MSM under weights derived on the device from the batch (pcdl.decide_rho),
    with an exact rerun if it fails, or with bisect=True a bisection of the batch (pcdl.decide_batch); rhos (k, 4):
    the same under the caller's nonzero scalars, drawn AFTER the proofs were fixed.  Returns the k verdict bytes:
    the verify_succinct code if nonzero, else DECIDER_SUCCINCT, DECIDER or ACCEPT."""
    a = pack_batch(circuit, public_inputs, acc_prevs, proofs)
    k = len(proofs)
    verdict = np.zeros(k, dtype=np.uint8)
    if k == 0:
        return verdict
    lg = circuit.rows.bit_length() - 1
    pis = [Instance(*p.acc_next).pi for p in proofs]
    for pi in pis:
        if len(H.point_array(pi["Ls"])) != lg or len(H.point_array(pi["Rs"])) != lg:
            raise ValueError(f"acc_next's evaluation proof has {len(pi['Ls'])} rounds, {circuit.rows} rows need {lg}")
    nLs = np.ascontiguousarray(np.stack([H.point_array(pi["Ls"]).reshape(lg, 8) for pi in pis]))
    nRs = np.ascontiguousarray(np.stack([H.point_array(pi["Rs"]).reshape(lg, 8) for pi in pis]))
    nU = np.ascontiguousarray(np.stack([H.point_array(pi["U"]).reshape(8) for pi in pis]))
    nc = np.ascontiguousarray(np.stack([H.fe_array(pi["c"], 1)[0] for pi in pis]))
    rh, derive = H.fs_rhos(rhos, k)
    H.ensure_device()
    names = ARG_ORDER[:-1]  # mds comes after acc_next's evaluation proof
    with H.bisecting(bisect), H.deriving(derive):
        H.check(H.load().halo_plonk_verify_batch(
            _curve(curve), circuit.rows, k, H.ptr(a["C_qs"]), H.ptr(a["public_inputs"]), circuit.public_input_count,
            *[H.ptr(a[name]) for name in names], H.ptr(nLs), H.ptr(nRs), H.ptr(nU), H.ptr(nc), H.ptr(a["mds"]), H.ptr(rh),
            H.ptr(verdict)))
    return verdict


def verify_succinct(proof: PlonkProof, circuit: PlonkCircuit, public_inputs, acc_prev, curve="pallas") -> None:
    """protocol.rs:357-491 for one proof; raises CheckFailed with the reference's message."""
    code = int(verify_succinct_batch(circuit, [public_inputs], [acc_prev], [proof], curve)[0])
    if code != ACCEPT:
        raise CheckFailed(MESSAGES[code], code - INSTANCE_0 if INSTANCE_0 <= code <= INSTANCE_2 else None)


def verify(proof: PlonkProof, circuit: PlonkCircuit, public_inputs, acc_prev, curve="pallas") -> None:
    """protocol.rs:493-502: verify_succinct, then acc::decider of acc_next (pcdl::check with its transcript on
    the device)."""
    verify_succinct(proof, circuit, public_inputs, acc_prev, curve)
    a = Instance(*proof.acc_next)
    pcdl.check_device(a.C, a.d, a.z, a.v, a.pi, curve=_curve(curve))
