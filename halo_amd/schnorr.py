"""Mirror of crates/schnorr/src/lib.rs (hash_message, PublicKey::verify) and of the inner Poseidon
sponge (crates/poseidon/src/inner_sponge.rs) on the MI355X backend, as batches of independent items:
the reference's benchmark verifies 40 000 signatures in a parallel loop (crates/plonk/src/main.rs:35-47).

verify_batch's default is exact, one ladder per signature; with ``rhos`` it checks the whole batch by one MSM of
2 k + 1 terms under the caller's random weights or under weights derived from the batch (batch_weights), which the
reference does not have: an accept is then sound up to about k / 2^254, a reject is resolved exactly.

Signing and key generation stay with the caller (they need its RNG).  The Poseidon constants are the
caller's too (``PastaConfig::POSEIDON_*``): install them once per field with set_poseidon_params.
"""
from __future__ import annotations

import numpy as np

from . import _lib as H
from .group import _curve, _field


def set_poseidon_params(field, mds, rc) -> None:
    """Install the Poseidon parameters of `field`: mds (9, 4) row-major, rc (165, 4), ark Montgomery limbs
    (host-only; the hashing and Schnorr calls of that field need it first)."""
    mds, rc = H.fe_array(mds, 9), H.fe_array(rc, 165)
    H.check(H.load().halo_poseidon_set_params(_field(field), H.ptr(mds), H.ptr(rc)))


def poseidon_hash_batch(rows, field="fq") -> np.ndarray:
    """k independent inner sponges: rows (k, len, 4) -> absorb row i, squeeze once -> (k, 4)."""
    H.ensure_device()
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.uint64))
    assert rows.ndim == 3 and rows.shape[2] == 4, "rows: (k, len, 4) uint64"
    k, ln = rows.shape[0], rows.shape[1]
    out = np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_poseidon_hash_batch(_field(field), H.ptr(rows) if ln else None, ln, k, H.ptr(out)))
    return out


def _messages(msgs, k: int):
    msgs = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64))
    if msgs.size == 0:
        return None, 0
    msgs = msgs.reshape(k, -1, 4)
    return msgs, msgs.shape[1]


def hash_message_batch(pk, R, msgs, curve="pallas") -> np.ndarray:
    """lib.rs:24-35 ``hash_message`` for k (pk, R, message) triples: pk, R (k, 8) WrappedPoints, msgs
    (k, msg_len, 4) base-field elements -> (k, 4) scalars e."""
    H.ensure_device()
    pk, R = H.point_array(pk), H.point_array(R)
    k = len(pk)
    assert len(R) == k
    m, ml = _messages(msgs, k)
    out = np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_schnorr_hash_batch(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(m), ml, k, H.ptr(out)))
    return out


def verify_batch(pk, R, s, msgs, curve="pallas", rhos=None, return_combined=False):
    """lib.rs:71-79 ``PublicKey::verify`` for k signatures (R[i], s[i]) over msgs[i] under pk[i]:
    (k,) uint8, 1 = valid.  A pk or R that is neither (0, 0) nor on the curve gives 0.

    ``rhos`` (the convention of pcdl.decide_batch): None is the exact call, one ladder per signature.  A (k, 4) array
    of nonzero scalars, or "fs" for the weights of batch_weights, takes the combined pass instead
    (halo_schnorr_verify_combined): ONE MSM of 2 k + 1 terms, and only if that rejects the exact ladders, so the
    verdicts are per item either way.  The caller's weights must be drawn uniformly AFTER the signatures are fixed; an
    accept is then sound up to about k / 2^254 (derived weights: Q k / 2^254 over Q batches tried), a reject is exact.
    ``return_combined``: also return the combined pass's byte (1 = it held; None for the exact call)."""
    H.ensure_device()
    pk, R, s = H.point_array(pk), H.point_array(R), H.fe_array(s)
    k = len(pk)
    assert len(R) == k and len(s) == k
    m, ml = _messages(msgs, k)
    out = np.zeros(k, dtype=np.uint8)
    if rhos is None:
        H.check(H.load().halo_schnorr_verify_batch(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(out)))
        return (out, None) if return_combined else out
    rho, _ = H.fs_rhos(rhos, k)
    comb = np.zeros(1, dtype=np.uint8)
    H.check(H.load().halo_schnorr_verify_combined(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(rho),
                                                  H.ptr(out), H.ptr(comb)))
    return (out, int(comb[0])) if return_combined else out


def batch_weights(pk, R, s, msgs, curve="pallas") -> np.ndarray:
    """The weights that ``verify_batch(..., rhos="fs")`` runs under (halo_schnorr_batch_rho), derived on the device
    from the batch itself: (k, 4) scalars, 0 for an item whose pk or R is neither (0, 0) nor on the curve."""
    H.ensure_device()
    pk, R, s = H.point_array(pk), H.point_array(R), H.fe_array(s)
    k = len(pk)
    assert len(R) == k and len(s) == k
    m, ml = _messages(msgs, k)
    out = np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_schnorr_batch_rho(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(out)))
    return out
