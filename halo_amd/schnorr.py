"""Mirror of crates/schnorr/src/lib.rs (hash_message, PublicKey::verify) and of the inner Poseidon
sponge (crates/poseidon/src/inner_sponge.rs) on the MI355X backend, as batches of independent items:
the reference's benchmark verifies 40 000 signatures in a parallel loop (crates/plonk/src/main.rs:35-47).

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


def verify_batch(pk, R, s, msgs, curve="pallas") -> np.ndarray:
    """lib.rs:71-79 ``PublicKey::verify`` for k signatures (R[i], s[i]) over msgs[i] under pk[i]:
    (k,) uint8, 1 = valid.  A pk or R that is neither (0, 0) nor on the curve gives 0."""
    H.ensure_device()
    pk, R, s = H.point_array(pk), H.point_array(R), H.fe_array(s)
    k = len(pk)
    assert len(R) == k and len(s) == k
    m, ml = _messages(msgs, k)
    out = np.zeros(k, dtype=np.uint8)
    H.check(H.load().halo_schnorr_verify_batch(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(out)))
    return out
